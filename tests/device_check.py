"""Exact checks of tables that are too large for the CPU oracle, with torch on the
device that holds them (or on the CPU: tests/test_device_check.py).  TEST
INFRASTRUCTURE (the checker, never the thing checked): a restatement of the
reference's own linear-time checkers

  gt_suftab_lightweightcheck   src/match/sfx-lwcheck.c:181-337
  gt_lcptab_lightweightcheck   src/match/sfx-linlcp.c:548

for tables in device memory; check_lcp_exact turns Kasai's inheritance argument
into a check of every .lcp and .llv entry.  Sortedness of a suffix array is a LOCAL property
once it is a permutation: with rank = its inverse,

    suffix SA[i-1] < suffix SA[i]   for all i
  <=>  for all i:  c(SA[i-1]) < c(SA[i])  or
                   c(SA[i-1]) = c(SA[i]) is a letter and rank[SA[i-1]+1] < rank[SA[i]+1]

(induction over the common prefix), where c(p) is the letter at p, or -- special
symbols being unique and larger than every letter, larger at larger positions
(src/core/encseq.h:640, src/match/sfx-bentsedg.c:75-80) -- 256 + p.
"""
import numpy as np
import torch

CHUNK = 1 << 27


def _chunks(n, step=CHUNK):
    for a in range(0, n, step):
        yield a, min(n, a + step)


def suffix_ranks(sa):
    """the inverse of a suffix table that is a permutation of [0, n]: (rank, "") with
    rank an int64 tensor of N entries on the table's device, or (None, message)"""
    N = sa.numel()
    n = N - 1
    dev = sa.device
    rank = torch.empty(N, dtype=torch.int64, device=dev)
    rank.fill_(-1)
    for a, b in _chunks(N):
        p = sa[a:b]
        if int(p.min()) < 0 or int(p.max()) > n:
            return None, "entry outside [0, n] in [%d, %d)" % (a, b)
        rank[p] = torch.arange(a, b, dtype=torch.int64, device=dev)
    for a, b in _chunks(N):
        if not bool((sa[rank[a:b]] == torch.arange(a, b, dtype=torch.int64, device=dev)).all()):
            return None, "not a permutation (positions [%d, %d))" % (a, b)
    return rank, ""


def check_suffix_array_exact(sa, enc, rank=None):
    """sa: int64 device tensor, N = n + 1 entries; enc: uint8 device tensor, n
    encoded symbols; rank: suffix_ranks(sa) when the caller keeps it for
    check_lcp_exact.  Returns (ok, message)."""
    N = sa.numel()
    n = N - 1
    if rank is None:
        rank, msg = suffix_ranks(sa)
        if rank is None:
            return False, msg
    # ---- order of every pair of neighbours
    def c_of(p):
        sym = torch.where(p < n, enc[torch.clamp(p, max=n - 1)].to(torch.int64),
                          torch.full_like(p, 255))
        return torch.where(sym >= 254, 256 + p, sym)
    for a, b in _chunks(N - 1):
        p, q = sa[a:b], sa[a + 1:b + 1]
        cp, cq = c_of(p), c_of(q)
        rp = rank[torch.clamp(p + 1, max=n)]
        rq = rank[torch.clamp(q + 1, max=n)]
        ok = (cp < cq) | ((cp == cq) & (cp < 254) & (rp < rq))
        if not bool(ok.all()):
            i = int(torch.nonzero(~ok)[0].item()) + a + 1
            return False, "suffixes out of order at table index %d" % i
    return True, ""


def check_bwt_exact(sa, enc, bwt):
    N = sa.numel()
    for a, b in _chunks(N):
        p = sa[a:b]
        want = torch.where(p > 0, enc[torch.clamp(p - 1, min=0)], torch.full_like(p, 254, dtype=torch.uint8))
        if not bool((want == bwt[a:b]).all()):
            i = int(torch.nonzero(want != bwt[a:b])[0].item()) + a
            return False, "bwt differs at table index %d" % i
    return True, ""


LCP_CHUNK = 1 << 21          # text positions per step of check_lcp_exact
SWEEP = 1 << 25              # symbol pairs per sweep of its part (b)


def _sym(enc, i):
    """the symbols at positions i (int64), 255 (a special) at and beyond the end"""
    n = enc.numel()
    return torch.where(i < n, enc[torch.clamp(i, max=n - 1)],
                       torch.full_like(i, 255, dtype=torch.uint8))


def check_lcp_exact(sa, enc, lcp, llv_idx, llv_val, rank=None):
    """EVERY entry of .lcp and .llv, in time linear in n: Kasai's inheritance
    argument (the reference's src/match/sfx-linlcp.c) turned into a check.  Only
    for a suffix table that check_suffix_array_exact has accepted; rank: its
    suffix_ranks(sa) if the caller has it.

    C[i] is the claimed LCP of table index i (the byte, the .llv value where the
    byte is 255), PLCP[p] = C[rank[p]], phi(p) = sa[rank[p] - 1].  For every
    position p with rank[p] >= 1:
      (a) suffixes p and phi(p) differ at offset PLCP[p] (different symbols, a
          special or the end on either side): true LCP <= claim;
      (b) they hold equal letters at every offset in [s, PLCP[p]), with
          s = max(PLCP[p-1] - 1, 0) (0 for p = 0 or rank[p-1] = 0): suffixes
          phi(p-1)+1 and p share PLCP[p-1] - 1 symbols and phi(p) lies between
          them in the table, so by induction over p the offsets below s agree:
          true LCP >= claim.
    (b) compares sum(max(0, PLCP[p] - PLCP[p-1] + 1)) <= 2N symbol pairs."""
    N = sa.numel()
    n = N - 1
    dev = sa.device
    # ---- .llv: exactly the table indices whose byte is 255, ascending
    m = llv_idx.numel()
    if int(lcp[0].item()) != 0:
        return False, "lcp byte at table index 0 is %d" % int(lcp[0].item())
    overflows = count_lcp_overflows(lcp)
    if overflows != m:
        return False, "%d lcp bytes of 255, %d .llv entries" % (overflows, m)
    if m > 0:
        if not bool((llv_idx[1:] > llv_idx[:-1]).all()):
            return False, ".llv indices not ascending"
        if int(llv_idx[0].item()) < 1 or int(llv_idx[-1].item()) > n:
            return False, ".llv index outside [1, n]"
        for a, b in _chunks(m):
            i, v = llv_idx[a:b], llv_val[a:b]
            if not bool((lcp[i] == 255).all()):
                return False, ".llv entry where the lcp byte is not 255"
            if int(v.min().item()) < 255 or int(v.max().item()) > n:
                return False, ".llv value outside [255, n]"
    if rank is None:
        rank, msg = suffix_ranks(sa)
        if rank is None:
            return False, msg

    def claims(r):
        c = lcp[r].to(torch.int64)
        big = c == 255
        c[big] = llv_val[torch.searchsorted(llv_idx, r[big])]
        return c

    def report(p, q, r, claim, at, what):
        return False, "lcp at table index %d (suffixes %d, %d) is %d, %s at offset %d" % (
            r, q, p, claim, what, at)

    for a, b in _chunks(N, LCP_CHUNK):
        lo = max(a - 1, 0)              # (PLCP[a - 1] gives the start of (b) at a)
        r = rank[lo:b]
        has = r >= 1
        rc = torch.clamp(r, min=1)
        plcp = torch.where(has, claims(rc), torch.zeros_like(r))
        phi = sa[rc - 1]
        s = torch.zeros_like(plcp)
        s[1:] = torch.where(has[:-1], torch.clamp(plcp[:-1] - 1, min=0), s[1:])
        k = a - lo
        p = torch.arange(a, b, dtype=torch.int64, device=dev)
        r, has, plcp, phi, s = r[k:], has[k:], plcp[k:], phi[k:], s[k:]
        # (a) the first offset where the two differ is the claim
        va, vb = _sym(enc, p + plcp), _sym(enc, phi + plcp)
        bad = has & (va == vb) & (va < 254)
        if bool(bad.any()):
            j = int(torch.nonzero(bad)[0].item())
            return report(a + j, int(phi[j]), int(r[j]), int(plcp[j]), int(plcp[j]), "they agree")
        # (b) equal letters in [s, claim), sweeps of 16 symbols that double, up to
        # 16 K, while the positions still open fit SWEEP
        act = torch.nonzero(has & (plcp > s)).flatten()
        cur, end, pa, qa = s[act], plcp[act], p[act], phi[act]
        w = 16
        while act.numel() > 0:
            o = cur[:, None] + torch.arange(w, dtype=torch.int64, device=dev)[None, :]
            xa, xb = _sym(enc, pa[:, None] + o), _sym(enc, qa[:, None] + o)
            bad = (o < end[:, None]) & ((xa != xb) | (xa >= 254))
            if bool(bad.any()):
                j, t = (int(x) for x in torch.nonzero(bad)[0])
                return report(int(pa[j]), int(qa[j]), int(rank[pa[j]]), int(end[j]), int(o[j, t]),
                              "they differ")
            cur = cur + w
            keep = cur < end
            act, cur, end, pa, qa = act[keep], cur[keep], end[keep], pa[keep], qa[keep]
            w = min(2 * w, 1 << 14)
            while w > 16 and act.numel() * w > SWEEP:
                w //= 2
    return True, ""


def check_llv_all(sa, enc, lcp, llv_idx, llv_val, rng_seed=1, probes=16):
    """EVERY .llv entry: index ascending, byte 255 in the table, the suffixes
    differ (or one ends / meets a special) exactly at offset value, agree at value-1
    and at `probes` random offsets below"""
    m = llv_idx.numel()
    n = enc.numel()
    if m == 0:
        return True, ""
    if not bool((llv_idx[1:] > llv_idx[:-1]).all()):
        return False, ".llv indices not ascending"
    g = torch.Generator(device=sa.device)
    g.manual_seed(rng_seed)
    for a, b in _chunks(m, 1 << 24):
        i, v = llv_idx[a:b], llv_val[a:b]
        if not bool((lcp[i] == 255).all()) or int(v.min()) < 255:
            return False, ".llv entry without a 255 in the lcp table, or value < 255"
        p, q = sa[i - 1], sa[i]
        ia, ib = p + v, q + v
        va = torch.where(ia < n, enc[torch.clamp(ia, max=n - 1)], torch.full_like(ia, 255, dtype=torch.uint8))
        vb = torch.where(ib < n, enc[torch.clamp(ib, max=n - 1)], torch.full_like(ib, 255, dtype=torch.uint8))
        if not bool(((va != vb) | (va >= 254)).all()):
            return False, "suffixes of an .llv entry agree beyond its value"
        r = (torch.rand((b - a, probes), device=sa.device, generator=g) * v[:, None].to(torch.float64)).to(torch.int64)
        r = torch.cat([r, (v - 1)[:, None]], dim=1)
        xa, xb = enc[p[:, None] + r], enc[q[:, None] + r]
        if not bool(((xa == xb) & (xa < 254)).all()):
            return False, "suffixes of an .llv entry differ before its value"
    return True, ""


def check_esastats_exact(sa, enc, lcp, llv_idx, llv_val, prefixlength, stats):
    """the .prj numbers that depend on the tables, by the oracle's definition
    (oracle/esa_oracle.c, ora_esastats_compute): `longest` is the table index of
    suffix 0, `largelcpvalues` the entries of LCP >= 255, `maxbranchdepth` the
    largest LCP, `lcptabsum` the sum of the LCPs of the entries whose suffix has
    at least `prefixlength` letters in front of the first special or the end.
    Only for tables the other checkers have accepted; stats: the engine's dict.
    Returns (ok, message)."""
    N = sa.numel()
    n = N - 1
    dev = sa.device
    # letters in front of the next special: the next special's position from a
    # reverse cumulative minimum, chunk by chunk from the end of the text
    enough = torch.empty(N, dtype=torch.bool, device=dev)
    enough[n] = prefixlength == 0
    carry = n
    for a, b in reversed(list(_chunks(n))):
        p = torch.arange(a, b, dtype=torch.int64, device=dev)
        nxt = torch.where(enc[a:b] >= 254, p, torch.full_like(p, carry))
        nxt = torch.flip(torch.cummin(torch.flip(nxt, [0]), 0).values, [0])
        enough[a:b] = nxt - p >= prefixlength
        carry = int(nxt[0].item())
    longest, large, depth, total = -1, 0, 0, 0
    for a, b in _chunks(N):
        p = sa[a:b]
        at = torch.nonzero(p == 0).flatten()
        if at.numel() > 0:
            longest = a + int(at[0].item())
        c = lcp[a:b].to(torch.int64)
        big = c == 255
        if bool(big.any()):
            r = torch.nonzero(big).flatten() + a
            c[big] = llv_val[torch.searchsorted(llv_idx, r)]
        large += int(big.sum().item())
        depth = max(depth, int(c.max().item()))
        total += int((c * enough[p]).sum().item())
    want = {"longest": longest, "largelcpvalues": large, "maxbranchdepth": depth,
            "lcptabsum": total}
    for name, v in want.items():
        if int(stats[name]) != v:
            return False, "%s is %d, the tables give %d" % (name, int(stats[name]), v)
    return True, ""


def count_lcp_overflows(lcp):
    total = 0
    for a, b in _chunks(lcp.numel()):
        total += int((lcp[a:b] == 255).sum().item())
    return total


def as_tensor(ptr, count, typestr, device="cuda:0"):
    class _W:
        pass
    w = _W()
    w.__cuda_array_interface__ = {"shape": (count,), "typestr": typestr, "data": (ptr, False), "version": 2}
    return torch.as_tensor(w, device=device)


def numpy_pairs_to_device(llv, device="cuda:0"):
    t = torch.from_numpy(np.ascontiguousarray(llv).view(np.int64).reshape(-1, 2)).to(device)
    return t[:, 0].contiguous(), t[:, 1].contiguous()
