"""Exact checks of tables that are too large for the CPU oracle, with torch on the
device that holds them (or on the CPU: tests/test_device_check.py).  TEST
INFRASTRUCTURE (the checker, never the thing checked): a restatement of the
reference's own linear-time checkers

  gt_suftab_lightweightcheck   src/match/sfx-lwcheck.c:181-337
  gt_lcptab_lightweightcheck   src/match/sfx-linlcp.c:548

for tables in device memory; check_lcp_exact turns Kasai's inheritance argument
into a check of every .lcp and .llv entry, and check_packed_index_exact checks
every field of a packed index (INDEX.bdx) against the .bwt and .suf tables it was
made from.  Sortedness of a suffix array is a LOCAL property once it is a
permutation: with rank = its inverse,

    suffix SA[i-1] < suffix SA[i]   for all i
  <=>  for all i:  c(SA[i-1]) < c(SA[i])  or
                   c(SA[i-1]) = c(SA[i]) is a letter and rank[SA[i-1]+1] < rank[SA[i]+1]

(induction over the common prefix), where c(p) is the letter at p, or -- special
symbols being unique and larger than every letter, larger at larger positions
(src/core/encseq.h:640, src/match/sfx-bentsedg.c:75-80) -- 256 + p.
"""
import struct
from math import comb, factorial

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


# ---- the packed index (INDEX.bdx) -------------------------------------------------
# Layout of the file, as oracle/pck_oracle.c restates it with its citations
# (src/match/eis-blockcomp.c, eis-bwtseq-extinfo.c, eis-seqblocktranslate.c,
# eis-seqranges.c): header | [locate header] | zeros up to a multiple of 8192 |
# one constant-width record per bucket of bsize x blbuck BWT positions | the
# variable-width parts of all buckets, one bit string | the region list.

PCK_CHUNK = 1 << 24          # table entries per step of check_packed_index_exact
PCK_LOCATE_BITMAP, PCK_LOCATE_COUNT = 1, 2     # enum BWTFeatures, eis-bwtseq-param.h:78-94


def _reqbits(v):
    """gt_requiredUInt64Bits, src/core/bitpackstringop.c:60-79: 1 for 0"""
    return max(1, int(v).bit_length())


def read_bits(raw, pos, n):
    """n bits at bit position pos of a byte string, most significant first"""
    v = 0
    for b in range(pos, pos + n):
        v = (v << 1) | ((raw[b >> 3] >> (7 - (b & 7))) & 1)
    return v


def unrank_block(comp, perm, sigma, B):
    """the block with composition index `comp` and permutation index `perm`
    (inverse of gt_block2IndexPair, src/match/eis-seqblocktranslate.c:436-540),
    and the function that counts the arrangements of a composition"""
    cnt, left = [], B
    for i in range(sigma - 1):
        k = sigma - i - 1
        v = 0
        while True:
            ways = comb(left - v + k - 1, k - 1)
            if comp < ways:
                break
            comp -= ways
            v += 1
        cnt.append(v)
        left -= v
    cnt.append(left)

    def arrangements(c):
        r = factorial(sum(c))
        for x in c:
            r //= factorial(x)
        return r
    out = []
    for _ in range(B):
        for s in range(sigma):
            if cnt[s] == 0:
                continue
            cnt[s] -= 1
            ways = arrangements(cnt)
            if perm < ways:
                out.append(s)
                break
            perm -= ways
            cnt[s] += 1
    return out, arrangements


def block_ranks(blocks, sigma):
    """(composition index, permutation index, bits of the permutation index) of
    every row of `blocks`, an int64 tensor [M, B] of letters: gt_block2IndexPair,
    src/match/eis-seqblocktranslate.c:436-540, as oracle/pck_oracle.c comp_index /
    perm_index restate it.  The compositions are listed in ascending order of
    (count of letter 0, count of letter 1, ...), from (0, ..., 0, B); the
    arrangements of a composition in ascending order of the string; the index of
    a composition with a single arrangement takes 0 bits, any other
    bits(arrangements - 1)."""
    M, B = blocks.shape
    dev = blocks.device
    i64 = torch.int64
    fact = torch.tensor([factorial(i) for i in range(B + 1)], dtype=i64, device=dev)
    binom = torch.tensor([[comb(n, k) for k in range(sigma + 1)] for n in range(B + sigma + 1)],
                         dtype=i64, device=dev)
    cnt = torch.zeros(M, sigma, dtype=i64, device=dev)
    cnt.scatter_add_(1, blocks, torch.ones_like(blocks))
    # composition: those with fewer of letter i (and the same counts before it)
    # come first, sum_{v < c_i} C(left - v + k - 1, k - 1) with k = sigma - 1 - i
    # letters after i, which is C(left + k, k) - C(left - c_i + k, k)
    comp = torch.zeros(M, dtype=i64, device=dev)
    left = torch.full((M,), B, dtype=i64, device=dev)
    for i in range(sigma - 1):
        k = sigma - 1 - i
        c = cnt[:, i]
        comp += binom[left + k, k] - binom[left - c + k, k]
        left = left - c
    # permutation: at each position p, the arrangements of what is left that start
    # with a smaller letter s come first, multinomial(rest - e_s) of them =
    # (left - 1)! rest_s / D with D = prod(rest_t!) -- summed over s < letter:
    # (left - 1)! below / D, exact (each term is), below <= left
    D = fact[cnt].prod(1)
    arrangements = fact[B] // D
    pow2 = torch.tensor([1 << t for t in range(63)], dtype=i64, device=dev)
    pbits = torch.searchsorted(pow2, arrangements - 1, right=True)
    perm = torch.zeros(M, dtype=i64, device=dev)
    rest = cnt.clone()
    letters = torch.arange(sigma, dtype=i64, device=dev)
    for p in range(B):
        x = blocks[:, p:p + 1]
        below = (rest * (letters[None, :] < x)).sum(1)
        perm += fact[B - p - 1] * below // D
        D = D // rest.gather(1, x).squeeze(1)
        rest.scatter_add_(1, x, torch.full_like(x, -1))
    return comp, perm, pbits


def _take32(img, pos, w):
    """fields of w <= 32 bits (w: a number or a tensor like pos) at bit positions
    pos of the uint8 tensor img, most significant bit first; bytes beyond the
    image read as 0"""
    n = img.numel()
    byte = pos >> 3
    x = torch.zeros_like(pos)
    for k in range(5):              # 7 + 32 bits fit 5 bytes
        i = byte + k
        b = torch.where(i < n, img[torch.clamp(i, max=n - 1)].to(torch.int64), torch.zeros_like(i))
        x = (x << 8) | b
    w = torch.as_tensor(w, dtype=torch.int64, device=pos.device)
    return (x >> (40 - (pos & 7) - w)) & ((torch.ones_like(w) << w) - 1)


def take_bits(img, pos, w):
    """fields of w <= 63 bits at bit positions pos (int64 tensor) of the uint8
    image, most significant bit first (gt_bsGetUInt64, src/core/bitpackstringop.c)"""
    if isinstance(w, int) and w <= 32:
        return _take32(img, pos, w)
    w = torch.as_tensor(w, dtype=torch.int64, device=pos.device)
    hi_w = torch.clamp(w - 32, min=0)
    lo_w = w - hi_w
    return (_take32(img, pos, hi_w) << lo_w) | _take32(img, pos + hi_w, lo_w)


def pck_toggles(bsize=8, blbuck=8, locfreq=16, locbitmap=None):
    """the feature toggles `gt packedindex` derives from its options:
    gt_computePackedIndexDefaults / estimateBestLocateTypeFeature,
    src/match/eis-bwtseq-param.c:69-103 (locbitmap None: option not given)"""
    if locbitmap is not None:
        return PCK_LOCATE_BITMAP if locbitmap else PCK_LOCATE_COUNT
    if not locfreq:
        return 0
    seg = bsize * blbuck
    return PCK_LOCATE_COUNT if seg > (seg + 1) * _reqbits(seg) // locfreq else PCK_LOCATE_BITMAP


def pck_layout(N, sigma, letters, bsize=8, blbuck=8, locfreq=16, locbitmap=None, mkindex=False):
    """widths and positions of INDEX.bdx for N table entries over sigma letters,
    letters[s] = occurrences of letter s in the BWT (the sequence statistics of
    mkindex); oracle/pck_oracle.c ora_pck_bdx, which cites each formula"""
    B, K, locint = bsize, blbuck, locfreq
    L = B * K
    toggles = pck_toggles(B, K, locint, locbitmap)
    bitmap = bool(locint) and bool(toggles & PCK_LOCATE_BITMAP)
    count = bool(locint) and bool(toggles & PCK_LOCATE_COUNT)
    nb = (N + 1) // L + (1 if (N + 1) % L else 0)
    bits_per_ulong = _reqbits(N - 1)
    sym_bits = [_reqbits(letters[s]) if mkindex else bits_per_ulong for s in range(sigma)]
    sym_off = [sum(sym_bits[:s]) for s in range(sigma)]
    comp_idx_bits = _reqbits(comb(B + sigma - 1, sigma - 1) - 1)
    even = [B // sigma + (1 if s < B % sigma else 0) for s in range(sigma)]
    max_perms = factorial(B)
    for c in even:
        max_perms //= factorial(c)
    max_perm_idx_bits = _reqbits(max_perms - 1)
    cw_ext_bits = L if bitmap else 0
    cb_off_bits = _reqbits(max_perm_idx_bits * K) if locint else 0
    bits_orig_pos = _reqbits(N - 1) if locint else 0
    max_var_bits = nb * max_perm_idx_bits * K
    max_var_ext = 0
    if locint:
        extra = 0
        if locint > 1:
            extra = min(N // 2, N - N // locint)
            if mkindex:
                nonval = N - sum(letters[:sigma]) + 1
                extra = min(extra, nonval, N - nonval)
        seg = [(L, (N + 1) // L), (N % L, 1 if (N + 1) % L else 0)]
        max_seg = max(s for s, _ in seg)
        tot = sum(_reqbits(s) * r for s, r in seg) if count else 0
        tot += (N // locint + extra) * ((_reqbits(max_seg) if count else 0) + bits_orig_pos)
        max_var_ext = max_seg * ((_reqbits(N - 1) if count else 0) + bits_orig_pos) + \
            (_reqbits(max_seg) if count else 0)
        max_var_bits += tot
    var_off_bits = _reqbits(max_var_bits)
    sym_sum_bits = sum(sym_bits)
    pre_cb_off = sym_sum_bits + var_off_bits
    pre_comp_idx = pre_cb_off + cb_off_bits
    pre_cw_ext = pre_comp_idx + comp_idx_bits * K
    cw_bits = pre_cw_ext + cw_ext_bits
    header_len = 4 + 4 + 8 + 8 + 12 + 12 + 8 + 8 + 8 + 4 * sigma + 8 + 8 + 8 + 12 + 4 * 2 + \
        (8 + 12 + 12 if cb_off_bits else 0)
    cw_data_pos = -(-(header_len + (8 + 16 if locint else 0)) // 8192) * 8192
    return dict(B=B, K=K, L=L, locint=locint, toggles=toggles, bitmap=bitmap, count=count, nb=nb,
                bits_per_ulong=bits_per_ulong, sym_bits=sym_bits, sym_off=sym_off,
                comp_idx_bits=comp_idx_bits, cw_ext_bits=cw_ext_bits, cb_off_bits=cb_off_bits,
                bits_orig_pos=bits_orig_pos, var_off_bits=var_off_bits, max_var_ext=max_var_ext,
                pre_var_idx=sym_sum_bits, pre_cb_off=pre_cb_off, pre_comp_idx=pre_comp_idx,
                pre_cw_ext=pre_cw_ext, cw_bits=cw_bits, header_len=header_len,
                cw_data_pos=cw_data_pos, var_data_pos=cw_data_pos + (cw_bits * nb + 7) // 8)


def _first(bad):
    return int(torch.nonzero(bad)[0].item())


def check_packed_index_exact(img, bwt, suf, sigma, bsize=8, blbuck=8, locfreq=16, locbitmap=None,
                             mkindex=False, sprank=False, longest=None, chunk=PCK_CHUNK,
                             report=None):
    """EVERY field of an INDEX.bdx image (uint8 tensor img, the whole file) against
    the tables it was made from: bwt (uint8 tensor, N entries), suf (int64 tensor,
    N entries; None without locate information), with the options of `gt
    packedindex` (-bsize, -blbuck, -locfreq, -locbitmap; mkindex: the file of
    `gt packedindex mkindex`, with sequence statistics).  Linear in N, chunked over
    buckets, on the tables' device; int64 throughout.  Returns (ok, message); the
    message names the first bad bucket and field.  report: a dict that receives
    the buckets checked, the largest occurrence counter and the largest var offset.

    Expected values come from the tables, the fields from the image by a big-endian
    bit gather (layout: oracle/pck_oracle.c):
      header   every field determined by N, sigma, the options and (mkindex) the
               letter counts; the zeros up to the first record
      bucket   the occurrence counter of each letter (exclusive prefix count in the
               BWT), the var offset (exclusive prefix sum of the var bits of the
               buckets before), [the bits of its permutation indices], the
               composition index of each block (specials stored as letter 0, the
               last block filled with letter 0), each permutation index at its
               place in the var part (block_ranks)
      locate   a row is marked when suf % locfreq == 0 or where letters and
               specials meet (the BWT symbol is a special xor the row lies in the
               tail of the table, the rows of the suffixes that start with a
               special: as many as the BWT holds specials); counts: the number of
               marks, then (row in bucket, text position) per mark; bitmap: one bit
               per row in the record, the text positions in the var part
      regions  the runs of specials in the BWT, then the closing record
    Not constrained: the bits between fields that the reference's staging
    buffers leave stale (the comp indices and bitmap bits behind the end of the
    last bucket among them; oracle/pck_oracle.c:8-9) -- the byte-for-byte
    comparisons with the oracle at small sizes pin those.  -sprank (reversibly
    sorted specials) is refused: the oracle comparisons cover it."""
    if sprank:
        raise ValueError("check_packed_index_exact: -sprank (reversibly sorted specials) is not "
                         "covered; compare with oracle/pck_oracle.c instead")
    if not 2 <= sigma <= 28:
        raise ValueError("check_packed_index_exact: %d letters, 2 to 28 are covered" % sigma)
    dev = bwt.device
    i64 = torch.int64
    N = bwt.numel()
    # ---- letter counts and specials of the BWT, the row of suffix 0
    hist = torch.zeros(256, dtype=i64, device=dev)
    for a, b in _chunks(N):
        hist += torch.bincount(bwt[a:b].to(i64), minlength=256)
    hist = hist.cpu().tolist()
    if sum(hist[sigma:254]):
        return False, "the BWT holds symbols outside the %d letters" % sigma
    letters, nspecial = hist[:sigma], hist[254] + hist[255]
    ly = pck_layout(N, sigma, letters, bsize, blbuck, locfreq, locbitmap, mkindex)
    B, K, L, nb, locint = ly["B"], ly["K"], ly["L"], ly["nb"], ly["locint"]
    if locint and longest is None:
        for a, b in _chunks(N):
            at = torch.nonzero(suf[a:b] == 0).flatten()
            if at.numel():
                longest = a + int(at[0].item())
                break
    cw_base, var_base = 8 * ly["cw_data_pos"], 8 * ly["var_data_pos"]
    cw_bits, bop = ly["cw_bits"], ly["bits_orig_pos"]
    first_special_row = N - nspecial
    rb = torch.tensor([_reqbits(v) for v in range(L + 1)], dtype=i64, device=dev)
    carry = torch.zeros(sigma, dtype=i64, device=dev)
    var_carry, max_counter, max_var_off = 0, 0, 0
    step = max(1, chunk // L)
    for j0 in range(0, nb, step):
        j1 = min(nb, j0 + step)
        nbk, p0 = j1 - j0, j0 * L
        real = max(0, min(j1 * L, N) - p0)
        js = torch.arange(j0, j1, dtype=i64, device=dev)
        rec = cw_base + js * cw_bits                          # bit of each record
        lens = torch.clamp(N - js * L, min=0, max=L)
        sym = torch.zeros(nbk * L, dtype=i64, device=dev)     # the fill: letter 0
        sym[:real] = bwt[p0:p0 + real].to(i64)
        off = torch.arange(nbk * L, dtype=i64, device=dev)
        bl = off // L                                         # bucket in the chunk
        special = sym >= 254
        letter = torch.where(special, torch.zeros_like(sym), sym)

        def bad_bucket(bad, what, got, want):
            i = _first(bad)
            return False, "bucket %d: %s is %d, the tables give %d" % (
                j0 + i, what, int(got[i]), int(want[i]))

        # occurrence counters: letters before the bucket
        live = (off < real) & ~special
        cnt = torch.bincount(bl[live] * sigma + sym[live], minlength=nbk * sigma).view(nbk, sigma)
        before = carry[None, :] + torch.cumsum(cnt, 0) - cnt
        carry += cnt.sum(0)
        for s in range(sigma):
            got = take_bits(img, rec + ly["sym_off"][s], ly["sym_bits"][s])
            bad = got != before[:, s]
            if bool(bad.any()):
                return bad_bucket(bad, "occurrence counter of letter %d" % s, got, before[:, s])
        max_counter = max(max_counter, int(before.max().item()))
        # blocks: composition and permutation indices (blocks behind the end of
        # the last bucket do not exist)
        comp, perm, pbits = block_ranks(letter.view(nbk * K, B), sigma)
        blk_live = torch.arange(nbk * K, dtype=i64, device=dev) * B < real
        pbits = torch.where(blk_live, pbits, torch.zeros_like(pbits))
        pb = pbits.view(nbk, K)
        pb_before = torch.cumsum(pb, 1) - pb
        pb_sum = pb.sum(1)
        # locate marks
        varbits = pb_sum.clone()
        if locint:
            rows = p0 + off
            v = torch.zeros_like(sym)
            v[:real] = suf[p0:p0 + real]
            mark = (off < real) & ((v % locint == 0) | (special != (rows >= first_special_row)))
            nm = mark.view(nbk, L).sum(1)
            rowbits = rb[torch.clamp(lens - 1, min=0)]
            if ly["count"]:
                varbits += rb[lens] + nm * (rowbits + bop)
            else:
                varbits += nm * bop
        var_off = var_carry + torch.cumsum(varbits, 0) - varbits
        var_carry += int(varbits.sum().item())
        max_var_off = max(max_var_off, int(var_off.max().item()))
        got = take_bits(img, rec + ly["pre_var_idx"], ly["var_off_bits"])
        bad = got != var_off
        if bool(bad.any()):
            return bad_bucket(bad, "var offset", got, var_off)
        if locint:
            got = take_bits(img, rec + ly["pre_cb_off"], ly["cb_off_bits"])
            bad = got != pb_sum
            if bool(bad.any()):
                return bad_bucket(bad, "bits of the permutation indices", got, pb_sum)
        bk = torch.nonzero(blk_live).flatten()
        b_of, b_in = bk // K, bk % K
        got = take_bits(img, rec[b_of] + ly["pre_comp_idx"] + b_in * ly["comp_idx_bits"],
                        ly["comp_idx_bits"])
        bad = got != comp[bk]
        if bool(bad.any()):
            i = _first(bad)
            return False, "bucket %d: composition index of block %d is %d, the tables give %d" % (
                j0 + int(b_of[i]), int(b_in[i]), int(got[i]), int(comp[bk[i]]))
        got = take_bits(img, var_base + var_off[b_of] + pb_before.flatten()[bk], pbits[bk])
        bad = got != perm[bk]
        if bool(bad.any()):
            i = _first(bad)
            return False, "bucket %d: permutation index of block %d is %d, the tables give %d" % (
                j0 + int(b_of[i]), int(b_in[i]), int(got[i]), int(perm[bk[i]]))
        if not locint:
            continue
        at = var_base + var_off + pb_sum                      # locate part of the var part
        if ly["count"]:
            got = take_bits(img, at, rb[lens])
            bad = got != nm
            if bool(bad.any()):
                return bad_bucket(bad, "mark count", got, nm)
            at = at + rb[lens]
        mi = torch.nonzero(mark).flatten()
        mb = bl[mi]
        k = torch.cumsum(mark.to(i64), 0)[mi] - 1 - (torch.cumsum(nm, 0) - nm)[mb]
        width = bop + (rowbits[mb] if ly["count"] else 0)
        pos = at[mb] + k * width
        if ly["count"]:
            got = take_bits(img, pos, rowbits[mb])
            want = mi - mb * L
            bad = got != want
            if bool(bad.any()):
                i = _first(bad)
                return False, "bucket %d: row of mark %d is %d, the tables give %d" % (
                    j0 + int(mb[i]), int(k[i]), int(got[i]), int(want[i]))
            pos = pos + rowbits[mb]
        got = take_bits(img, pos, bop)
        bad = got != v[mi]
        if bool(bad.any()):
            i = _first(bad)
            return False, "bucket %d: text position of mark %d is %d, the tables give %d" % (
                j0 + int(mb[i]), int(k[i]), int(got[i]), int(v[mi[i]]))
        if ly["bitmap"]:
            r = torch.arange(real, dtype=i64, device=dev)
            got = take_bits(img, rec[bl[:real]] + ly["pre_cw_ext"] + r % L, 1)
            bad = got != mark[:real].to(i64)
            if bool(bad.any()):
                i = _first(bad)
                return False, "bucket %d: locate bit of row %d is %d, the tables give %d" % (
                    j0 + i // L, i % L, int(got[i]), int(mark[i]))
    if report is not None:
        report.update(buckets=nb, max_counter=max_counter, max_var_offset=max_var_off,
                      var_bits=var_carry)
    # ---- the region list: runs of specials in the BWT (symbol 0 wildcard, 1
    # separator), the closing record just beyond the sequence
    starts, ends = [], []
    for a, b in _chunks(N):
        w = torch.zeros(b - a + 2, dtype=torch.uint8, device=dev)
        w[1:-1] = bwt[a:b]
        if a > 0:
            w[0] = bwt[a - 1]
        if b < N:
            w[-1] = bwt[b]
        s = w[1:-1]
        sp = s >= 254
        starts.append(torch.nonzero(sp & (w[:-2] != s)).flatten() + a)
        ends.append(torch.nonzero(sp & (w[2:] != s)).flatten() + a + 1)
    starts, ends = torch.cat(starts), torch.cat(ends)
    nr = starts.numel() + 1
    range_enc_pos = ly["var_data_pos"] + (var_carry + 7) // 8
    if report is not None:
        report.update(regions=nr)
    # ---- header (writeIdxHeader, eis-blockcomp.c:1984-2094; the locate header,
    # eis-bwtseq-extinfo.c:39-76), then the zeros up to the first record
    fields = [("magic", "4s", b"BDX\0"), ("header size", "<I", -(-ly["header_len"] // 8192) * 8192),
              ("tag BKSZ", "<I", 0x424b535a), ("block size", "<I", B),
              ("tag BBLK", "<I", 0x42424c4b), ("blocks per bucket", "<I", K),
              ("tag VOFF", "<I", 0x564f4646), ("var data position", "<Q", ly["var_data_pos"]),
              ("tag ROFF", "<I", 0x524f4646), ("region list position", "<Q", range_enc_pos),
              ("tag SELE", "<I", 0x53454c45), ("sequence length", "<Q", N),
              ("tag SPBT", "<I", 0x53504254), ("bits per position", "<I", ly["bits_per_ulong"]),
              ("tag VDOB", "<I", 0x56444f42), ("var offset bits", "<I", ly["var_off_bits"]),
              ("tag SSBT", "<I", 0x53534254), ("alphabet size", "<I", sigma)]
    fields += [("counter bits of letter %d" % s, "<I", ly["sym_bits"][s]) for s in range(sigma)]
    fields += [("tag BEFB", "<I", 0x42454642), ("BEFB", "<I", 0),
               ("tag REFB", "<I", 0x52454642), ("REFB", "<I", 0),
               ("tag NMRN", "<I", 0x4e4d524e), ("range modes", "<I", 2),
               ("mode of letters", "<I", 1), ("mode of specials", "<I", 2)]
    if ly["cb_off_bits"]:
        fields += [("tag CBMB", "<I", 0x43424d42), ("permutation bits width", "<I", ly["cb_off_bits"]),
                   ("tag CEXB", "<I", 0x43455842), ("record extension bits", "<Q", ly["cw_ext_bits"]),
                   ("tag MEXB", "<I", 0x4d455842), ("var extension bound", "<Q", ly["max_var_ext"])]
    if locint:
        fields += [("tag of the locate header", "<I", 0x45480000 | 1111), ("locate header size", "<I", 16),
                   ("row of suffix 0", "<Q", longest), ("locate interval", "<I", locint),
                   ("feature toggles", "<I", ly["toggles"])]
    head = img[:ly["cw_data_pos"]].cpu().numpy().tobytes()
    if len(head) < ly["cw_data_pos"]:
        return False, "image of %d bytes ends in the header" % img.numel()
    o = 0
    for name, fmt, want in fields:
        got = struct.unpack_from(fmt, head, o)[0]
        if got != want:
            return False, "header: %s at byte %d is %r, the tables give %r" % (name, o, got, want)
        o += struct.calcsize(fmt)
    nz = np.flatnonzero(np.frombuffer(head, dtype=np.uint8)[o:])
    if nz.size:
        return False, "header: byte %d before the first record is not zero" % (o + int(nz[0]))
    # ---- size, then the region list
    size = range_enc_pos + 8 + 16 * nr
    if img.numel() != size:
        return False, "image is %d bytes, the tables give %d" % (img.numel(), size)
    # (the count and the starts are little-endian 64-bit numbers)
    got = int.from_bytes(img[range_enc_pos:range_enc_pos + 8].cpu().numpy().tobytes(), "little")
    if got != nr:
        return False, "region list: %d records, the tables give %d" % (got, nr)
    rs = torch.cat([starts, torch.tensor([N + B], dtype=i64, device=dev)])
    rl = torch.cat([ends - starts, torch.ones(1, dtype=i64, device=dev)])
    rsym = torch.cat([(bwt[torch.clamp(starts, max=N - 1)] == 255).to(i64),
                      torch.zeros(1, dtype=i64, device=dev)])
    for a, b in _chunks(nr):
        t = torch.arange(a, b, dtype=i64, device=dev)
        base = range_enc_pos + 8 + 16 * t
        start = torch.zeros_like(t)
        for k in range(8):
            start |= img[base + k].to(i64) << (8 * k)
        gs = take_bits(img, 8 * (base + 8), 1)
        gl = take_bits(img, 8 * (base + 8) + 1, 63)
        bad = (start != rs[a:b]) | (gs != rsym[a:b]) | (gl != rl[a:b])
        if bool(bad.any()):
            i = _first(bad)
            return False, "region record %d is (%d, %d, %d), the tables give (%d, %d, %d)" % (
                a + i, int(start[i]), int(gs[i]), int(gl[i]), int(rs[a + i]), int(rsym[a + i]),
                int(rl[a + i]))
    return True, ""
