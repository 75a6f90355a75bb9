"""Criteria 1, 2 and 5 of include/gtamd_check.h restated with numpy, for the
tests of the index checker: which entry of a damaged suffix table, and which
value of a damaged LCP table, is reported.  TEST INFRASTRUCTURE (the checker of
the checker)."""
import numpy as np

from genometools_amd import check


def first_suf_failure(enc, suf):
    """criteria 1 and 2 of include/gtamd_check.h with numpy: (criterion, index)"""
    n = enc.size
    N = n + 1
    suf = suf.astype(np.uint64)
    out = np.flatnonzero(suf > n)
    if out.size:
        return check.CRIT_RANGE, int(out[0])
    unset = (1 << 32) - 1
    rank = np.full(N, unset, dtype=np.int64)
    rank[suf.astype(np.int64)] = np.arange(N)
    p = np.arange(N)
    bad = (rank == unset) | (suf[np.where(rank == unset, 0, rank)].astype(np.int64) != p)
    if bad.any():
        return check.CRIT_PERM, int(np.flatnonzero(bad)[0])
    s = suf.astype(np.int64)
    sym = np.append(enc.astype(np.int64), 255)
    c = np.where(sym >= 254, 256 + p, sym)
    a, b = s[:-1], s[1:]
    ca, cb = c[a], c[b]
    ok = (ca < cb) | ((ca == cb) & (ca < 254) & (rank[np.minimum(a + 1, n)] < rank[np.minimum(b + 1, n)]))
    if not ok.all():
        return check.CRIT_ORDER, int(np.flatnonzero(~ok)[0]) + 1
    return check.CRIT_NONE, None


def claims(lcp, llv):
    """C[i] of criterion 5: the byte, or the value of the row's .llv pair where
    the byte is 255 (criterion 4 holds: every byte 255 has its pair)"""
    C = lcp.astype(np.int64)
    big = np.flatnonzero(lcp == 255)
    if big.size:
        llv = np.asarray(llv).reshape(-1, 2).astype(np.int64)
        C[big] = llv[np.searchsorted(llv[:, 0], big), 1]
    return C


def _common_letters(sym, a, b):
    """length of the common prefix of letters of suffixes a and b; sym: the
    symbols, specials behind the end"""
    k, w = 0, 64
    while True:
        xa, xb = sym[a + k:a + k + w], sym[b + k:b + k + w]
        m = min(xa.size, xb.size)
        stop = np.flatnonzero((xa[:m] != xb[:m]) | (xa[:m] >= 254))
        if stop.size:
            return k + int(stop[0])
        k += m


def first_lcp_failure(enc, suf, lcp, llv):
    """criterion 5 of include/gtamd_check.h with numpy, for tables that pass
    criteria 1 to 4 (suf: a correct table): None, or (table, criterion, index,
    llv_entry, claimed, found, pos_a, pos_b) of the smallest table index that
    fails (a) or (b).  It works from the CLAIMS as the header words it: s comes
    from the claim of position p - 1, (a) is tested at offset C, (b) over [s, C);
    an offset at or beyond n reads as a special."""
    n = enc.size
    N = n + 1
    sa = suf.astype(np.int64)
    rank = np.empty(N, dtype=np.int64)
    rank[sa] = np.arange(N)
    C = claims(lcp, llv)
    sym = np.concatenate([enc.astype(np.uint8), np.full(n + 2, 255, dtype=np.uint8)])   # p + C <= 2n
    p = np.arange(N)
    has = rank >= 1
    row = np.maximum(rank, 1)
    Cp = np.where(has, C[row], 0)
    q = sa[row - 1]
    s = np.zeros(N, dtype=np.int64)
    s[1:] = np.maximum(Cp[:-1] - 1, 0)               # (Cp is 0 where rank[p - 1] = 0)
    va, vb = sym[p + Cp], sym[q + Cp]
    bad = has & (va == vb) & (va < 254)              # (a)
    act = np.flatnonzero(has & ~bad & (Cp > s))      # (b), sweeps that widen
    cur, end, qa = s[act], Cp[act], q[act]
    w = 2
    while act.size:
        o = cur[:, None] + np.arange(w)[None, :]
        inside = o < end[:, None]
        o = np.minimum(o, end[:, None] - 1)
        xa, xb = sym[act[:, None] + o], sym[qa[:, None] + o]
        hit = (inside & ((xa != xb) | (xa >= 254))).any(axis=1)
        bad[act[hit]] = True
        cur = cur + w
        keep = ~hit & (cur < end)
        act, cur, end, qa = act[keep], cur[keep], end[keep], qa[keep]
        w = min(4 * w, 4096)
        while w > 2 and act.size * w > 1 << 24:
            w //= 2
    if not bad.any():
        return None
    r = int(rank[bad].min())
    a, b = int(sa[r - 1]), int(sa[r])
    claimed, found = int(C[r]), _common_letters(sym, a, b)
    in_llv = lcp[r] == 255
    entry = int(np.searchsorted(np.asarray(llv).reshape(-1, 2)[:, 0].astype(np.int64), r)) if in_llv else check.NONE
    return (check.LLV if in_llv else check.LCP,
            check.CRIT_LCP_SMALL if claimed < found else check.CRIT_LCP_LARGE,
            r, entry, claimed, found, a, b)
