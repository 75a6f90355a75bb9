"""Criteria 1 and 2 of include/gtamd_check.h restated with numpy, for the tests
of the index checker: which entry of a damaged suffix table is reported.  TEST
INFRASTRUCTURE (the checker of the checker)."""
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
