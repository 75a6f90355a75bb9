"""The local alignments of include/gtamd_locali.h as plain numpy: the statement
per suffix, column by column with stored traces and a traceback, no tree, no
band and no start row that travels with a score.  All start positions advance
together, one numpy operation per row.  The yardstick of tests/test_locali_gpu.py
and of the core test; it reproduces the recorded calls of the reference
(tests/test_locali_host.py).  Keep subjects to some 20 k symbols."""
import numpy as np

WILDCARD, SEPARATOR = 254, 255
NONE, INSERT, REPLACE, DELETE = 0, 1, 2, 3


def max_depth(m, match, gapextend):
    """the deepest column that can hold a cell > 0: match * m + gapextend * (d - m) > 0"""
    return m + -(-(match * m) // -gapextend) - 1


def column(prev, c, query, match, mismatch, gapextend):
    """column d of every start position at once: prev (A, m + 1) is column d - 1 or
    None for d = 1, c (A,) the subject letters; (scores, traces)"""
    m = query.size
    A = c.size
    col = np.full((A, m + 1), -1, dtype=np.int64)
    tr = np.zeros((A, m + 1), dtype=np.uint8)
    for i in range(1, m + 1):
        r = np.where(query[i - 1] == c, match, mismatch)
        v = np.full(A, -1, dtype=np.int64)
        t = np.zeros(A, dtype=np.uint8)

        def take(cand, allowed, bit):
            better = allowed & (cand > v)
            v[better] = cand[better]
            t[better] = bit

        take(col[:, i - 1] + gapextend, col[:, i - 1] > 0, DELETE)
        if prev is None:
            take(r, np.ones(A, dtype=bool), REPLACE)
            take(np.full(A, gapextend), np.ones(A, dtype=bool), INSERT)
        else:
            take(prev[:, i - 1] + r, prev[:, i - 1] > 0, REPLACE)
            take(prev[:, i] + gapextend, prev[:, i] > 0, INSERT)
        col[:, i] = v
        tr[:, i] = t
    return col, tr


def matches_of_query(enc, query, match=1, mismatch=-1, gapextend=-1, T=1):
    """{p: (dblen, score, qstart, qlen)} for one query"""
    enc = np.asarray(enc, dtype=np.uint8)
    query = np.asarray(query, dtype=np.uint8)
    n, m = enc.size, query.size
    alive = np.arange(n, dtype=np.int64)
    prev = None
    history = []                       # per depth: (the start positions, ascending; their traces)
    found = {}
    for d in range(1, max_depth(m, match, gapextend) + 2):
        ok = alive + d - 1 < n
        ok[ok] &= enc[alive[ok] + d - 1] < WILDCARD
        alive = alive[ok]
        if alive.size == 0:
            break
        col, tr = column(None if prev is None else prev[ok], enc[alive + d - 1], query, match, mismatch, gapextend)
        history.append((alive, tr))
        pos = np.where(col > 0, col, 0)
        M = pos.max(axis=1)
        e = pos.argmax(axis=1)             # (the first of equal maxima: the smallest row)
        for k in np.flatnonzero(M >= T):
            p, i, dd = int(alive[k]), int(e[k]), d
            while dd > 0:
                ids, traces = history[dd - 1]
                bit = traces[np.searchsorted(ids, p), i]
                assert bit != NONE
                if bit == INSERT:
                    dd -= 1
                elif bit == REPLACE:
                    dd -= 1
                    i -= 1
                else:
                    i -= 1
            found[p] = (d, int(M[k]), i, int(e[k]) - i)
        go = (M < T) & (M > 0)
        alive, prev = alive[go], col[go]
        assert d <= max_depth(m, match, gapextend) or alive.size == 0
    return found


def records(enc, suf, queries, match=1, mismatch=-1, gapextend=-1, T=1):
    """the records of the C ABI, (matches, 4) uint64, in its order: ascending
    query, then ascending table index of dbstart"""
    enc = np.asarray(enc, dtype=np.uint8)
    suf = np.asarray(suf).astype(np.int64)
    rank = np.zeros(enc.size + 1, dtype=np.int64)
    rank[suf] = np.arange(suf.size)
    out = []
    for qn, query in enumerate(queries):
        found = matches_of_query(enc, query, match, mismatch, gapextend, T)
        for p in sorted(found, key=lambda x: rank[x]):
            dblen, score, qstart, qlen = found[p]
            out.append((qn, p, dblen | score << 32, qstart | qlen << 32))
    return np.array(out, dtype=np.uint64).reshape(-1, 4)


def alignment_lines(enc, p, dblen, query, e, match, mismatch, gapextend, letters, wildcardshow, width=70):
    """the alignment of a match as `-s` shows it: the columns again with stored
    traces, the traceback from (e, dblen), blocks of `width` columns with the
    query on top"""
    history, prev = [], None
    for d in range(1, dblen + 1):
        prev, tr = column(prev, enc[p + d - 1:p + d], query, match, mismatch, gapextend)
        history.append(tr[0])
    ops, d, i = [], dblen, e
    while d > 0:
        bit = history[d - 1][i]
        ops.append(bit)
        if bit != DELETE:
            d -= 1
        if bit != INSERT:
            i -= 1
    show = lambda c: letters[c] if c < WILDCARD else wildcardshow
    top, mid, low, iv = "", "", "", p
    for bit in reversed(ops):
        a = query[i] if bit != INSERT else None
        b = enc[iv] if bit != DELETE else None
        top += "-" if a is None else show(a)
        low += "-" if b is None else show(b)
        mid += "|" if bit == REPLACE and a == b and a < WILDCARD else " "
        i += bit != INSERT
        iv += bit != DELETE
    out = []
    for at in range(0, len(top), width):
        out += [top[at:at + width], mid[at:at + width], low[at:at + width]]
    return out


def tool_stdout(enc, suf, queries, T, match=1, mismatch=-3, gapextend=-2, show=False, letters="acgt",
                wildcardshow="n"):
    """the stdout of the tool behind its two path lines, the matches of a query
    in table order"""
    enc = np.asarray(enc, dtype=np.uint8)
    seqstart = np.concatenate([[0], np.flatnonzero(enc == SEPARATOR) + 1])
    rec = records(enc, suf, queries, match, mismatch, gapextend, T)
    out = ["# threshold=%d" % T]
    at = 0
    for qn, query in enumerate(queries):
        out.append("process sequence %d of length %d" % (qn, len(query)))
        while at < rec.shape[0] and rec[at, 0] == qn:
            p, ls, qs = (int(x) for x in rec[at, 1:])
            dblen, score, qstart, qlen = ls & 0xffffffff, ls >> 32, qs & 0xffffffff, qs >> 32
            seq = int(np.searchsorted(seqstart, p, side="right")) - 1
            out.append("%d\t%d\t%d\t\t%d\t%d\t%d\t%d" % (seq, p - seqstart[seq], dblen, qn, qstart, qlen, score))
            if show:
                out += alignment_lines(enc, p, dblen, np.asarray(query, dtype=np.uint8), qstart + qlen, match, mismatch,
                                       gapextend, letters, wildcardshow)
            at += 1
    return "".join(line + "\n" for line in out)
