"""Brute-force restatement of include/gtamd_mstat.h, independent of any binary
search: for a query position, the SET of subject positions whose suffix still
matches is extended by one letter until it is empty.

  ms = the last depth at which the set is not empty
  w  = the member of that last set with the smallest rank in the suffix table
  mu = the first depth at which the set has one member, 0 if there is none

The sets of the first depths are taken for all query positions at once: two
positions are in the same set exactly when their d letters, read as a number,
agree, so one sort of those numbers per depth gives every set, its size and its
member of smallest rank.  Positions that still match at depth DEPTHS go on one
by one.  Also the text `gt matstat` / `gt uniquesub` print
(src/match/greedyfwdmat.c:168-211).  Test infrastructure only."""
import functools

import numpy as np

import oracle_util as ou

DEPTHS = 12            # sigma ** DEPTHS < 2 ** 62 for up to 35 letters


def _padded(a, special, pad):
    """int64 symbols with every special replaced by `special`, and `pad` of them behind"""
    out = np.full(a.size + pad, special, dtype=np.int64)
    out[:a.size] = np.where(a >= 254, special, a.astype(np.int64))
    return out


def _shared(Q, i, E, p, d):
    """letters Q[i..) and E[p..) share, the first d of them known; the sequences
    end in specials that differ between the two, so no length is needed"""
    step = 64
    while True:
        a, b = Q[i + d:i + d + step], E[p + d:p + d + step]
        k = min(a.size, b.size)
        ne = np.flatnonzero(a[:k] != b[:k])
        if ne.size:
            return d + int(ne[0])
        if k < step:
            return d + k
        d += k
        step *= 2


def brute_force(enc, suf, query):
    """(ms, w, mu) for every query position: int64 arrays; w is 0 where ms is 0"""
    enc = np.ascontiguousarray(enc, dtype=np.uint8)
    query = np.ascontiguousarray(query, dtype=np.uint8)
    n, m = enc.size, query.size
    rank = np.empty(n + 1, dtype=np.int64)
    rank[np.asarray(suf, dtype=np.int64)] = np.arange(n + 1)
    E, Q = _padded(enc, -1, DEPTHS + 1), _padded(query, -2, DEPTHS + 1)
    letters = [int(a[a < 254].max()) + 1 if (a < 254).any() else 1 for a in (enc, query)]
    base = max(letters)
    assert base ** DEPTHS < 2 ** 62
    ms, w, mu = (np.zeros(m, dtype=np.int64) for _ in range(3))
    spos, scode = np.arange(n), np.zeros(n, dtype=np.int64)       # subject positions still all letters
    qpos, qcode = np.arange(m), np.zeros(m, dtype=np.int64)       # query positions that still match
    groups = None
    for d in range(1, DEPTHS + 1):
        keep = E[spos + d - 1] >= 0
        spos, scode = spos[keep], scode[keep] * base + E[spos[keep] + d - 1]
        keep = Q[qpos + d - 1] >= 0
        qpos, qcode = qpos[keep], qcode[keep] * base + Q[qpos[keep] + d - 1]
        order = np.lexsort((rank[spos], scode))                   # every set, smallest rank first
        by_set = spos[order]
        codes, first, count = np.unique(scode[order], return_index=True, return_counts=True)
        j = np.searchsorted(codes, qcode)
        hit = (j < codes.size)
        hit[hit] = codes[j[hit]] == qcode[hit]
        qpos, qcode, j = qpos[hit], qcode[hit], j[hit]
        ms[qpos] = d
        w[qpos] = by_set[first[j]]
        once = qpos[(count[j] == 1) & (mu[qpos] == 0)]
        mu[once] = d
        groups = (by_set, first[j], count[j])
        if qpos.size == 0:
            return ms, w, mu
    by_set, first, count = groups
    for i, f, c in zip(qpos.tolist(), first.tolist(), count.tolist()):
        alive, d = by_set[f:f + c], DEPTHS
        while alive.size > 8:                     # letter by letter
            nxt = alive[E[alive + d] == Q[i + d]]
            if nxt.size == 0:
                break
            alive, d = nxt, d + 1
        else:
            # few are left: how far each of them goes.  The set of depth l holds
            # those that go at least that far; the last set, those that go farthest.
            if alive.size == 1 and mu[i] == 0:
                mu[i] = d
            far = np.array([_shared(Q, i, E, int(p), d) for p in alive])
            d = int(far.max())
            if mu[i] == 0 and far.size > 1:
                second = int(np.sort(far)[-2])
                if second < d:
                    mu[i] = second + 1
            alive = alive[far == d]
        ms[i] = d
        w[i] = alive[np.argmin(rank[alive])]
    return ms, w, mu


@functools.lru_cache(maxsize=None)
def encoded(name, protein):
    enc = ou.encode_fasta(ou.fixture_path(name), protein)
    enc.setflags(write=False)
    return enc


@functools.lru_cache(maxsize=None)
def suffix_table(name, protein):
    suf = ou.esa(encoded(name, protein), 20 if protein else 4)["suf"]
    suf.setflags(write=False)
    return suf


@functools.lru_cache(maxsize=None)
def expected(subject, query, protein):
    """(ms, w, mu) of the brute force for two fixtures; shared, never written to"""
    res = brute_force(encoded(subject, protein), suffix_table(subject, protein), encoded(query, protein))
    for a in res:
        a.setflags(write=False)
    return res


def capped(values, max_len):
    """what a call with max_len reports for the exact values"""
    return np.minimum(values, max_len + 1)


def split_units(query):
    """the sequences of an encoded query: (start, length) between the separators"""
    cuts = np.flatnonzero(query == 255)
    starts = np.concatenate([[0], cuts + 1])
    ends = np.concatenate([cuts, [query.size]])
    return list(zip(starts.tolist(), (ends - starts).tolist()))


def read_descriptions(path):
    with open(path, "rb") as f:
        return [line[1:].rstrip(b"\r\n").decode("latin-1") for line in f if line.startswith(b">")]


def tool_output(query, descriptions, length, subjectpos, characters, show, minlen=None, maxlen=None,
                first_unit=0):
    """stdout of `gt matstat` / `gt uniquesub` for one encoded query (sequences
    joined by separators), its descriptions and the per-position results; show:
    subset of {"querypos", "subjectpos", "sequence"}"""
    out = []
    for u, (start, cnt) in enumerate(split_units(query)):
        desc = descriptions[u]
        out.append("unit %d%s\n" % (first_unit + u, " (%s)" % desc if desc else ""))
        for k in range(cnt):
            v = int(length[start + k])
            if v == 0 or (minlen is not None and v < minlen) or (maxlen is not None and v > maxlen):
                continue
            fields = []
            if "querypos" in show:
                fields.append("%d" % k)
            fields.append("%d" % v)
            if "subjectpos" in show:
                fields.append("%d" % int(subjectpos[start + k]))
            if "sequence" in show:
                fields.append("".join(characters[c] for c in query[start + k:start + k + v]))
            out.append(" ".join(fields) + "\n")
    return "".join(out)
