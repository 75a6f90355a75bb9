"""Brute-force restatement of include/gtamd_qmatch.h, independent of any suffix
table search: on every diagonal p - i of subject and query, the maximal runs of
equal letters of at least L symbols are the matches.  The suffix table is used
for the ORDER alone (ascending query position, then table index of the subject
suffix).  Also the query transformations of the reverse and reverse-complement
modes, the `ordered` filter of a search of the index against itself and the
lines `gt repfind` prints (gt_querymatch_position_convert, gt_querymatch_ordered:
src/match/querymatch.c).  Test infrastructure only."""
import functools

import numpy as np

import oracle_util as ou

MODES = {"fwd": "F", "rev": "R", "rcl": "P"}


def brute_force(enc, query, min_len):
    """the matches as an int32 array of rows (dbpos, qpos, len), diagonal by diagonal"""
    enc = np.ascontiguousarray(enc, dtype=np.uint8)
    query = np.ascontiguousarray(query, dtype=np.uint8)
    n, m = enc.size, query.size
    out = []
    for d in range(-(m - 1), n):              # subject p, query i = p - d
        p0, p1 = max(0, d), min(n, m + d)
        a, b = enc[p0:p1], query[p0 - d:p1 - d]
        eq = (a == b) & (a < 254)
        edges = np.flatnonzero(np.diff(np.concatenate([[0], eq.view(np.int8), [0]])))
        start, length = edges[::2], edges[1::2] - edges[::2]
        keep = length >= min_len
        if keep.any():
            start, length = start[keep], length[keep]
            out.append(np.stack([p0 + start, p0 - d + start, length], axis=1).astype(np.int32))
    return np.concatenate(out) if out else np.zeros((0, 3), dtype=np.int32)


def in_order(records, suf):
    """the records in the reference's order: ascending qpos, then table index of dbpos"""
    suf = np.asarray(suf).astype(np.int64)
    rank = np.empty(suf.size, dtype=np.int64)
    rank[suf] = np.arange(suf.size)
    return records[np.lexsort((rank[records[:, 0]], records[:, 1]))]


def units(seq):
    """the sequences of an encoded sequence set: (start, length) between the separators"""
    cuts = np.flatnonzero(np.asarray(seq) == 255)
    starts = np.concatenate([[0], cuts + 1])
    ends = np.concatenate([cuts, [np.asarray(seq).size]])
    return list(zip(starts.tolist(), (ends - starts).tolist()))


def transformed(query, mode):
    """gt_mmsearch_accessquery: every sequence reversed on its own ("rev"), its
    letters c turned into 3 - c in addition ("rcl")"""
    query = np.ascontiguousarray(query, dtype=np.uint8)
    if mode == "fwd":
        return query
    out = query.copy()
    for start, length in units(query):
        unit = query[start:start + length][::-1]
        out[start:start + length] = np.where(unit < 254, 3 - unit, unit) if mode == "rcl" else unit
    return out


def expected(enc, suf, query, min_len, mode="fwd"):
    """rows (dbpos, qpos, len) in order, in the coordinates of the transformed query"""
    return in_order(brute_force(enc, transformed(query, mode), min_len), suf).astype(np.int64)


def _unit_of(starts, pos):
    return np.searchsorted(starts, pos, side="right") - 1


def tool_lines(enc, suf, query, min_len, modes, first_unit=0, self_match=False, records=None):
    """the lines of `gt repfind -l min_len [-f] [-r] [-p] -q ...` (query: the
    encoded query files joined by separators) or, with self_match, of `-r` / `-p`
    without -q, where the query is the index itself and only `ordered` records
    are kept; modes: a subset of MODES, run in the order f, r, p.  records: mode
    -> what `expected` gives for it, if the caller has that already"""
    enc = np.ascontiguousarray(enc, dtype=np.uint8)
    query = enc if self_match else np.ascontiguousarray(query, dtype=np.uint8)
    dbstart = np.array([s for s, _ in units(enc)], dtype=np.int64)
    qunits = units(query)
    qstart = np.array([s for s, _ in qunits], dtype=np.int64)
    qlen = np.array([l for _, l in qunits], dtype=np.int64)
    lines = []
    for mode in ("fwd", "rev", "rcl"):
        if mode not in modes:
            continue
        rec = records[mode] if records is not None else expected(enc, suf, query, min_len, mode)
        rec = rec[rec[:, 2] >= min_len]
        dbseq = _unit_of(dbstart, rec[:, 0])
        dbrel = rec[:, 0] - dbstart[dbseq]
        unit = _unit_of(qstart, rec[:, 1])
        offset = rec[:, 1] - qstart[unit]
        qfwd = offset if mode == "fwd" else qlen[unit] - offset - rec[:, 2]
        keep = np.ones(rec.shape[0], dtype=bool)
        if self_match:
            keep = (dbseq < unit) | ((dbseq == unit) & (dbrel < qfwd + (0 if mode == "fwd" else 1)))
        for k in np.flatnonzero(keep).tolist():
            lines.append("%d %d %d %s %d %d %d" % (rec[k, 2], dbseq[k], dbrel[k], MODES[mode], rec[k, 2],
                                                  first_unit + unit[k], qfwd[k]))
    return lines


def normalised(raw):
    """the lines of a tool's stdout that are compared: those starting with `#`
    dropped, runs of white space made one blank; the order is kept"""
    return [" ".join(l.split()) for l in raw.decode("latin-1").splitlines() if l.strip() and not l.startswith("#")]


@functools.lru_cache(maxsize=None)
def encoded(name, protein=False):
    enc = ou.encode_fasta(ou.fixture_path(name), protein)
    enc.setflags(write=False)
    return enc


@functools.lru_cache(maxsize=None)
def suffix_table(name, protein=False):
    suf = ou.esa(encoded(name, protein), 20 if protein else 4)["suf"]
    suf.setflags(write=False)
    return suf


def joined(names, protein=False):
    """several query files as one encoded query: a separator between two files"""
    parts = []
    for k, name in enumerate(names):
        if k:
            parts.append(np.array([255], dtype=np.uint8))
        parts.append(encoded(name, protein))
    return np.concatenate(parts)


BASE_LEN = 4           # the shortest minimum length of a golden call


@functools.lru_cache(maxsize=None)
def fixture_records(subject, queries, mode, protein=False):
    """`expected` at BASE_LEN for fixtures, once: the records of a larger minimum
    length are those of them that are long enough, in the same order.  queries:
    a tuple of names, () for the index against itself"""
    enc = encoded(subject, protein)
    rec = expected(enc, suffix_table(subject, protein), joined(queries, protein) if queries else enc, BASE_LEN, mode)
    rec.setflags(write=False)
    return rec


def call_lines(subject, queries, min_len, modes, protein=False):
    """tool_lines for fixtures, min_len >= BASE_LEN"""
    assert min_len >= BASE_LEN
    return tool_lines(encoded(subject, protein), suffix_table(subject, protein),
                      joined(queries, protein) if queries else None, min_len, modes, self_match=not queries,
                      records={m: fixture_records(subject, queries, m, protein) for m in modes})
