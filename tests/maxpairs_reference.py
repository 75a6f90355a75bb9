"""Brute-force restatement of include/gtamd_maxpairs.h, independent of any
suffix or LCP table: for every offset d, the maximal runs of positions p with
T[p] == T[p + d], both letters.  A run of `len` positions from p is, by its
maximality on both sides, exactly one maximal pair (len, p, p + d): the run
cannot go on to the left (p = 0, or the symbols in front differ or one is a
special) nor to the right.  Also the lines `gt repfind` prints for exact matches
and the segments the walk of csrc/esa_maxpairs_walk.h works on.  Test
infrastructure only."""
import ctypes
import functools
import os
import subprocess

import numpy as np

import oracle_util as ou

UNIQUE = 255           # left-character class of position 0 and behind a special


def brute_force(enc, min_len):
    """every maximal pair of at least min_len letters: int64 array of rows
    (pos1, pos2, len), pos1 < pos2, sorted"""
    enc = np.ascontiguousarray(enc, dtype=np.uint8)
    n = enc.size
    letter = enc < 254
    out = []
    for d in range(1, n - min_len + 1):
        eq = (enc[:n - d] == enc[d:]) & letter[:n - d]
        if eq.size < min_len:
            break
        edges = np.diff(np.concatenate([[0], eq.view(np.int8), [0]]))
        starts, ends = np.flatnonzero(edges == 1), np.flatnonzero(edges == -1)
        keep = ends - starts >= min_len
        if keep.any():
            s, ln = starts[keep], (ends - starts)[keep]
            out.append(np.stack([s, s + d, ln], axis=1))
    if not out:
        return np.zeros((0, 3), dtype=np.int64)
    return sort_records(np.concatenate(out).astype(np.int64))


def sort_records(rec):
    rec = np.asarray(rec).reshape(-1, 3).astype(np.int64)
    return rec[np.lexsort((rec[:, 2], rec[:, 1], rec[:, 0]))]


def sequence_starts(enc):
    """absolute position of the first symbol of every sequence"""
    return np.concatenate([[0], np.flatnonzero(np.asarray(enc) == 255) + 1]).astype(np.int64)


def format_lines(rec, enc):
    """`len seqnum1 relpos1 F len seqnum2 relpos2`, one line per record, in the
    order of the records (src/match/esa-mmsearch.c / querymatch display of an
    exact match)"""
    starts = sequence_starts(enc)
    rec = np.asarray(rec).reshape(-1, 3).astype(np.int64)
    s1 = np.searchsorted(starts, rec[:, 0], side="right") - 1
    s2 = np.searchsorted(starts, rec[:, 1], side="right") - 1
    return ["%d %d %d F %d %d %d" % (ln, a, p - starts[a], ln, b, q - starts[b])
            for (p, q, ln), a, b in zip(rec.tolist(), s1.tolist(), s2.tolist())]


def normalised(text):
    """sorted lines of a tool's or the reference's output: `#` lines dropped,
    runs of white space one blank"""
    if isinstance(text, bytes):
        text = text.decode("latin-1")
    return sorted(" ".join(l.split()) for l in text.splitlines() if l.strip() and not l.startswith("#"))


@functools.lru_cache(maxsize=None)
def encoded(name, protein=False):
    enc = ou.encode_fasta(ou.fixture_path(name), protein)
    enc.setflags(write=False)
    return enc


def table_order(rec, suf):
    """the records in table order: ascending table index of the suffix that
    stands first in the table, then of the other"""
    suf = np.asarray(suf).astype(np.int64)
    rank = np.empty(suf.size, dtype=np.int64)
    rank[suf] = np.arange(suf.size)
    rec = np.asarray(rec).reshape(-1, 3).astype(np.int64)
    r1, r2 = rank[rec[:, 0]], rank[rec[:, 1]]
    return rec[np.lexsort((np.maximum(r1, r2), np.minimum(r1, r2)))]


def segments(enc, suf, lcpfull, min_len):
    """what steps 1 and 2 of the device part hand to the walk, made with numpy:
    dict of idx, val, cls (one entry per suffix in a run), seg_first (one entry
    per segment and M behind them), seg_of"""
    enc = np.ascontiguousarray(enc, dtype=np.uint8)
    suf = np.asarray(suf).astype(np.int64)
    lcp = np.asarray(lcpfull).astype(np.int64)
    N = suf.size
    flag = lcp >= min_len
    flag[0] = False
    inrun = flag | np.concatenate([flag[1:], [False]])
    idx = np.flatnonzero(inrun)
    val = np.where(flag[idx], lcp[idx], 0)
    pos = suf[idx]
    left = np.where(pos > 0, enc[np.maximum(pos, 1) - 1], UNIQUE)
    cls = np.where(left >= 254, UNIQUE, left).astype(np.uint8)
    M = idx.size
    start = np.ones(M, dtype=bool)
    if M > 1:
        start[1:] = (val[1:] == 0) | (cls[1:] == UNIQUE) | (cls[1:] != cls[:-1])
    seg_first = np.concatenate([np.flatnonzero(start), [M]])
    seg_of = np.cumsum(start) - 1
    return {"idx": idx.astype(np.uint32), "val": val.astype(np.uint32), "cls": cls,
            "seg_first": seg_first.astype(np.uint32), "seg_of": seg_of.astype(np.uint32), "N": N}


WILDCARD, SEPARATOR = 254, 255


def _random(n, sigma, seed):
    return np.random.default_rng(seed).integers(0, sigma, n, dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def subject(name):
    """(enc, sigma) of a synthetic subject; shared, never written to"""
    kind, _, arg = name.partition(":")
    v = int(arg) if arg else 0
    sigma = 4
    if kind == "homopolymer":      # one run of about v suffixes, about v pairs
        enc = np.zeros(v, dtype=np.uint8)
    elif kind == "tandem":         # (ACG)^v
        enc = np.tile(np.array([0, 1, 2], dtype=np.uint8), v)
    elif kind == "copies":         # two copies of v random letters, flanks that differ
        body = _random(v, 4, 31)
        enc = np.concatenate([_random(37, 4, 32), [(body[0] + 1) % 4], body, [(body[-1] + 1) % 4],
                              _random(101, 4, 33), [(body[0] + 2) % 4], body, [(body[-1] + 2) % 4],
                              _random(29, 4, 34)]).astype(np.uint8)
    elif kind == "leftspecials":   # one 40-mer at position 0, behind N, a separator and letters
        mer = _random(40, 4, 35)
        parts = [mer]
        for k, before in enumerate([WILDCARD, SEPARATOR, 0, 1, WILDCARD, SEPARATOR, 0]):
            parts += [[(mer[-1] + 1 + k) % 4], _random(13 + k, 4, 36 + k), [before], mer]
        enc = np.concatenate(parts).astype(np.uint8)
    elif kind == "bigruns":        # two letters: runs of many suffixes
        enc = _random(v, 2, 44)
        sigma = 2
    elif kind == "protein":
        enc, sigma = _random(v, 20, 45), 20
        enc[v // 3:v // 3 + 50] = enc[20:70]
        enc[2 * v // 3:2 * v // 3 + 30] = enc[30:60]
        enc[np.random.default_rng(46).integers(0, v, 6)] = WILDCARD
        enc[v // 2] = SEPARATOR
    elif kind == "small":          # v symbols over four letters, one wildcard, one separator
        enc = _random(v, 4, 47)
        enc[v // 3] = WILDCARD
        enc[2 * v // 3] = SEPARATOR
    else:
        raise KeyError(name)
    enc = np.ascontiguousarray(enc, dtype=np.uint8)
    enc.setflags(write=False)
    return enc, sigma


@functools.lru_cache(maxsize=None)
def tables(name):
    """the oracle's tables of a synthetic subject or (`fixture:NAME[:protein]`) a fixture"""
    if name.startswith("fixture:"):
        parts = name.split(":")
        protein = len(parts) > 2
        enc, sigma = encoded(parts[1], protein), 20 if protein else 4
    else:
        enc, sigma = subject(name)
    t = ou.esa(enc, sigma)
    for a in t.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return enc, sigma, t


@functools.lru_cache(maxsize=None)
def expected(name, min_len):
    """sorted records of the brute force; shared, never written to"""
    rec = brute_force(tables(name)[0], min_len)
    rec.setflags(write=False)
    return rec


# ---- the walk of csrc/esa_maxpairs_walk.h on the CPU ------------------------------
SHIM_SRC = os.path.join(ou.ROOT, "tests", "maxpairs_walk_shim.cpp")
HEADER = os.path.join(ou.ROOT, "genometools_amd", "csrc", "esa_maxpairs_walk.h")
SHIM = os.path.join(ou.ROOT, "oracle", "_build", "libmaxpairs_walk_shim.so")


def load_shim():
    ou.build()
    if not os.path.exists(SHIM) or os.path.getmtime(SHIM) < max(os.path.getmtime(SHIM_SRC),
                                                                 os.path.getmtime(HEADER)):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-shared", "-fPIC", "-o", SHIM,
                        SHIM_SRC], check=True)
    lib = ctypes.CDLL(SHIM)
    P = ctypes.c_void_p
    lib.mp_shim_run.argtypes = [P, P, P, ctypes.c_uint32, P, P, ctypes.c_uint32, P, ctypes.c_int, P, P]
    lib.mp_shim_run.restype = ctypes.c_uint64
    return lib


def walk(lib, enc, suf, lcpfull, min_len):
    """(records in the order the walk emits them, figures: pairs, largest count of
    one entry, largest length, steps of the count pass, M, segments)"""
    g = segments(enc, suf, lcpfull, min_len)
    suf = np.ascontiguousarray(suf)
    M, nseg = g["idx"].size, g["seg_first"].size - 1
    figures = np.zeros(4, dtype=np.uint64)
    args = [g[k].ctypes.data for k in ("idx", "val", "cls")] + [M, g["seg_first"].ctypes.data,
                                                                g["seg_of"].ctypes.data, nseg, suf.ctypes.data,
                                                                suf.dtype.itemsize]
    z = lib.mp_shim_run(*args, None, figures.ctypes.data)
    out = np.full((z + 1, 3), 0xdeadbeef, dtype=np.uint64)
    assert lib.mp_shim_run(*args, out.ctypes.data, figures.ctypes.data) == z
    assert (out[z] == 0xdeadbeef).all()           # nothing written behind the count
    return out[:z].astype(np.int64), [int(f) for f in figures] + [M, nseg]
