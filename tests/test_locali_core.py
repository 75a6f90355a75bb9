"""The lane code of the local aligner (genometools_amd/csrc/esa_locali_core.h:
the column in chunks of 64 rows with the Delete chain as a prefix maximum, its
maximum, the start row that travels with a score, the walk of a single suffix
in the text), compiled with g++ and run on the CPU against the statement with
stored traces and a traceback.  No GPU: what is left for
tests/test_locali_gpu.py is the walk over the intervals around it.

The cases of tests/locali_core_cases.h -- m in {1, 2, 3, 63, 64, 65, 127, 128,
129}, five sets of scores, sigma in {2, 4}, a wildcard in the query, a
wildcard, a separator and the end at every distance from the start, a Delete
run across rows 63, 64, 65, all short queries over two letters against all
subjects of six symbols for the ties, the deepest walk the bound allows; and
the long queries: m in {191, 192, 193, 1000, 4097, 16384} with two sets of
scores, walked from where the query's tail aligns (bands in the last chunk,
every column from an unaligned row) and from where its head does (columns that
stop long before row m), Delete runs of 200 rows that hang from one letter and
runs that end on every row of a chunk beyond the last candidate, exact copies
that score 65504, 65472, 65408, 65534 and 49152 under T equal to that and one
above it, the last of them with 16384 letters and a gap of 32767, equal
maxima of which one lies in row 16384 -- run
twice: inside the library this test loads, and as a program of their own built
with -fsanitize=address,undefined, started as a child process.

The sanitized program ran 8.8 s before the long queries were added and runs
16.3 s with them (one core of the build machine; 1.5 s and 4.7 s without the
sanitizers); most of what was added is the plain statement's 16384 full
columns of the longest exact copy, whose traces take 268 MB in either run."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import locali_reference as lr
import oracle_util as ou

ROOT = ou.ROOT
SRC = [os.path.join(ROOT, "tests", f) for f in ("locali_core_shim.cpp", "locali_core_main.cpp",
                                                 "locali_core_cases.h")] + \
      [os.path.join(ROOT, "genometools_amd", "csrc", f) for f in ("esa_locali_core.h", "esa_ivwalk.h")]
SHIM = os.path.join(ROOT, "oracle", "_build", "liblocali_core_shim.so")
MAIN = os.path.join(ROOT, "oracle", "_build", "locali_core_main_san")
TALLY = ("walks", "columns", "matches", "failures", "tie_del_rep", "tie_del_ins", "tie_rep_ins", "delete_across",
         "two_maxima", "zero_cells", "depth_one", "deepest_reached", "stopped_by_special", "columns_past_three_chunks",
         "band_starts_unaligned", "stopped_before_last_row", "delete_across_three", "row_above_16000",
         "score_above_65000", "chain_dies_on_first_row", "chain_dies_on_last_row", "tie_with_last_row")


def _stale(target):
    return not os.path.exists(target) or os.path.getmtime(target) < max(os.path.getmtime(f) for f in SRC)


@pytest.fixture(scope="module")
def shim():
    ou.build()
    if _stale(SHIM):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-shared", "-fPIC", "-o", SHIM, SRC[0]], check=True)
    lib = ctypes.CDLL(SHIM)
    P, U32, U64, INT = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int
    lib.lc_shim_walk.argtypes = [P, U32, P, U64, U64, INT, INT, INT, U32, P]
    lib.lc_shim_walk.restype = U32
    lib.lc_shim_max_depth.argtypes = [U32, INT, INT]
    lib.lc_shim_max_depth.restype = U32
    lib.lc_shim_cases.argtypes = [P]
    lib.lc_shim_cases.restype = None
    return lib


def test_the_cases_inside_the_library(shim):
    fig = np.zeros(len(TALLY), dtype=np.uint64)
    shim.lc_shim_cases(fig.ctypes.data)
    t = dict(zip(TALLY, fig.tolist()))
    assert t["failures"] == 0
    assert t["walks"] > 20_000 and t["columns"] > 200_000 and t["walks"] // 50 < t["matches"] < t["walks"]
    # what the cases are there for did happen
    for event in TALLY[4:]:
        assert t[event] > 0, event
    assert t["delete_across"] >= 2 and t["deepest_reached"] >= 1


def test_the_cases_under_the_sanitizers():
    """a program with its own main, never loaded into python; the sanitizer's
    runtime is linked into it"""
    ou.build()
    if _stale(MAIN):
        subprocess.run(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-static-libasan", "-o", MAIN, SRC[1]], check=True)
    p = subprocess.run([MAIN], capture_output=True, text=True)
    assert p.returncode == 0 and p.stderr == "", (p.returncode, p.stdout, p.stderr[-2000:])
    assert p.stdout.endswith(" 0 failures\n") and int(p.stdout.split()[0]) > 20_000


def _walk(shim, q, enc, p, match, mismatch, gapextend, T):
    out = np.zeros(4, dtype=np.uint32)
    hit = shim.lc_shim_walk(q.ctypes.data, q.size, enc.ctypes.data if enc.size else None, enc.size, p, match, mismatch,
                            gapextend, T, out.ctypes.data)
    return tuple(out.tolist()) if hit else None


def test_the_depth_bound(shim):
    for m, match, gap in ((4, 5, -1), (1, 1, -1), (64, 1, -1), (10, 3, -2), (300, 2, -1), (7, 1, -5), (16384, 3, -1),
                          (16384, 1, -32767), (1000, 65, -1)):
        d = shim.lc_shim_max_depth(m, match, gap)
        assert d == lr.max_depth(m, match, gap)
        assert match * m + gap * (d - m) > 0 >= match * m + gap * (d + 1 - m)


def test_single_walks_on_the_fixtures(shim):
    """every start position of pieces of two fixtures, the walk of the lanes
    against the numpy statement, which knows no band and no chunk"""
    total = 0
    for name, scores, T in (("Duplicate.fna", (1, -1, -1), 14), ("Atinsert.fna", (2, -1, -1), 30),
                            ("Atinsert.fna", (1, -2, -2), 9)):
        enc = ou.encode_fasta(ou.fixture_path(name))[:1200].copy()
        for query in (enc[40:70].copy(), np.concatenate([enc[500:540], enc[545:620]])):
            query[query >= 254] = 254
            want = lr.matches_of_query(enc, query, *scores, T=T)
            got = {}
            for start in range(enc.size + 1):
                hit = _walk(shim, query, enc, start, *scores, T)
                if hit is not None:
                    got[start] = hit
            assert got == want, (name, scores, T, query.size)
            total += len(want)
    assert total > 10          # (the comparison is not an empty one)


def test_the_end_and_the_specials_stop_a_walk(shim):
    q = np.array([0, 1, 2, 3], dtype=np.uint8)
    enc = np.array([0, 1, 2, 3, 255, 0, 1, 254, 3, 0, 1, 2], dtype=np.uint8)
    one = (1, -1, -1)
    assert _walk(shim, q, enc, 0, *one, 4) == (4, 4, 0, 4)        # ends on the last letter before the separator
    assert _walk(shim, q, enc, 1, *one, 3) == (3, 3, 1, 3)        # cgt
    assert _walk(shim, q, enc, 1, *one, 4) is None                # the separator is never read past
    assert _walk(shim, q, enc, 5, *one, 2) == (2, 2, 0, 2)        # ac, then the wildcard ends the columns
    assert _walk(shim, q, enc, 5, *one, 3) is None
    assert _walk(shim, q, enc, 9, *one, 3) == (3, 3, 0, 3)        # ends at n - 1
    assert _walk(shim, q, enc, 9, *one, 4) is None
    assert _walk(shim, q, enc, 12, *one, 1) is None and _walk(shim, q, enc[:0], 0, *one, 1) is None
    assert _walk(shim, q, enc, 11, *one, 1) == (1, 1, 2, 1)       # T <= match: a match at depth 1
    wild = np.array([0, 254, 2], dtype=np.uint8)                  # a wildcard in the query equals nothing
    assert _walk(shim, wild, enc, 0, 3, -1, -1, 5) == (3, 5, 0, 3)
    assert _walk(shim, wild, enc, 0, 3, -1, -1, 6) is None
