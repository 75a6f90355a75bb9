"""The lane code of the tag matcher (genometools_amd/csrc/esa_tagmatch_core.h:
the step of the bit-vector column, the tests for success and for the end, the
walk of a single suffix in the text), compiled with g++ and run on the CPU
against the plain table of edit distances.  No GPU: what is left for
tests/test_tagmatch_gpu.py is the walk over the intervals around it.

The cases of tests/tagmatch_core_cases.h -- m in {1, 2, 3, 63, 64}, K in {0, 1,
2, m - 1}, sigma in {2, 4}, subjects with a separator, a wildcard and the end at
every distance from the start -- run twice: inside the library this test loads,
and as a program of their own built with -fsanitize=address,undefined (a shift
by 64 at m = 64 is the classic fault of this algorithm), started as a child
process."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import oracle_util as ou
import tagmatch_reference as tr

ROOT = ou.ROOT
SRC = [os.path.join(ROOT, "tests", f) for f in ("tagmatch_core_shim.cpp", "tagmatch_core_main.cpp",
                                                 "tagmatch_core_cases.h")] + \
      [os.path.join(ROOT, "genometools_amd", "csrc", f) for f in ("esa_tagmatch_core.h", "esa_ivwalk.h")]
SHIM = os.path.join(ROOT, "oracle", "_build", "libtagmatch_core_shim.so")
MAIN = os.path.join(ROOT, "oracle", "_build", "tagmatch_core_main_san")


def _stale(target):
    return not os.path.exists(target) or os.path.getmtime(target) < max(os.path.getmtime(f) for f in SRC)


@pytest.fixture(scope="module")
def shim():
    ou.build()
    if _stale(SHIM):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-shared", "-fPIC", "-o", SHIM, SRC[0]], check=True)
    lib = ctypes.CDLL(SHIM)
    P, U32, U64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
    lib.tm_shim_walk.argtypes = [P, U32, U32, ctypes.c_int, P, U64, U64, P]
    lib.tm_shim_walk.restype = U32
    lib.tm_shim_columns.argtypes = [P, U32, U32, P, U32, P, P]
    lib.tm_shim_columns.restype = U32
    lib.tm_shim_cases.argtypes = [P]
    lib.tm_shim_cases.restype = None
    return lib


def test_the_cases_inside_the_library(shim):
    fig = np.zeros(4, dtype=np.uint64)
    shim.tm_shim_cases(fig.ctypes.data)
    walks, columns, matches, failures = fig.tolist()
    assert failures == 0
    assert walks > 2_000_000 and columns > 4_000_000 and walks // 10 < matches < walks


def test_the_cases_under_the_sanitizers():
    """a program with its own main, never loaded into python; the sanitizer's
    runtime is linked into it"""
    ou.build()
    if _stale(MAIN):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-static-libasan", "-o", MAIN, SRC[1]], check=True)
    p = subprocess.run([MAIN], capture_output=True, text=True)
    assert p.returncode == 0 and p.stderr == "", (p.returncode, p.stdout, p.stderr[-2000:])
    assert p.stdout.endswith(" 0 failures\n") and int(p.stdout.split()[0]) > 2_000_000


def _walk(shim, tag, K, wild, enc, p):
    dist = ctypes.c_uint32(0)
    length = shim.tm_shim_walk(tag.ctypes.data, tag.size, K, int(wild), enc.ctypes.data if enc.size else None,
                               enc.size, p, ctypes.byref(dist))
    return (length, dist.value) if length else None


def test_columns_against_the_python_table(shim):
    """the same judge as the brute force of tests/tagmatch_reference.py has"""
    rng = np.random.default_rng(5)
    for m, K in ((1, 0), (5, 2), (12, 3), (33, 4), (63, 62), (64, 0), (64, 2), (64, 63)):
        tag = rng.integers(0, 4, m).astype(np.uint8)
        text = np.concatenate([tag[:m // 2], rng.integers(0, 4, 3), tag[m // 2:], rng.integers(0, 4, K + 2)]).astype(np.uint8)
        text[rng.integers(0, text.size)] = 254
        rows, vals = np.zeros(text.size, dtype=np.uint32), np.zeros(text.size, dtype=np.uint32)
        steps = shim.tm_shim_columns(tag.ctypes.data, m, K, text.ctypes.data, text.size, rows.ctypes.data,
                                     vals.ctypes.data)
        D = tr.dp_table(tag, text)
        assert steps >= 1
        for d in range(1, steps + 1):
            below = np.flatnonzero(D[:, d] <= K)
            if below.size == 0:
                assert rows[d - 1] == tr.NO_K and d == steps
            else:
                assert (rows[d - 1], vals[d - 1]) == (below[-1], D[below[-1], d]), (m, K, d)
                assert rows[d - 1] != m or d == steps
        assert steps == text.size or rows[steps - 1] in (m, tr.NO_K)


def test_single_walks_on_the_fixtures(shim):
    """every start position of two fixtures, the walk against the brute force"""
    total = 0
    for name, K, wild in (("Duplicate.fna", 1, False), ("Atinsert.fna", 2, True), ("Atinsert.fna", 2, False)):
        enc = ou.encode_fasta(ou.fixture_path(name))[:1500].copy()
        for tag in (enc[40:52].copy(), enc[700:764].copy()):
            tag[tag >= 254] = 0
            p, length, dist = tr.strand_matches(enc, tag, K, wild)
            want = {int(a): (int(b), int(c)) for a, b, c in zip(p, length, dist)}
            got = {}
            for start in range(enc.size):
                hit = _walk(shim, tag, K, wild, enc, start)
                if hit is not None:
                    got[start] = hit
            assert got == want, (name, K, wild, tag.size)
            total += len(want)
    assert total > 10          # (the comparison is not an empty one)


def test_the_end_and_the_specials_stop_a_walk(shim):
    tag = np.array([0, 1, 2, 3], dtype=np.uint8)
    enc = np.array([0, 1, 2, 3, 255, 0, 1, 254, 3, 0, 1, 2], dtype=np.uint8)
    assert _walk(shim, tag, 0, False, enc, 0) == (4, 0)          # ends on the last letter before the separator
    assert _walk(shim, tag, 1, False, enc, 1) == (3, 1)          # cgt, the same: the separator is never read past
    assert _walk(shim, tag, 1, False, enc, 2) is None            # gt| would need one more symbol
    assert _walk(shim, tag, 1, True, enc, 5) == (4, 1)           # ac?t: the wildcard as a symbol that equals nothing
    assert _walk(shim, tag, 1, False, enc, 5) is None            # ... and not passed: ac is two away
    assert _walk(shim, tag, 2, False, enc, 5) == (2, 2)
    assert _walk(shim, tag, 1, False, enc, 9) == (3, 1)          # ends at n - 1
    assert _walk(shim, tag, 0, False, enc, 9) is None            # would need one more symbol
    assert _walk(shim, tag, 1, False, enc, 12) is None and _walk(shim, tag, 1, False, enc[:0], 0) is None
    assert _walk(shim, tag, 3, False, enc, 11) == (1, 3)
