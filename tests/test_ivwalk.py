"""The search both interval walkers share (genometools_amd/csrc/esa_ivwalk.h:
iv_symbol, iv_right_bound_by, iv_right_bound), compiled with g++ and run on the
CPU with the 64 lanes as a loop, against a linear scan: the first index behind
cur whose entry differs, or end.  No GPU: tests/test_tagmatch_gpu.py and
tests/test_locali_gpu.py run the walks around it.

The cases of tests/ivwalk_cases.h -- every boundary of the spans 1 to 300;
spans around 64^2, 64^3 and 2^24 up to the whole of the largest table, at its
start, at its end and ending at 2^32 - 1, with the boundary around the first
and the last probe; tables in memory with entries of 4 and of 8 bytes, entries
that are no position and positions too close to the end; tables that are no
index -- run twice: inside the library this test loads, and as a program of
their own built with -fsanitize=address,undefined (a probe that wraps at 2^32
reads in front of the table), started as a child process.  The table of a large
span is a callable, so nothing of that size is allocated."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import oracle_util as ou

ROOT = ou.ROOT
SRC = [os.path.join(ROOT, "tests", f) for f in ("ivwalk_shim.cpp", "ivwalk_main.cpp", "ivwalk_cases.h")] + \
      [os.path.join(ROOT, "genometools_amd", "csrc", "esa_ivwalk.h")]
SHIM = os.path.join(ROOT, "oracle", "_build", "libivwalk_shim.so")
MAIN = os.path.join(ROOT, "oracle", "_build", "ivwalk_main_san")
TALLY = ("cases", "failures", "small", "large", "tables", "no_index", "no_position", "behind_the_end", "letters",
         "max_rounds")


def _stale(target):
    return not os.path.exists(target) or os.path.getmtime(target) < max(os.path.getmtime(f) for f in SRC)


@pytest.fixture(scope="module")
def shim():
    ou.build()
    if _stale(SHIM):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-shared", "-fPIC", "-o", SHIM, SRC[0]], check=True)
    lib = ctypes.CDLL(SHIM)
    P, U32, U64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
    lib.iv_shim_right_bound.argtypes = [P, U64, P, U32, U32, U32, U32, P]
    lib.iv_shim_right_bound.restype = U32
    lib.iv_shim_cases.argtypes = [P]
    lib.iv_shim_cases.restype = None
    return lib


def test_the_cases_inside_the_library(shim):
    fig = np.zeros(len(TALLY), dtype=np.uint64)
    shim.iv_shim_cases(fig.ctypes.data)
    t = dict(zip(TALLY, fig.tolist()))
    assert t["failures"] == 0, t
    # every boundary of the spans 1 to 300 at three places: 3 * (1 + ... + 300)
    assert t["small"] == 3 * 300 * 301 // 2
    # ten spans at three places with up to eleven boundaries each, some of which coincide or fall outside
    assert 10 * 3 * 8 <= t["large"] <= 10 * 3 * 11
    assert t["tables"] > 50_000 and t["no_index"] == 3 * 10 * 7 * 8
    assert t["cases"] == t["small"] + t["large"] + t["tables"] + t["no_index"]
    # the three cases of iv_symbol
    assert min(t["no_position"], t["behind_the_end"], t["letters"]) > 100, t
    # a round leaves fewer than span / 64 + 1 entries, so six do for a span below 2^32; six are seen, so
    # the spans of the whole table have been searched
    assert t["max_rounds"] == 6


def test_the_cases_under_the_sanitizers():
    """a program with its own main, never loaded into python; the sanitizer's
    runtime is linked into it"""
    ou.build()
    if _stale(MAIN):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-static-libasan", "-o", MAIN, SRC[1]], check=True)
    p = subprocess.run([MAIN], capture_output=True, text=True)
    assert p.returncode == 0 and p.stderr == "", (p.returncode, p.stdout, p.stderr[-2000:])
    assert p.stdout.endswith(" at most 6 rounds, 0 failures\n") and int(p.stdout.split()[0]) > 180_000


def _symbols(enc, suf, d):
    """iv_symbol of every table entry, stated with numpy"""
    at = suf.astype(np.uint64) + np.uint64(d)
    padded = np.concatenate([enc, np.full(d + 2, 255, dtype=np.uint8)])
    return np.where(suf.astype(np.uint64) >= enc.size, 255, padded[np.minimum(at, enc.size).astype(np.int64)])


@pytest.mark.parametrize("dtype", [np.uint32, np.uint64])
def test_the_children_of_a_real_index(shim, dtype):
    """the first four levels of the walk over the suffix table of a fixture: every
    child's right bound is where the symbols at its depth change"""
    enc = ou.encode_fasta(ou.fixture_path("Atinsert.fna"))[:3000].copy()
    suf = ou.esa(enc)["suf"].astype(dtype)
    rounds = ctypes.c_uint32(0)
    children = wide = 0
    level = [(0, suf.size)]
    for d in range(4):
        sym = _symbols(enc, suf, d)
        below = []
        for lo, end in level:
            cur = lo
            while cur < end and sym[cur] < 254:          # (specials end a level: they lie in no order)
                e = shim.iv_shim_right_bound(enc.ctypes.data, enc.size, suf.ctypes.data, suf.itemsize, cur, end, d,
                                             ctypes.byref(rounds))
                differ = np.flatnonzero(sym[cur + 1:end] != sym[cur])
                assert e == (cur + 1 + differ[0] if differ.size else end), (d, cur, end)
                assert rounds.value <= 2          # (a span of at most 64 * 64)
                children += 1
                wide += e - cur > 64
                below.append((cur, e))
                cur = e
        level = below
    assert children > 50 and wide > 10          # (the comparison is not an empty one)
