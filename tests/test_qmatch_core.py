"""What one lane of the query match kernels does
(genometools_amd/csrc/esa_qmatch_core.h: the interval of a query position, the
left-maximality test and the right extension of a candidate), compiled with g++
and run on the CPU over every position and every candidate, against the brute
force of tests/qmatch_reference.py.  No GPU: what is left for
tests/test_qmatch_gpu.py is the kernels around it, the scans, the compaction and
the C ABI."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import oracle_util as ou
import qmatch_reference as qr

ROOT = ou.ROOT
SHIM_SRC = os.path.join(ROOT, "tests", "qmatch_core_shim.cpp")
HEADERS = [os.path.join(ROOT, "genometools_amd", "csrc", h) for h in ("esa_qmatch_core.h", "esa_mstat_search.h")]
SHIM = os.path.join(ROOT, "oracle", "_build", "libqmatch_core_shim.so")
DNA = ["Atinsert.fna", "Duplicate.fna", "Random-Small.fna", "Random.fna", "Random159.fna",
       "Random160.fna", "RandomN.fna", "TTT-small.fna", "trna_glutamine.fna"]
FIGURES = ("candidates", "seeds", "max_width", "search_symbols", "extension_symbols")


@pytest.fixture(scope="module")
def shim():
    ou.build()
    if not os.path.exists(SHIM) or os.path.getmtime(SHIM) < max(os.path.getmtime(f) for f in [SHIM_SRC] + HEADERS):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-shared", "-fPIC", "-o", SHIM, SHIM_SRC],
                       check=True)
    lib = ctypes.CDLL(SHIM)
    P = ctypes.c_void_p
    lib.qm_shim_run.argtypes = [P, ctypes.c_uint64, P, ctypes.c_int, P, ctypes.c_uint64, ctypes.c_uint32, P, P, P, P]
    lib.qm_shim_run.restype = ctypes.c_uint64
    return lib


def _framed(a):
    """cut out of a larger array filled with specials, so that a read beside it finds no letter"""
    big = np.full(a.size + 64, 255, dtype=np.uint8)
    big[32:32 + a.size] = a
    return big[32:32 + a.size]


def _run(lib, enc, suf, query, min_len):
    """(records in order as int32 rows, lo, width, figures)"""
    enc, query = _framed(np.asarray(enc, dtype=np.uint8)), _framed(np.asarray(query, dtype=np.uint8))
    suf = np.ascontiguousarray(suf)
    lo, width = np.zeros(query.size, dtype=np.uint32), np.zeros(query.size, dtype=np.uint32)
    fig = np.zeros(5, dtype=np.uint64)
    args = (enc.ctypes.data, enc.size, suf.ctypes.data, suf.dtype.itemsize, query.ctypes.data, query.size, min_len,
            lo.ctypes.data, width.ctypes.data)
    kept = lib.qm_shim_run(*args, None, fig.ctypes.data)
    out = np.zeros((kept, 3), dtype=np.int32)
    assert lib.qm_shim_run(*args, out.ctypes.data, fig.ctypes.data) == kept
    return out, lo, width, dict(zip(FIGURES, fig.tolist()))


def _occurrences(runs, m, min_len):
    """how often the min_len symbols from every query position occur in the
    subject: a run of len letters on a diagonal holds len - min_len + 1 of them"""
    runs = runs[runs[:, 2] >= min_len].astype(np.int64)
    step = np.zeros(m + 1, dtype=np.int64)
    np.add.at(step, runs[:, 1], 1)
    np.add.at(step, runs[:, 1] + runs[:, 2] - min_len + 1, -1)
    return np.cumsum(step)[:m]


def _agree(lib, enc, suf, query, min_len, runs):
    """runs: the brute force's records of minimum length 1, in order"""
    want = runs[runs[:, 2] >= min_len]
    got, lo, width, fig = _run(lib, enc, suf, query, min_len)
    assert np.array_equal(got, want)
    count = _occurrences(runs, len(query), min_len)
    assert np.array_equal(width, count)
    assert (lo.astype(np.int64) + width <= len(enc)).all()
    assert fig["candidates"] == count.sum() and fig["seeds"] == np.count_nonzero(count)
    assert fig["max_width"] == (count.max() if count.size else 0)
    # derived: an extension looks at the len - L letters behind the seed and at the
    # symbol that ends it; a search makes at most ceil(log2 N) comparisons of at
    # most L symbols and the one that ends it, twice a position
    assert fig["extension_symbols"] <= int((want[:, 2].astype(np.int64) - min_len + 1).sum())
    steps = 2 * math.ceil(math.log2(len(enc) + 1)) + 2
    assert fig["search_symbols"] <= len(query) * steps * (min_len + 1)
    return fig


@pytest.mark.parametrize("subject", DNA)
def test_fixtures_pairwise(shim, subject):
    enc, suf = qr.encoded(subject), qr.suffix_table(subject)
    for k, name in enumerate(q for q in DNA if q != subject):
        query = qr.encoded(name)
        runs = qr.in_order(qr.brute_force(enc, query, 1), suf)
        for min_len in (1, 8, 14):
            _agree(shim, enc, suf.astype(np.uint32 if (k + min_len) % 2 else np.uint64), query, min_len, runs)


def _both_widths(shim, enc, query, min_len, sigma=4):
    suf = ou.esa(enc, sigma)["suf"]
    runs = qr.in_order(qr.brute_force(enc, query, 1), suf)
    fig = _agree(shim, enc, suf, query, min_len, runs)
    assert _agree(shim, enc, suf.astype(np.uint32), query, min_len, runs) == fig
    return fig, runs[runs[:, 2] >= min_len]


def test_one_letter(shim):
    """A^300 against A^40: every query position is a seed of 300 - L + 1
    candidates, of which only those at p = 0 or i = 0 are left-maximal"""
    enc, query = np.zeros(300, dtype=np.uint8), np.zeros(40, dtype=np.uint8)
    for min_len in (1, 16, 40):
        fig, rec = _both_widths(shim, enc, query, min_len)
        assert fig["seeds"] == 41 - min_len and fig["max_width"] == 301 - min_len
        assert fig["candidates"] == (41 - min_len) * (301 - min_len)
        assert rec.shape[0] == (301 - min_len) + (40 - min_len)
    assert _both_widths(shim, enc, query, 41)[0]["candidates"] == 0
    assert _both_widths(shim, query, enc, 16)[1].shape[0] == 25 + 284


def test_period_three(shim):
    enc = np.tile(np.array([0, 1, 2], dtype=np.uint8), 200)
    query = np.concatenate([np.tile(np.array([1, 2, 0], dtype=np.uint8), 20), [3], enc[:50], [254], enc[1:30]])
    for min_len in (1, 5, 29, 50, 61):
        _both_widths(shim, enc, query.astype(np.uint8), min_len)


def test_specials_only_and_specials_around(shim):
    rng = np.random.default_rng(31)
    enc = rng.integers(0, 4, 3000, dtype=np.uint8)
    enc[[0, 999, 2999]] = 254
    enc[[1500, 1501]] = 255
    wild = np.full(70, 254, dtype=np.uint8)
    fig, rec = _both_widths(shim, enc, wild, 1)
    assert fig["candidates"] == 0 and fig["search_symbols"] <= 70 * 26 * 2 and rec.shape[0] == 0
    # copies that touch the specials and the ends of both sequences
    query = np.concatenate([enc[1:40], [255], enc[980:1020], [254], enc[1480:1520], enc[2960:], [255], enc[:30]])
    for min_len in (1, 12, 20):
        _both_widths(shim, enc, query.astype(np.uint8), min_len)


def test_protein_fixture(shim):
    enc, query = qr.encoded("sw100K1.fsa", True), qr.encoded("sw100K2.fsa", True)
    for min_len in (1, 4):
        fig, rec = _both_widths(shim, enc, query, min_len, sigma=20)
    assert rec.shape[0] == 388
