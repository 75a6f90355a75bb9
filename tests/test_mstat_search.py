"""The search of one query position (genometools_amd/csrc/esa_mstat_search.h) --
the code every lane of the matching statistics kernel runs -- compiled with g++
and run on the CPU over every position, against the brute force of
tests/mstat_reference.py.  No GPU: what is left for tests/test_mstat_gpu.py is
the kernel around it, the memory it is given and the C ABI."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import mstat_reference as mr
import oracle_util as ou
from genometools_amd import mstat

ROOT = ou.ROOT
SHIM_SRC = os.path.join(ROOT, "tests", "mstat_search_shim.cpp")
HEADER = os.path.join(ROOT, "genometools_amd", "csrc", "esa_mstat_search.h")
SHIM = os.path.join(ROOT, "oracle", "_build", "libmstat_search_shim.so")
NO_CAP = (1 << 32) - 1
DNA = ["Atinsert.fna", "Duplicate.fna", "Random-Small.fna", "Random.fna", "Random159.fna",
       "Random160.fna", "RandomN.fna", "TTT-small.fna", "trna_glutamine.fna"]


@pytest.fixture(scope="module")
def shim():
    ou.build()
    if not os.path.exists(SHIM) or os.path.getmtime(SHIM) < max(os.path.getmtime(SHIM_SRC),
                                                                 os.path.getmtime(HEADER)):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-shared", "-fPIC", "-o", SHIM,
                        SHIM_SRC], check=True)
    lib = ctypes.CDLL(SHIM)
    P = ctypes.c_void_p
    lib.mst_shim_run.argtypes = [P, ctypes.c_uint64, P, ctypes.c_int, P, ctypes.c_uint64, ctypes.c_uint32,
                                 ctypes.c_int, P, P, ctypes.POINTER(ctypes.c_uint64)]
    lib.mst_shim_run.restype = ctypes.c_uint64
    return lib


def _run(lib, enc, suf, query, matstat, max_len=0):
    """(length, subjectpos, symbols compared, reruns); the arrays are cut out of
    larger ones filled with specials, so that a read beside them finds no letter"""
    def framed(a):
        big = np.full(a.size + 64, 255, dtype=np.uint8)
        big[32:32 + a.size] = a
        return big[32:32 + a.size]
    enc, query = framed(np.asarray(enc, dtype=np.uint8)), framed(np.asarray(query, dtype=np.uint8))
    suf = np.ascontiguousarray(suf)
    length = np.zeros(query.size, dtype=np.uint32)
    pos = np.zeros(query.size, dtype=np.uint64)
    compared = ctypes.c_uint64()
    reruns = lib.mst_shim_run(enc.ctypes.data, enc.size, suf.ctypes.data, suf.dtype.itemsize, query.ctypes.data,
                              query.size, max_len + 1 if max_len else NO_CAP, int(matstat), length.ctypes.data,
                              pos.ctypes.data, ctypes.byref(compared))
    return length, pos, compared.value, reruns


def _agree(lib, enc, suf, query, want, max_len=0):
    ms, w, mu = want
    length, pos, _, _ = _run(lib, enc, suf, query, True, max_len)
    unique, _, _, _ = _run(lib, enc, suf, query, False, max_len)
    if max_len == 0:
        assert np.array_equal(length, ms) and np.array_equal(pos, w) and np.array_equal(unique, mu)
    else:
        assert np.array_equal(length, mr.capped(ms, max_len))
        assert np.array_equal(pos[ms <= max_len], w[ms <= max_len])
        assert np.array_equal(unique, mr.capped(mu, max_len))


@pytest.mark.parametrize("width", [np.uint64, np.uint32])
@pytest.mark.parametrize("subject", DNA)
def test_fixtures_pairwise(shim, subject, width):
    enc, suf = mr.encoded(subject, False), mr.suffix_table(subject, False).astype(width)
    for query in DNA:
        if query != subject:
            want = mr.expected(subject, query, False)
            _agree(shim, enc, suf, mr.encoded(query, False), want)
            _agree(shim, enc, suf, mr.encoded(query, False), want, max_len=20)


def test_planted_lengths_and_every_alignment(shim):
    """copies of lengths around the word comparison's sizes, from subject offsets
    0..33, each followed by a letter that differs, a wildcard, a separator, the end"""
    _, word, word_min = mstat.geometry()
    rng = np.random.default_rng(21)
    enc = rng.integers(0, 4, 5000, dtype=np.uint8)
    enc[1000:1005] = 254
    enc[[2000, 3500]] = 255
    suf = ou.esa(enc, 4)["suf"]
    lengths = sorted({1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257, word_min - 1, word_min,
                      word_min + 1, word - 1, word, word + 1})
    parts, offset = [], 0
    for k, length in enumerate(lengths * 2):
        after = [(int(enc[offset + length]) + 1) % 4, 254, 255][k % 3]
        parts += [enc[offset:offset + length], np.array([after], dtype=np.uint8)]
        offset = (offset + 1) % 34
    query = np.concatenate(parts + [enc[4960:], rng.integers(0, 4, 9, dtype=np.uint8), enc[1960:2000],
                                    enc[990:1000], enc[4700:]])
    want = mr.brute_force(enc, suf, query)
    for max_len in (0, word, 5):
        _agree(shim, enc, suf, query, want, max_len)


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65])
def test_runs_of_one_letter(shim, n):
    enc = np.full(n, 3, dtype=np.uint8)
    suf = ou.esa(enc, 4)["suf"]
    for query in (enc, np.full(n + 1, 3, dtype=np.uint8), np.array([3, 0, 3, 3], dtype=np.uint8)):
        _agree(shim, enc, suf, query, mr.brute_force(enc, suf, query))


def test_a_copy_of_the_subject_and_the_cap(shim):
    half = np.random.default_rng(26).integers(0, 4, 1500, dtype=np.uint8)
    enc = np.concatenate([half, half])
    suf = ou.esa(enc, 4)["suf"]
    want = mr.brute_force(enc, suf, enc)
    ms, w, mu = want
    _agree(shim, enc, suf, enc, want)
    _agree(shim, enc, suf, enc, want, max_len=20)
    _, _, uncapped, reruns = _run(shim, enc, suf, enc, True)
    assert uncapped > ms.sum() and reruns == 0
    _, _, capped, reruns = _run(shim, enc, suf, enc, True, 20)
    # (at most 15 steps of each of the two searches, 22 symbols a step)
    assert capped < 40 * 21 * enc.size < ms.sum() and reruns == 0
    _, _, _, reruns = _run(shim, enc, suf, enc, False, 20)
    rest = enc.size - np.arange(enc.size)
    assert reruns == np.count_nonzero((ms >= 21) & ((mu == 0) | (mu > 21)) & (rest > 21))


def test_other_alphabets(shim):
    rng = np.random.default_rng(23)
    for sigma in (20, 2):
        enc = rng.integers(0, sigma, 2000, dtype=np.uint8)
        enc[rng.integers(0, 2000, 8)] = 254
        enc[700] = 255
        suf = ou.esa(enc, sigma)["suf"]
        query = np.concatenate([enc[7:300], rng.integers(0, sigma, 200, dtype=np.uint8), [254], enc[1900:],
                                [sigma + 1], enc[690:720]]).astype(np.uint8)
        _agree(shim, enc, suf, query, mr.brute_force(enc, suf, query))
