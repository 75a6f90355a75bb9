"""What one lane of the suffix-prefix match kernels does
(genometools_amd/csrc/esa_spm_core.h: the terminal test, the read start test,
the interval of a terminal suffix, the read starts inside it and the record of a
candidate), compiled with g++ and run on the CPU over every table entry and
every candidate, against the brute force of tests/spm_reference.py: every
triple, in the stated order.  The tables are the oracle's.  No GPU: what is left
for tests/test_spm_gpu.py is the kernels around it, the compaction, the scans
and the C ABI."""
import ctypes
import functools
import math
import os
import subprocess

import numpy as np
import pytest

import oracle_util as ou
import spm_reference as sr

ROOT = ou.ROOT
SHIM_SRC = os.path.join(ROOT, "tests", "spm_core_shim.cpp")
HEADERS = [os.path.join(ROOT, "genometools_amd", "csrc", h)
           for h in ("esa_spm_core.h", "esa_qmatch_core.h", "esa_mstat_search.h")]
SHIM = os.path.join(ROOT, "oracle", "_build", "libspm_core_shim.so")
DNA = ["Atinsert.fna", "Duplicate.fna", "Random-Small.fna", "Random.fna", "Random159.fna",
       "Random160.fna", "RandomN.fna", "TTT-small.fna", "trna_glutamine.fna"]
FIGURES = ("terminals", "starts", "separators", "matches", "min_width", "max_width", "max_count", "search_symbols")


@pytest.fixture(scope="module")
def shim():
    ou.build()
    if not os.path.exists(SHIM) or os.path.getmtime(SHIM) < max(os.path.getmtime(f) for f in [SHIM_SRC] + HEADERS):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-shared", "-fPIC", "-o", SHIM, SHIM_SRC],
                       check=True)
    lib = ctypes.CDLL(SHIM)
    P = ctypes.c_void_p
    lib.sp_shim_run.argtypes = [P, ctypes.c_uint64, P, ctypes.c_int, P, P, ctypes.c_uint64, ctypes.c_uint32, P, P]
    lib.sp_shim_run.restype = ctypes.c_uint64
    return lib


def _framed(a):
    """cut out of a larger array filled with wildcards, so that a read beside it finds neither a letter nor a
    separator"""
    big = np.full(a.size + 64, 254, dtype=np.uint8)
    big[32:32 + a.size] = a
    return big[32:32 + a.size]


def _run(lib, enc, t, width, min_len):
    """(records in order as int64 rows, figures) for the oracle's tables t"""
    enc = _framed(np.asarray(enc, dtype=np.uint8))
    suf = np.ascontiguousarray(t["suf"].astype(width))
    lcp, llv = np.ascontiguousarray(t["lcp"]), np.ascontiguousarray(t["llv"], dtype=np.uint64).reshape(-1)
    fig = np.zeros(len(FIGURES), dtype=np.uint64)
    args = (enc.ctypes.data, enc.size, suf.ctypes.data, suf.dtype.itemsize, lcp.ctypes.data,
            llv.ctypes.data if llv.size else None, llv.size // 2, min_len)
    z = lib.sp_shim_run(*args, None, fig.ctypes.data)
    assert z != 2 ** 64 - 1, "an interval without its own terminal suffix"
    out = np.zeros((z, 3), dtype=np.int64)
    assert lib.sp_shim_run(*args, out.ctypes.data, fig.ctypes.data) == z
    return out, dict(zip(FIGURES, fig.tolist()))


def _agree(lib, enc, min_len, t=None, widths=(np.uint64, np.uint32)):
    """both table widths against the brute force; the brute force's rows"""
    enc = np.ascontiguousarray(enc, dtype=np.uint8)
    t = ou.esa(enc, 4) if t is None else t
    rows, terminals, starts = sr.brute_force(enc, min_len)
    want = sr.in_order(rows, t["suf"])
    for width in widths:
        got, fig = _run(lib, enc, t, width, min_len)
        assert np.array_equal(got, want)
        assert (fig["matches"], fig["terminals"], fig["starts"]) == (want.shape[0], terminals, starts)
        assert fig["separators"] == np.count_nonzero(enc == 255)
        # no kept interval has width 1: the rule of the trivial triple
        assert terminals == 0 or fig["min_width"] >= 2
        assert fig["max_count"] == (np.unique(rows[:, 3], return_counts=True)[1].max() if rows.size else 0)
        # derived: each of the two searches of a terminal suffix of h letters makes at
        # most ceil(log2 N) + 1 comparisons of at most h symbols and the one that ends it
        longest = max((l for _, l in sr.units(enc)), default=0)
        assert fig["search_symbols"] <= terminals * 2 * (math.ceil(math.log2(enc.size + 1)) + 1) * (longest + 1)
    return rows


@functools.lru_cache(maxsize=None)
def _reads(name):
    enc = sr.mirrored(ou.encode_fasta(os.path.join(ou.GOLDEN_DIR, "spm", name)))
    t = ou.esa(enc, 4)
    enc.setflags(write=False)
    return enc, t


@pytest.mark.parametrize("name,min_len", [("mixed.fna", 12), ("mixed.fna", 30), ("mixed.fna", 61),
                                          ("equal.fna", 20), ("equal.fna", 36), ("equal.fna", 37)])
def test_golden_read_sets_mirrored(shim, name, min_len):
    enc, t = _reads(name)
    rows = _agree(shim, enc, min_len, t)
    assert (rows.shape[0] == 0) == (min_len in (61, 37))


@pytest.mark.parametrize("name", DNA)
def test_fixtures_unmirrored(shim, name):
    """few sequences, long ones; the self-overlaps of a sequence and nothing else where it is alone"""
    enc = ou.encode_fasta(ou.fixture_path(name))
    t = ou.esa(enc, 4)
    for min_len in (1, 3, 8):
        _agree(shim, enc, min_len, t)


def test_wildcards_inside_and_at_the_ends_of_reads(shim):
    """a wildcard ends the letters of a suffix and of a prefix: reads that would overlap across one do not; a
    read that starts or ends with one is no read start, or has no terminal suffix"""
    enc = sr.wildcard_reads()
    for data in (enc, sr.mirrored(enc)):
        for min_len in (1, 10, 19, 30):
            rows = _agree(shim, data, min_len)
        assert rows.shape[0] > 20
        assert not any(s == t == 3 and k == 50 for s, t, k, _, _ in rows.tolist())


def test_long_reads_consult_llv(shim):
    """reads of 300 and 600 letters that overlap by 280 and 400: LCP bytes of 255"""
    enc = sr.long_reads()
    t = ou.esa(enc, 4)
    assert t["llv"].shape[0] > 100 and np.count_nonzero(t["lcp"] == 255) == t["llv"].shape[0]
    for min_len in (20, 255, 256, 280, 400, 401, 600, 601):
        rows = _agree(shim, enc, min_len, t)
        lens = sorted(set(rows[:, 2].tolist()))
        assert lens == [k for k in (200, 280, 300, 400, 600) if k >= min_len]
    assert rows.shape[0] == 0


@pytest.mark.parametrize("count", [30, 63, 64, 65, 66, 200])
def test_many_copies_of_one_read(shim, count):
    """copies of one 40-letter read: every copy with every copy at the whole length, and the shorter
    overlaps of the read with itself.  The interval of the read holds `count` terminal suffixes, the
    k-th of them k entries from its start and count - 1 - k from its end: around 64 copies the walk
    over .lcp ends just before, at and behind the point where a lane searches the text instead"""
    read = np.array([0, 1] * 20, dtype=np.uint8)
    enc = sr.copies(read, count)
    rows = _agree(shim, enc, 10)
    assert rows.shape[0] == count * count * 16    # lengths 40, 38, ..., 10
    if count == 30:
        alone = _agree(shim, read, 10)            # one read alone: the whole length occurs once only
        assert sorted(alone[:, 2].tolist()) == list(range(10, 40, 2))


@pytest.mark.parametrize("count", [0, 1, 2, 255, 256, 257])
def test_sets_with_a_given_number_of_terminal_suffixes(shim, count):
    """what tests/test_spm_gpu.py sizes its tiles with: pairs of duplicates give two terminal suffixes and
    four matches each, a read inside a longer one gives one and its trivial triple"""
    enc = sr.counted_terminals(count)
    rows, terminals, _ = sr.brute_force(enc, 30)
    assert terminals == count and rows.shape[0] == 4 * (count // 2) + count % 2
    if count:
        _agree(shim, enc, 30)
