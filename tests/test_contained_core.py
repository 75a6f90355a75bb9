"""What one lane of the contained-read kernels does
(genometools_amd/csrc/esa_contained_core.h: what a sequence of the mirrored set
finds out about itself, the verdict of a read from its two images, the symbols
of the compacted and of the mirrored set), compiled with g++ and run on the CPU
over every read, against the brute force of tests/prefilter_reference.py.  The
tables are the oracle's.  No GPU: what is left for tests/test_contained_gpu.py
is the kernels around it, the ballots, the scan and the C ABI."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import oracle_util as ou
import prefilter_reference as pr
import spm_reference as sr
from spmred_reference import revcomp

ROOT = ou.ROOT
SHIM_SRC = os.path.join(ROOT, "tests", "contained_core_shim.cpp")
HEADERS = [os.path.join(ROOT, "genometools_amd", "csrc", h)
           for h in ("esa_contained_core.h", "esa_spmred_core.h", "esa_spm_core.h", "esa_qmatch_core.h",
                     "esa_mstat_search.h")]
SHIM = os.path.join(ROOT, "oracle", "_build", "libcontained_core_shim.so")
SP_WALK = 64


@pytest.fixture(scope="module")
def shim():
    ou.build()
    if not os.path.exists(SHIM) or os.path.getmtime(SHIM) < max(os.path.getmtime(f) for f in [SHIM_SRC] + HEADERS):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-shared", "-fPIC", "-o", SHIM, SHIM_SRC],
                       check=True)
    lib = ctypes.CDLL(SHIM)
    P = ctypes.c_void_p
    lib.ct_shim_run.argtypes = [P, ctypes.c_uint64, P, ctypes.c_int, P, P, ctypes.c_uint64, P, P]
    lib.ct_shim_run.restype = ctypes.c_int64
    lib.ct_shim_compact.argtypes = [P, ctypes.c_uint64, P, ctypes.c_uint64, ctypes.c_uint64, P, ctypes.c_uint32, P]
    lib.ct_shim_compact.restype = ctypes.c_uint64
    lib.ct_shim_mirror.argtypes = [P, ctypes.c_uint64, P]
    lib.ct_shim_mirror.restype = None
    return lib


def _framed(a):
    """cut out of a larger array filled with wildcards, so that a read beside it finds neither a letter nor a
    separator"""
    big = np.full(a.size + 64, 254, dtype=np.uint8)
    big[32:32 + a.size] = a
    return big[32:32 + a.size]


def _run(lib, enc, t, width):
    """(verdicts, counts) for the mirrored set enc and the oracle's tables t; None for a refusal"""
    enc = _framed(np.asarray(enc, dtype=np.uint8))
    suf = np.ascontiguousarray(t["suf"].astype(width))
    lcp, llv = np.ascontiguousarray(t["lcp"]), np.ascontiguousarray(t["llv"], dtype=np.uint64).reshape(-1)
    verdict = np.full(enc.size, 99, dtype=np.uint8)
    count = np.zeros(5, dtype=np.uint64)
    R = lib.ct_shim_run(enc.ctypes.data, enc.size, suf.ctypes.data, suf.dtype.itemsize, lcp.ctypes.data,
                        llv.ctypes.data if llv.size else None, llv.size // 2, verdict.ctypes.data, count.ctypes.data)
    return None if R < 0 else (verdict[:R], count)


def _agree(lib, reads, widths=(np.uint64, np.uint32)):
    """both table widths against the brute force; its verdicts and the tables"""
    want = pr.verdicts(reads)
    enc = sr.mirrored(sr.joined(reads))
    t = ou.esa(enc, 4)
    for width in widths:
        got, count = _run(lib, enc, t, width)
        assert np.array_equal(got, want), np.flatnonzero(got != want)[:10]
        assert count.tolist() == np.bincount(want, minlength=5).tolist()
    return want, t


@pytest.mark.parametrize("seed", range(100, 140))
def test_equal_length_sets(shim, seed):
    reads = pr.seeded_reads(seed, 36)
    want, _ = _agree(shim, reads)
    fig = pr.tallies(want)
    assert fig["duplicates"] >= 9 and fig["self_complementary"] >= 1 and fig["affixes"] == fig["internal"] == 0


@pytest.mark.parametrize("seed", range(200, 240))
def test_variable_length_sets(shim, seed):
    reads = pr.seeded_reads(seed, (20, 60))
    want, _ = _agree(shim, reads)
    fig = pr.tallies(want)
    assert fig["duplicates"] >= 9 and fig["affixes"] >= 8 and fig["kept"] >= 5


def test_every_verdict_occurs_in_the_seeded_sets():
    seen = np.zeros(5, dtype=np.int64)
    for seed in range(200, 240):
        seen += np.bincount(pr.verdicts(pr.seeded_reads(seed, (20, 60))), minlength=5)
    assert (seen >= 40).all(), seen


def test_the_lower_number_is_the_mirror_copy(shim):
    rng = np.random.default_rng(7)
    a, b, c = (rng.integers(0, 4, 30, dtype=np.uint8) for _ in range(3))
    reads = [revcomp(a), b, a, c, revcomp(c), revcomp(a), a]
    want, _ = _agree(shim, reads)
    assert want.tolist() == [0, 0, 1, 0, 1, 1, 1]


@pytest.mark.parametrize("count", [65, 257])
def test_a_run_of_duplicates_wider_than_a_wave(shim, count):
    """the run of equal whole reads is wider than the walk over .lcp: every lane reads its survivor off the two ends"""
    reads = pr.copies_on_both_strands(count, count)
    want, _ = _agree(shim, reads)
    assert pr.tallies(want) == dict(kept=9, duplicates=count - 1, affixes=0, internal=0, self_complementary=0)
    # all of them on one strand, and a self-complementary read as often
    one = [reads[0]] * count
    assert _agree(shim, one)[0].tolist() == [0] + [1] * (count - 1)
    palindrome = pr.self_complementary(np.random.default_rng(3), 36)
    assert _agree(shim, [palindrome] * count)[0].tolist() == [4] + [1] * (count - 1)


def test_long_reads_consult_llv(shim):
    """reads of 256 to 300 letters, one of 260 the prefix of another: LCP bytes of 255"""
    reads, last = pr.llv_reads()
    want, t = _agree(shim, reads)
    assert t["llv"].shape[0] > 10
    assert want[-5:].tolist() == last and (want[:-5] == 0).all()
    # a neighbour shares 255 letters or more, not all 260: the byte alone does not decide
    text = np.random.default_rng(11).integers(0, 4, 3000, dtype=np.uint8)
    reads = [text[:300].copy(), np.concatenate([text[:258], 3 - text[258:260]]), text[400:700].copy()]
    assert _agree(shim, reads)[0].tolist() == [0, 0, 0]


def test_an_interval_wider_than_the_walk(shim):
    """more than SP_WALK sequences start with the read: its interval is searched for in the text"""
    reads, inner = pr.wide_interval_reads(SP_WALK + 6)
    want, _ = _agree(shim, reads)
    assert want[20] == 2 and want[41] == 1 and pr.tallies(want)["kept"] == SP_WALK + 7
    # the same reads behind 30 other letters: inside, SP_WALK + 6 times
    want, _ = _agree(shim, inner)
    assert want[-1] == 3 and (want[:-1] == 0).all()


def test_a_duplicate_that_is_a_prefix_of_a_third_read(shim):
    """both copies go, the first as an affix and the second as a duplicate: the reference keeps one"""
    for reads, verdicts in pr.blind_spot_sets():
        assert _agree(shim, reads)[0].tolist() == verdicts


@pytest.mark.parametrize("count", [255, 256, 257, 769])
def test_sized_sets(shim, count):
    want, _ = _agree(shim, pr.sized_reads(count), widths=(np.uint64,))
    fig = pr.tallies(want)
    assert fig["duplicates"] >= count // 5 and fig["self_complementary"] >= count // 50


def test_short_reads(shim):
    """reads of one letter: of any number two survive, A and C (T is the mirror image of A)"""
    rng = np.random.default_rng(19)
    reads = [rng.integers(0, 4, 1, dtype=np.uint8) for _ in range(40)]
    want, _ = _agree(shim, reads)
    assert pr.tallies(want)["kept"] == 2
    for k in (2, 3, 4):
        _agree(shim, [rng.integers(0, 4, k, dtype=np.uint8) for _ in range(40)])
    assert _agree(shim, [np.array([0, 3], dtype=np.uint8)])[0].tolist() == [4]
    assert _agree(shim, [np.array([0, 1, 2], dtype=np.uint8)])[0].tolist() == [0]


def test_an_odd_number_of_sequences_is_no_mirrored_set(shim):
    rng = np.random.default_rng(23)
    enc = sr.joined([rng.integers(0, 4, 20, dtype=np.uint8) for _ in range(3)])
    assert _run(shim, enc, ou.esa(enc, 4), np.uint64) is None


@pytest.mark.parametrize("strict", [False, True])
def test_compaction(shim, strict):
    for seed, length in ((100, 36), (200, (20, 60))):
        reads = pr.seeded_reads(seed, length)
        v = pr.verdicts(reads)
        enc = sr.joined(reads)
        want = pr.kept_symbols(reads, v, strict)
        mask = pr.STRICT_MASK if strict else pr.DEFAULT_MASK
        for text in (enc, sr.mirrored(enc)):            # the separators of the set, or of its mirrored set
            seps = np.flatnonzero(text == 255).astype(np.uint32)
            out = np.full(enc.size, 77, dtype=np.uint8)
            n = shim.ct_shim_compact(_framed(enc).ctypes.data, enc.size, seps.ctypes.data, seps.size, len(reads),
                                     v.ctypes.data, mask, out.ctypes.data)
            assert np.array_equal(out[:n], want) and (out[n:] == 77).all()
    # nothing is left; the last read is left alone; the first
    enc = sr.joined([np.zeros(5, dtype=np.uint8), np.ones(3, dtype=np.uint8), np.full(4, 2, dtype=np.uint8)])
    seps = np.flatnonzero(enc == 255).astype(np.uint32)
    out = np.zeros(enc.size, dtype=np.uint8)
    for v, want in (([1, 1, 1], []), ([1, 2, 0], [2] * 4), ([0, 1, 1], [0] * 5), ([0, 1, 0], [0] * 5 + [255] + [2] * 4)):
        v = np.array(v, dtype=np.uint8)
        n = shim.ct_shim_compact(enc.ctypes.data, enc.size, seps.ctypes.data, seps.size, 3, v.ctypes.data,
                                 pr.DEFAULT_MASK, out.ctypes.data)
        assert out[:n].tolist() == want


def test_mirror(shim):
    for enc in (sr.wildcard_reads(), np.zeros(0, dtype=np.uint8), np.array([2], dtype=np.uint8)):
        out = np.zeros(2 * enc.size + 1, dtype=np.uint8)
        shim.ct_shim_mirror(_framed(enc).ctypes.data, enc.size, out.ctypes.data)
        assert np.array_equal(out, sr.mirrored(enc))
