"""What one lane of the irreducible suffix-prefix match kernels does
(genometools_amd/csrc/esa_spmred_core.h: the transitive test of one pair, the
mirror filter, the select in a bitmap word and the record), compiled with g++
and run on the CPU over every pair, against the brute force of
tests/spmred_reference.py: every verdict, pair by pair, every kept record in the
stated order, and the figures.  The tables are the oracle's.  For the sets with
duplicates, contained reads, a read equal to its own reverse complement, a
homopolymer, a tandem repeat or wildcards the reference is no yardstick
(include/gtamd_spmred.h) and the brute force of the definition is.  No GPU: what
is left for tests/test_spmred_gpu.py is the kernels around it, the sort, the
ballots, the scan and the C ABI."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

import oracle_util as ou
import spm_reference as sr
import spmred_reference as rr

ROOT = ou.ROOT
SHIM_SRC = os.path.join(ROOT, "tests", "spmred_core_shim.cpp")
HEADERS = [os.path.join(ROOT, "genometools_amd", "csrc", h)
           for h in ("esa_spmred_core.h", "esa_spm_core.h", "esa_qmatch_core.h", "esa_mstat_search.h")]
SHIM = os.path.join(ROOT, "oracle", "_build", "libspmred_core_shim.so")
FIGURES = ("matches", "kept", "transitive_same_read", "transitive_other", "contained_sequences", "candidates",
           "max_candidates", "letters")
ELIMTRANS, MIRRORED = 1, 2


@pytest.fixture(scope="module")
def shim():
    ou.build()
    if not os.path.exists(SHIM) or os.path.getmtime(SHIM) < max(os.path.getmtime(f) for f in [SHIM_SRC] + HEADERS):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-shared", "-fPIC", "-o", SHIM, SHIM_SRC],
                       check=True)
    lib = ctypes.CDLL(SHIM)
    P = ctypes.c_void_p
    lib.sr_shim_run.argtypes = [P, ctypes.c_uint64, P, ctypes.c_int, P, P, ctypes.c_uint64, ctypes.c_uint32,
                                ctypes.c_uint32, P, P, P]
    lib.sr_shim_run.restype = ctypes.c_uint64
    lib.sr_shim_select.argtypes = [ctypes.c_uint64, ctypes.c_uint32]
    lib.sr_shim_select.restype = ctypes.c_uint32
    return lib


def _framed(a):
    """cut out of a larger array filled with wildcards, so that a read beside it finds neither a letter nor a
    separator"""
    big = np.full(a.size + 64, 254, dtype=np.uint8)
    big[32:32 + a.size] = a
    return big[32:32 + a.size]


def _run(lib, enc, t, width, min_len, flags):
    """(verdicts pair by pair, kept records in order, figures) for the oracle's tables t"""
    enc = _framed(np.asarray(enc, dtype=np.uint8))
    suf = np.ascontiguousarray(t["suf"].astype(width))
    lcp, llv = np.ascontiguousarray(t["lcp"]), np.ascontiguousarray(t["llv"], dtype=np.uint64).reshape(-1)
    fig = np.zeros(len(FIGURES), dtype=np.uint64)
    args = (enc.ctypes.data, enc.size, suf.ctypes.data, suf.dtype.itemsize, lcp.ctypes.data,
            llv.ctypes.data if llv.size else None, llv.size // 2, min_len, flags)
    kept = lib.sr_shim_run(*args, None, None, fig.ctypes.data)
    verdict = np.zeros(int(fig[0]), dtype=np.uint8)
    out = np.zeros((kept, 4), dtype=np.int64)
    assert lib.sr_shim_run(*args, verdict.ctypes.data, out.ctypes.data, fig.ctypes.data) == kept
    return verdict.astype(bool), out, dict(zip(FIGURES, fig.tolist()))


def _agree(lib, enc, min_len, mirrored, t=None, widths=(np.uint64, np.uint32)):
    """both table widths, with and without the reduction, against the brute force; its figures"""
    enc = np.ascontiguousarray(enc, dtype=np.uint8)
    t = ou.esa(enc, 4) if t is None else t
    rows = sr.brute_force(enc, min_len)[0]
    rank = np.empty(t["suf"].size, dtype=np.int64)
    rank[t["suf"].astype(np.int64)] = np.arange(t["suf"].size)
    order = np.lexsort((rank[rows[:, 4]], rank[rows[:, 3]]))
    want_verdict = rr.transitive(enc, rows)[order]
    for elimtrans in (True, False):
        kept, figures = rr.brute_force(enc, min_len, elimtrans, mirrored)
        want = rr.in_order(kept, t["suf"])
        for width in widths:
            flags = (ELIMTRANS if elimtrans else 0) | (MIRRORED if mirrored else 0)
            verdict, got, fig = _run(lib, enc, t, width, min_len, flags)
            assert np.array_equal(verdict, want_verdict if elimtrans else np.zeros_like(want_verdict))
            assert np.array_equal(got, want)
            for name, value in figures.items():
                assert fig[name] == value, name
            if not elimtrans:
                assert fig["candidates"] == fig["letters"] == 0
    return rr.brute_force(enc, min_len, True, mirrored)[1]


@functools.lru_cache(maxsize=None)
def _golden_spm(name):
    """the read sets of tests/golden/spm: duplicates, a reverse-complemented duplicate, contained reads, a
    homopolymer, a tandem repeat, a reverse-complement palindrome"""
    enc = sr.mirrored(ou.encode_fasta(os.path.join(ou.GOLDEN_DIR, "spm", name)))
    t = ou.esa(enc, 4)
    enc.setflags(write=False)
    return enc, t


def test_select_finds_every_set_bit(shim):
    rng = np.random.default_rng(5)
    words = [1, 1 << 63, (1 << 64) - 1, 0x8000000100000001, 0xAAAAAAAAAAAAAAAA] + \
        [int(v) for v in rng.integers(0, 1 << 63, 40, dtype=np.uint64)]
    for b in words:
        places = [k for k in range(64) if b >> k & 1]
        assert [shim.sr_shim_select(b, r) for r in range(len(places))] == places


def test_mirror_filter_keeps_one_of_two_images():
    """an overlap (a, x) -> (b, y) of length l has the image (b, not y) -> (a, not x); of the two, one is kept
    -- both are one and the same for a read with its own reverse complement"""
    for sn in range(3):
        for pn in range(3):
            for sd in (True, False):
                for pd in (True, False):
                    image = (pn, not pd, sn, not sd)
                    kept = [rr.mirror_kept(sn, sd, pn, pd), rr.mirror_kept(*image)]
                    if image == (sn, sd, pn, pd):
                        assert kept[0] == kept[1]
                    else:
                        assert sum(kept) == 1, (sn, sd, pn, pd)


@pytest.mark.parametrize("seed,length,min_len", [(31, 36, 12), (31, 36, 20), (32, (25, 60), 12), (32, (25, 60), 20)])
def test_containment_free_reads_on_both_strands(shim, seed, length, min_len):
    """what the tool is made for: tiled reads with a planted repeat and its reverse complement"""
    reads = rr.tiled_reads(seed, 1100, length, 5, repeat=80)
    enc = rr.mirrored_set(reads)
    fig = _agree(shim, enc, min_len, True)
    assert fig["contained_sequences"] == 0
    assert fig["transitive_same_read"] + fig["transitive_other"] > 200 and fig["kept"] > 50
    _agree(shim, sr.joined(reads), min_len, False)


@pytest.mark.parametrize("name,min_len", [("mixed.fna", 12), ("mixed.fna", 30), ("equal.fna", 12), ("equal.fna", 20)])
def test_sets_with_contained_sequences(shim, name, min_len):
    """duplicates, contained reads, a palindrome, a homopolymer, a tandem repeat: by the definition as
    written, ties never reduce"""
    enc, t = _golden_spm(name)
    fig = _agree(shim, enc, min_len, True, t)
    assert fig["contained_sequences"] >= 14          # 6 duplicates and one reverse-complemented, on both strands
    assert fig["transitive_same_read"] > 0 and fig["transitive_other"] > 0


def test_the_three_kinds_of_containment_are_counted(shim):
    rng = np.random.default_rng(41)
    a, b, c = (rng.integers(0, 4, 40, dtype=np.uint8) for _ in range(3))
    half = rng.integers(0, 4, 15, dtype=np.uint8)
    palindrome = np.concatenate([half, rr.revcomp(half)])
    for reads, count in (([a, b, c], 0), ([a, b, a, c], 4), ([a, b, a[5:35], c], 2), ([a, palindrome, b], 2),
                         ([a, b, rr.revcomp(a), c[:30]], 4)):
        assert _agree(shim, rr.mirrored_set(reads), 12, True)["contained_sequences"] == count
    # unmirrored: a duplicate counts on its one strand, a palindrome is a read like any other
    assert _agree(shim, sr.joined([a, b, a, c]), 12, False)["contained_sequences"] == 2
    assert _agree(shim, sr.joined([a, palindrome, b]), 12, False)["contained_sequences"] == 0
    # a contained read of fewer than min_len letters is no terminal suffix of step 1
    assert _agree(shim, sr.joined([a, b, a[5:15], c]), 12, False)["contained_sequences"] == 0


def test_wildcards_at_read_ends(shim):
    enc = sr.wildcard_reads()
    for data, mirrored in ((enc, False), (sr.mirrored(enc), True)):
        for min_len in (10, 19, 30):
            fig = _agree(shim, data, min_len, mirrored)
        assert fig["matches"] > 20


def test_homopolymer_and_tandem_repeat(shim):
    """every suffix is a terminal suffix and every interval is wide: long walks, the same verdicts"""
    rng = np.random.default_rng(43)
    flank = rng.integers(0, 4, 60, dtype=np.uint8)
    reads = [np.zeros(30, dtype=np.uint8), np.zeros(35, dtype=np.uint8),
             np.concatenate([flank[:20], np.zeros(25, dtype=np.uint8)]),
             np.concatenate([np.zeros(25, dtype=np.uint8), flank[20:40]]),
             np.array([0, 1, 2] * 14, dtype=np.uint8), np.array([1, 2, 0] * 12, dtype=np.uint8),
             np.concatenate([flank[40:], np.array([0, 1, 2] * 9, dtype=np.uint8)])]
    fig = _agree(shim, sr.joined(reads), 8, False)
    assert fig["transitive_same_read"] > 10 and fig["transitive_other"] > 10
    _agree(shim, rr.mirrored_set(reads), 8, True)


def test_the_first_hit_is_not_the_longest_overlap(shim):
    """r = A B, its longest overlap goes to t1 = B' C1 with B' the end of r, which branches away from w; the
    shorter overlap to t2 proves (r, w) transitive: the walk must go on behind the longest candidate"""
    reads = rr.border_reads()
    kept, fig = rr.brute_force(sr.joined(reads), 12, True, False)
    assert [0, 3, 15, 3] not in kept[:, :4].tolist() and [0, 1, 40, 3] in kept[:, :4].tolist()
    assert fig["transitive_other"] == 1
    _agree(shim, sr.joined(reads), 12, False)


def test_the_implied_overlap_is_never_shorter_than_the_pair_s(shim):
    """(r, w, l) transitive through t: the first m = |t| - l' + l letters of t end r, m >= l >= L.  A t whose
    overlap with r is shorter than l proves nothing, however long its overlap with w"""
    reads = rr.short_implied_reads()
    kept, fig = rr.brute_force(sr.joined(reads), 12, True, False)
    assert fig["transitive_other"] == 0 and [0, 2, 15, 3] in kept[:, :4].tolist()
    assert [1, 2, 30, 3] in kept[:, :4].tolist()
    _agree(shim, sr.joined(reads), 12, False)
    # every transitive match of a larger set has its witness: m >= l
    enc = rr.mirrored_set(rr.tiled_reads(31, 1100, 36, 5, repeat=80))
    rows = sr.brute_force(enc, 12)[0]
    words = [enc.tobytes()[a:a + k] for a, k in sr.units(enc)]
    for (r, w, l, _, _), tr in zip(rows.tolist(), rr.transitive(enc, rows).tolist()):
        if tr:
            assert any(t2 == w and lp > l and len(words[t]) - lp + l >= l and
                       words[r][:len(words[r]) - l].endswith(words[t][:len(words[t]) - lp])
                       for t, t2, lp, _, _ in rows.tolist())


def test_a_fan_of_reads_worked_out(shim):
    """what tests/test_spmred_gpu.py crosses a chunk of decisions with: 70 x 70 matches of one interval, wider
    than the walk over .lcp, 10 of them transitive; the worked-out rows are the brute force's"""
    reads, rows, trans = rr.fan_reads(70, 10)
    enc = sr.joined(reads)
    found = sr.brute_force(enc, 20)[0]
    order = np.lexsort(found.T[::-1])
    assert np.array_equal(found[order], rows[np.lexsort(rows.T[::-1])])
    assert np.array_equal(rr.transitive(enc, found)[order], trans[np.lexsort(rows.T[::-1])])
    fig = _agree(shim, enc, 20, False)
    assert (fig["matches"], fig["transitive_other"], fig["kept"]) == (4920, 10, 4910)


def test_a_read_with_more_than_64_terminal_suffixes(shim):
    reads = rr.tandem_reads()
    enc = sr.joined(reads)
    rows = sr.brute_force(enc, 30)[0]
    lengths = {}
    for s, _, k, _, _ in rows.tolist():
        lengths.setdefault(s, set()).add(k)
    assert max(len(v) for v in lengths.values()) > 64
    fig = _agree(shim, enc, 30, False, widths=(np.uint64,))
    assert fig["transitive_other"] > 1000 and fig["kept"] >= len(reads) - 1


def test_long_reads_consult_llv(shim):
    """reads of 300 to 600 letters: LCP bytes of 255"""
    reads = rr.tiled_reads(59, 4000, (300, 600), 60, repeat=400)
    enc = rr.mirrored_set(reads)
    t = ou.esa(enc, 4)
    assert t["llv"].shape[0] > 100
    fig = _agree(shim, enc, 100, True, t, widths=(np.uint64,))
    assert fig["transitive_other"] > 100 and fig["kept"] > 20 and fig["contained_sequences"] == 0
