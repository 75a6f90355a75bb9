"""Contained reads on the device (include/gtamd_contained.h,
genometools_amd/contained.py) against the brute force of
tests/prefilter_reference.py: the verdict of every read, the counts, the reads
that are left, the mirrored set and the first filter.  The tables come from the
engine, in this process, resident or handed over as 8- and as 4-byte entries.

The shapes are the smallest at which each part can go wrong: a workgroup takes
TILE reads, sequences or symbols (contained.geometry()), a wave's verdicts of a
class are one ballot; the interval of a read is walked for 64 entries of .lcp to
either side before it is searched for; .lcp holds a byte 255 from 255 letters
on."""
import functools

import numpy as np
import pytest

import prefilter_reference as pr
import spm_reference as sr
from genometools_amd import _lib, contained, esa, spm, spmred

pytestmark = pytest.mark.gpu

TILE = contained.geometry()
SP_WALK = 64


@pytest.fixture(scope="module")
def finder(gpu):
    with contained.ContainedReads() as f:
        yield f


@functools.lru_cache(maxsize=None)
def _reads(name):
    kind, _, arg = name.partition(":")
    if kind == "equal":
        return pr.seeded_reads(int(arg), 36)
    if kind == "variable":
        return pr.seeded_reads(int(arg), (20, 60))
    if kind == "copies":
        return pr.copies_on_both_strands(int(arg), int(arg))
    if kind == "llv":
        return pr.llv_reads()[0]
    if kind == "wide":
        return pr.wide_interval_reads(SP_WALK + 6)[0]
    if kind == "inner":
        return pr.wide_interval_reads(SP_WALK + 6)[1]
    if kind == "blind":
        return pr.blind_spot_sets()[int(arg)][0]
    if kind == "sized":
        return pr.sized_reads(int(arg))
    if kind == "one":
        rng = np.random.default_rng(5)
        return [rng.integers(0, 4, 1, dtype=np.uint8) for _ in range(40)]
    raise ValueError(name)


@functools.lru_cache(maxsize=None)
def _expected(name):
    """(verdicts, unmirrored symbols) of the brute force; shared, never written to"""
    reads = _reads(name)
    out = (pr.verdicts(reads), sr.joined(reads))
    for a in out:
        a.setflags(write=False)
    return out


def _agree(finder, name, widths=(np.uint32,), strict=(False, True)):
    """the set through the resident engine and through host tables of the given widths"""
    import torch
    want, enc = _expected(name)
    both = torch.from_numpy(sr.mirrored(enc)).cuda()
    tallies = np.bincount(want, minlength=5).tolist()

    def check():
        info = finder.decide()
        assert np.array_equal(finder.verdicts(), want), np.flatnonzero(finder.verdicts() != want)[:10]
        assert info["count"] == tallies and info == finder.info()
        assert (info["reads"], info["sequences"], info["table_entries"]) == (want.size, 2 * want.size, 2 * enc.size + 2)
        assert info["device_bytes"] > 0 and info["device_ms"] >= info["lists_ms"] >= 0
        for s in strict:
            left = pr.kept_symbols(_reads(name), want, s)
            assert np.array_equal(finder.filtered(strict=s), left)
            assert np.array_equal(finder.filtered(enc, strict=s), left)

    with esa.EsaEngine(both.numel(), 4) as eng:
        eng.set_sequence_device(both.data_ptr(), both.numel())
        eng.run(esa.WANT_SUF | esa.WANT_LCP)
        finder.set_index_engine(eng, both.data_ptr(), both.numel())
        check()
        tables = (eng.table(esa.TAB_SUF), eng.table(esa.TAB_LCP), eng.table(esa.TAB_LLV))
    for width in widths:
        finder.set_index(both.cpu().numpy(), tables[0].astype(width), tables[1], tables[2])
        check()
    return want, tables


@pytest.mark.parametrize("first", range(100, 140, 10))
def test_equal_length_sets(finder, first):
    for seed in range(first, first + 10):
        _agree(finder, "equal:%d" % seed, widths=(np.uint32,) if seed % 2 else (np.uint64,), strict=(bool(seed & 2),))


@pytest.mark.parametrize("first", range(200, 240, 10))
def test_variable_length_sets(finder, first):
    for seed in range(first, first + 10):
        _agree(finder, "variable:%d" % seed, widths=(np.uint32,) if seed % 2 else (np.uint64,), strict=(bool(seed & 2),))


@pytest.mark.parametrize("count", [65, 257])
def test_a_run_of_duplicates_wider_than_a_wave(finder, count):
    want, _ = _agree(finder, "copies:%d" % count, widths=(np.uint32, np.uint64))
    assert pr.tallies(want)["duplicates"] == count - 1


def test_long_reads_consult_llv(finder):
    want, tables = _agree(finder, "llv", widths=(np.uint32, np.uint64))
    assert tables[2].size > 20 and want[-5:].tolist() == pr.llv_reads()[1]


@pytest.mark.parametrize("name", ["wide", "inner"])
def test_an_interval_wider_than_the_walk(finder, name):
    want, _ = _agree(finder, name)
    assert (name == "wide" and want[20] == pr.AFFIX) or (name == "inner" and want[-1] == pr.INTERNAL)


def test_a_duplicate_that_is_a_prefix_of_a_third_read(finder):
    for k, (_, verdicts) in enumerate(pr.blind_spot_sets()):
        assert _agree(finder, "blind:%d" % k)[0].tolist() == verdicts


@pytest.mark.parametrize("count", [TILE - 1, TILE, TILE + 1, 3 * TILE + 1])
def test_read_counts_either_side_of_a_tile(finder, count):
    assert TILE == 256                # (the sets of tests/test_contained_core.py are these)
    want, _ = _agree(finder, "sized:%d" % count)
    assert want.size == count and pr.tallies(want)["duplicates"] >= count // 5


def test_reads_of_one_letter(finder):
    want, _ = _agree(finder, "one")
    assert pr.tallies(want)["kept"] == 2


def _compacted(finder, lengths, drop):
    """reads of the given lengths, those at `drop` duplicates of read 0: what is left, and what should be"""
    import torch
    rng = np.random.default_rng(len(lengths))
    reads = [rng.integers(0, 4, k, dtype=np.uint8) for k in lengths]
    for k in drop:
        reads[k] = reads[0].copy()
    enc = sr.joined(reads)
    both = torch.from_numpy(sr.mirrored(enc)).cuda()
    with esa.EsaEngine(both.numel(), 4) as eng:
        eng.set_sequence_device(both.data_ptr(), both.numel())
        eng.run(esa.WANT_SUF | esa.WANT_LCP)
        finder.set_index_engine(eng, both.data_ptr(), both.numel())
        assert finder.decide()["duplicates"] == len(drop)
        got = finder.filtered(device=True)
    assert got.is_cuda and got.dtype == torch.uint8
    return got.cpu().numpy(), sr.joined([r for k, r in enumerate(reads) if k not in drop])


def test_compaction_across_tiles(finder):
    # 2 * TILE symbols exactly: the last workgroup is full; one fewer and one more
    for last in (32, 31, 33):
        lengths = [31] * 6 + [31] * 15 + [last]
        got, want = _compacted(finder, lengths, drop=(2, 3, 9, 11, 20, 7))
        assert want.size == 15 * 32 + last and np.array_equal(got, want)
    # a read that crosses two tile borders, a dropped read last; one read is left
    got, want = _compacted(finder, [20, 20, 600, 20, 30, 20], drop=(1, 5))
    assert np.array_equal(got, want)
    got, want = _compacted(finder, [40] * 3, drop=(1, 2))
    assert np.array_equal(got, want) and got.size == 40


def test_the_device_mirror(finder):
    import torch
    for enc in (sr.wildcard_reads(), np.array([2], dtype=np.uint8), np.zeros(0, dtype=np.uint8),
                np.random.default_rng(1).integers(0, 4, 2 * TILE, dtype=np.uint8)):
        got = finder.mirrored_device(enc)
        assert got.is_cuda and np.array_equal(got.cpu().numpy(), spm.mirrored(enc))
        assert np.array_equal(finder.mirrored_device(torch.from_numpy(enc.copy()).cuda()).cpu().numpy(), spm.mirrored(enc))


def test_the_wildcard_filter(finder):
    enc = sr.wildcard_reads()
    reads = [enc[a:a + k] for a, k in sr.units(enc)]
    clean = [r for r in reads if (r < 254).all()]
    assert 0 < len(clean) < len(reads)
    got, dropped = finder.without_wildcards(enc)
    assert np.array_equal(got, sr.joined(clean)) and dropped == len(reads) - len(clean)
    got, dropped = finder.without_wildcards(enc, separators=np.flatnonzero(enc == 255))
    assert np.array_equal(got, sr.joined(clean))
    # nothing to drop; everything; the first and the last read; a set of one read
    plain = sr.joined(clean)
    got, dropped = finder.without_wildcards(plain)
    assert np.array_equal(got, plain) and dropped == 0
    got, dropped = finder.without_wildcards(sr.joined([np.full(5, 254, dtype=np.uint8)] * 3))
    assert got.size == 0 and dropped == 3
    wild = np.array([0, 254, 1], dtype=np.uint8)
    got, dropped = finder.without_wildcards(sr.joined([wild] + clean[:TILE // 50 + 2] + [wild]))
    assert np.array_equal(got, sr.joined(clean[:TILE // 50 + 2])) and dropped == 2
    got, dropped = finder.without_wildcards(clean[0])
    assert np.array_equal(got, clean[0]) and dropped == 0
    with pytest.raises(_lib.EsaError, match="ascending positions below"):
        finder.without_wildcards(enc, separators=[5, 5])
    with pytest.raises(_lib.EsaError, match="ascending positions below"):
        finder.without_wildcards(enc, separators=[enc.size])


@pytest.mark.parametrize("seed", [200, 213])
def test_prefilter_end_to_end(gpu, seed):
    """reads in, kept symbols out; the strict result is a set `readjoiner overlap` accepts"""
    reads = pr.seeded_reads(seed, (20, 60))
    wild = reads[3].copy()
    wild[7] = 254
    want = pr.verdicts(reads)
    given = sr.joined(reads[:10] + [wild] + reads[10:])
    for strict in (False, True):
        kept, verdicts, info = contained.prefilter(given, strict=strict)
        assert np.array_equal(verdicts, want) and info["wildcard_reads"] == 1
        assert info["count"] == np.bincount(want, minlength=5).tolist()
        assert np.array_equal(kept, pr.kept_symbols(reads, want, strict))
    assert pr.tallies(want)["internal"] + pr.tallies(want)["self_complementary"] > 0
    both = spm.mirrored(kept)
    with esa.EsaEngine(both.size, 4) as eng, spmred.IrreducibleMatches() as matcher:
        eng.set_sequence(both)
        eng.run(esa.WANT_SUF | esa.WANT_LCP)
        matcher.set_index(both, eng.table(esa.TAB_SUF), eng.table(esa.TAB_LCP), eng.table(esa.TAB_LLV))
        assert matcher.prepare(1)["contained_sequences"] == 0
        # the default result is not such a set
        loose = spm.mirrored(contained.prefilter(given)[0])
    with esa.EsaEngine(loose.size, 4) as eng, spmred.IrreducibleMatches() as matcher:
        eng.set_sequence(loose)
        eng.run(esa.WANT_SUF | esa.WANT_LCP)
        matcher.set_index(loose, eng.table(esa.TAB_SUF), eng.table(esa.TAB_LCP), eng.table(esa.TAB_LLV))
        assert matcher.prepare(1)["contained_sequences"] > 0


def test_nothing_is_left_of_nothing(gpu):
    kept, verdicts, info = contained.prefilter(np.zeros(0, dtype=np.uint8))
    assert kept.size == verdicts.size == info["reads"] == 0
    kept, verdicts, info = contained.prefilter(np.array([254, 0, 1], dtype=np.uint8), strict=True)
    assert kept.size == verdicts.size == 0 and info["wildcard_reads"] == 1


def test_verdicts_on_the_device(finder):
    import torch
    want, _ = _agree(finder, "equal:100", widths=(np.uint64,))
    got = finder.verdicts(device=True)
    assert got.is_cuda and got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want)


def test_refusals(gpu):
    rng = np.random.default_rng(31)
    reads = [rng.integers(0, 4, 20, dtype=np.uint8) for _ in range(4)]

    def tables(enc):
        with esa.EsaEngine(enc.size, 4) as eng:
            eng.set_sequence(enc)
            eng.run(esa.WANT_SUF | esa.WANT_LCP)
            return enc, eng.table(esa.TAB_SUF), eng.table(esa.TAB_LCP), eng.table(esa.TAB_LLV)

    with contained.ContainedReads() as f:
        with pytest.raises(_lib.EsaError, match="no index is set"):
            f.decide()
        with pytest.raises(_lib.EsaError, match="nothing is decided"):
            f.verdicts()
        with pytest.raises(_lib.EsaError, match="nothing is decided"):
            f.filtered()
        f.set_index(*tables(sr.joined(reads[:3])))
        with pytest.raises(_lib.EsaError, match="3 sequences are no mirrored set: an even number"):
            f.decide()
        for first in (14, 15):                                  # an odd number of symbols, and an even one
            f.set_index(*tables(sr.joined([reads[0][:first]] + reads[1:])))
            with pytest.raises(_lib.EsaError, match="no mirrored set: that separator is expected in the middle"):
                f.decide()
        empty = sr.mirrored(np.concatenate([reads[0], [255, 255], reads[1]]).astype(np.uint8))
        f.set_index(*tables(empty))
        with pytest.raises(_lib.EsaError, match="2 of 6 sequences are empty or start with a wildcard"):
            f.decide()
        enc = sr.joined(reads)
        f.set_index(*tables(sr.mirrored(enc)))
        assert f.decide()["kept"] == 4
        with pytest.raises(_lib.EsaError, match="%d symbols given, the reads of the index are %d" % (enc.size - 1, enc.size)):
            f.filtered(enc[:-1])
        check = _lib.check
        out, count = _lib.ctypes.c_void_p(), _lib.ctypes.c_uint64()
        with pytest.raises(_lib.EsaError, match="mask 32 names a verdict that is none"):
            check(f._fn("compact")(f._p, 32, None, enc.size, _lib.ctypes.byref(out), _lib.ctypes.byref(count)))
        # a new index: what was decided is none
        f.set_index(*tables(sr.mirrored(enc)))
        with pytest.raises(_lib.EsaError, match="nothing is decided"):
            f.verdicts()
        with pytest.raises(_lib.EsaError, match="no .lcp table"):
            f.set_index_device(1, 10, 1, 8, None)
