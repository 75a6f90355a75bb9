"""Suffix-prefix matches on the device (include/gtamd_spm.h,
genometools_amd/spm.py) against the brute force of tests/spm_reference.py: every
record, none sampled, in the stated order.  The tables come from the engine, in
this process, and are used as 8- and as 4-byte entries.

The shapes are the smallest at which each part can go wrong: a select pass takes
1024 table entries a workgroup, the interval pass T terminal suffixes and the
emit pass T records, an emit call takes a capacity of at least LEAST records
(spm.geometry()); .lcp holds a byte 255 from 255 letters on.  The second level
of each -- more than 65,536 terminal suffixes, more than 4096 select tiles, more
than 2^24 records in one emit call -- is in tests/test_scale_gpu.py."""
import functools
import os

import numpy as np
import pytest

import oracle_util as ou
import spm_reference as sr
from genometools_amd import _lib, esa, spm

pytestmark = pytest.mark.gpu

T, LEAST = spm.geometry()
WIDTHS = [np.uint64, np.uint32]
ODD = 7919                       # a capacity that is no multiple of anything


@pytest.fixture(scope="module")
def matcher(gpu):
    with spm.SuffixPrefixMatches() as f:
        yield f


@functools.lru_cache(maxsize=None)
def _sequence(name):
    """a named sequence set; shared, never written to"""
    kind, _, arg = name.partition(":")
    if kind == "golden":
        enc = sr.mirrored(ou.encode_fasta(os.path.join(ou.GOLDEN_DIR, "spm", arg)))
    elif kind == "terminals":
        enc = sr.counted_terminals(int(arg))
    elif kind == "wildcards":
        enc = sr.mirrored(sr.wildcard_reads())
    elif kind == "long":
        enc = sr.long_reads()
    elif kind == "copies":
        # a 40-letter read that overlaps itself by 12 letters
        read = np.random.default_rng(3).integers(0, 4, 40, dtype=np.uint8)
        read[28:] = read[:12]
        enc = sr.copies(read, int(arg))
    elif kind == "nomatch":
        # ggacgt ends with acgt, which stands inside ttacgtcc: a terminal suffix
        # without a read start in its interval
        enc = sr.joined([[2, 2, 0, 1, 2, 3], [3, 3, 0, 1, 2, 3, 1, 1], [1, 0, 1, 0, 2, 2, 3, 0]])
    elif kind == "alone":
        enc = np.array([0, 1] * 20, dtype=np.uint8)
    else:
        raise ValueError(name)
    enc = np.ascontiguousarray(enc, dtype=np.uint8).copy()
    enc.setflags(write=False)
    return enc


@functools.lru_cache(maxsize=None)
def _engine_tables(name):
    """(enc, suf, lcp, llv) of the engine; shared, never written to"""
    enc = _sequence(name)
    with esa.EsaEngine(enc.size, 4) as eng:
        eng.set_sequence(enc)
        eng.run(esa.WANT_SUF | esa.WANT_LCP)
        out = (enc, eng.table(esa.TAB_SUF), eng.table(esa.TAB_LCP), eng.table(esa.TAB_LLV))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _expected(name, min_len):
    """(records in order, terminal suffixes, read starts, most records of one suffix) of the brute force"""
    rows, terminals, starts = sr.brute_force(_sequence(name), min_len)
    want = sr.in_order(rows, _engine_tables(name)[1])
    want.setflags(write=False)
    most = int(np.unique(rows[:, 3], return_counts=True)[1].max()) if rows.size else 0
    return want, terminals, starts, most


def _set(matcher, name, width=np.uint64):
    enc, suf, lcp, llv = _engine_tables(name)
    matcher.set_index(enc, suf.astype(width), lcp, llv)


def _check_info(info, name, min_len):
    want, terminals, starts, most = _expected(name, min_len)
    assert info["table_entries"] == _sequence(name).size + 1
    assert (info["matches"], info["terminal_suffixes"], info["read_starts"]) == (want.shape[0], terminals, starts)
    assert info["max_matches_of_one_suffix"] == most
    # an interval holds its own terminal suffix and another suffix, and every read start counted
    assert (info["max_width"] >= max(2, most)) if terminals else info["max_width"] == 0
    assert info["device_bytes"] > 0 and info["device_ms"] >= 0


def _agree(matcher, name, min_len, width=np.uint64, capacity=spm.DEFAULT_CAPACITY):
    _set(matcher, name, width)
    want = _expected(name, min_len)[0]
    got = matcher.all_matches(min_len, capacity)
    assert got.dtype == np.uint64 and got.shape == want.shape
    assert np.array_equal(got.astype(np.int64), want)
    _check_info(matcher.info(), name, min_len)
    return want


@pytest.mark.parametrize("width", WIDTHS)
def test_a_golden_read_set_on_both_strands(matcher, width):
    """about 500 sequences and 20,000 symbols: 20 workgroups of the select pass"""
    enc = _sequence("golden:mixed.fna")
    assert 480 <= len(sr.units(enc)) <= 520 and 18000 <= enc.size <= 24000
    assert _agree(matcher, "golden:mixed.fna", 12, width).shape[0] == 2434
    assert _agree(matcher, "golden:mixed.fna", 30, width, LEAST).shape[0] == 868
    assert _agree(matcher, "golden:mixed.fna", 61, width).shape[0] == 0


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("count", [T - 1, T, T + 1, 2 * T + 3])
def test_terminal_suffixes_around_the_tile_size(matcher, count, width):
    name = "terminals:%d" % count
    want = _agree(matcher, name, 30, width)
    assert matcher.info()["terminal_suffixes"] == count and want.shape[0] == 4 * (count // 2) + count % 2


def test_sets_without_a_match(matcher):
    """no terminal suffix at all; terminal suffixes whose intervals hold no read start"""
    for width in WIDTHS:
        assert _agree(matcher, "golden:equal.fna", 37, width).shape[0] == 0
        assert matcher.info()["terminal_suffixes"] == 0 and list(matcher.matches()) == []
        assert _agree(matcher, "nomatch", 4, width).shape[0] == 0
        assert matcher.info()["terminal_suffixes"] == 1 and matcher.info()["max_width"] == 2


@pytest.mark.parametrize("width", WIDTHS)
def test_one_read_alone(matcher, width):
    """(ac)^20 overlaps itself at every even length; its whole length stands nowhere else"""
    want = _agree(matcher, "alone", 10, width)
    assert sorted(want[:, 2].tolist()) == list(range(10, 40, 2)) and not want[:, :2].any()


@pytest.mark.parametrize("width", WIDTHS)
def test_many_copies_of_one_read(matcher, width):
    """300 copies of a 40-letter read: the interval of its 40 letters holds 300 read
    starts and 300 terminal suffixes, 300 x 300 records, and as many again for the
    12 letters the read shares with itself; every suffix of 10 letters or more is
    terminal, since every copy holds it.  Every border between two emit calls of
    LEAST records falls inside the records of one suffix"""
    name = "copies:300"
    _set(matcher, name, width)
    want = _expected(name, 10)[0]
    assert want.shape[0] == 2 * 300 * 300 and 300 % LEAST != 0
    info = matcher.prepare(10)
    _check_info(info, name, 10)
    assert info["max_matches_of_one_suffix"] == 300 and info["terminal_suffixes"] == 300 * 31
    single = np.concatenate(list(matcher.matches()))
    assert np.array_equal(single.astype(np.int64), want)
    if width is np.uint64:
        for capacity in (LEAST, ODD):
            chunks = list(matcher.matches(capacity))
            assert [c.shape[0] for c in chunks[:-1]] == [capacity] * (len(chunks) - 1) and len(chunks) > 20
            assert np.concatenate(chunks).tobytes() == single.tobytes()


@pytest.mark.parametrize("count", [63, 64, 65, 66])
def test_copies_around_the_walk_limit(matcher, count):
    """the interval of the read holds `count` terminal suffixes: a lane finds its ends by a walk of up to 64
    entries over .lcp to either side, and by a search in the text beyond that"""
    for width in WIDTHS:
        assert _agree(matcher, "copies:%d" % count, 10, width).shape[0] == 2 * count * count


@pytest.mark.parametrize("min_len", [20, 255, 256, 400, 401, 600, 601])
def test_long_reads(matcher, min_len):
    """the .llv look-up behind an LCP byte of 255"""
    _, _, lcp, llv = _engine_tables("long")
    assert llv.shape[0] > 100 and (lcp == 255).sum() == llv.shape[0]
    for width in WIDTHS:
        want = _agree(matcher, "long", min_len, width)
    assert sorted(set(want[:, 2].tolist())) == [k for k in (200, 280, 300, 400, 600) if k >= min_len]


@pytest.mark.parametrize("width", WIDTHS)
def test_wildcards(matcher, width):
    for min_len in (1, 10, 30):
        want = _agree(matcher, "wildcards", min_len, width)
    assert want.shape[0] > 20


def test_pieces_of_any_capacity_give_the_single_call(matcher):
    name = "golden:equal.fna"
    _set(matcher, name)
    want = _expected(name, 12)[0]
    assert want.shape[0] == 2180
    matcher.prepare(12)
    for capacity in (LEAST, LEAST + 1, 999, ODD):
        chunks = list(matcher.matches(capacity))
        assert [c.shape[0] for c in chunks] == [capacity] * (2180 // capacity) + [2180 % capacity]
        assert np.array_equal(np.concatenate(chunks).astype(np.int64), want)


def _device_copy(a, skew):
    import torch
    t = torch.empty(a.nbytes + 64, dtype=torch.uint8, device="cuda:0")
    t[skew:skew + a.nbytes] = torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to("cuda:0")
    torch.cuda.synchronize()
    return t, t.data_ptr() + skew


@pytest.mark.parametrize("width", WIDTHS)
def test_index_and_records_in_device_memory(matcher, width):
    """every alignment of the sequence's first symbol; the records left on the
    device and copied are those given to the host"""
    import torch
    name, min_len = "golden:mixed.fna", 20
    enc, suf, lcp, llv = _engine_tables(name)
    want = _expected(name, min_len)[0]
    assert want.shape[0] == 1724
    for skew in (0, 1, 2, 3):
        keep = [_device_copy(enc, skew), _device_copy(suf.astype(width), 8), _device_copy(lcp, (skew + 1) % 4),
                _device_copy(llv, 16)]
        matcher.set_index_device(keep[0][1], enc.size, keep[1][1], np.dtype(width).itemsize, keep[2][1],
                                 keep[3][1] if llv.size else None, llv.shape[0])
        matcher.prepare(min_len)
        chunks = [c.cpu().numpy().copy() for c in matcher.matches(LEAST, device=True)]
        torch.cuda.synchronize()
        assert len(chunks) == -(-1724 // LEAST) and np.array_equal(np.concatenate(chunks), want)
        assert np.array_equal(np.concatenate(list(matcher.matches(ODD))).astype(np.int64), want)


def test_index_from_a_live_engine(matcher):
    name, min_len = "long", 256
    enc = _sequence(name)
    want = _expected(name, min_len)[0]
    with esa.EsaEngine(enc.size, 4) as eng:
        eng.set_sequence(enc)
        eng.run(esa.WANT_SUF | esa.WANT_LCP)
        dev = _device_copy(enc, 0)
        matcher.set_index_engine(eng, dev[1], enc.size)
        got = matcher.all_matches(min_len)
        assert np.array_equal(got.astype(np.int64), want) and got.shape[0] > 8
        _check_info(matcher.info(), name, min_len)
        with pytest.raises(_lib.EsaError, match="not the whole table"):
            matcher.set_index_engine(eng, dev[1], enc.size - 1)
        assert matcher.all_matches(min_len).tobytes() == got.tobytes()     # (the index before is kept)
        eng.run(esa.WANT_SUF)
        with pytest.raises(_lib.EsaError, match="did not produce"):
            matcher.set_index_engine(eng, dev[1], enc.size)


def test_two_prepares_on_one_object(matcher):
    _set(matcher, "golden:mixed.fna")
    first = matcher.all_matches(12)
    matcher.prepare(12)
    info = matcher.prepare(30)                    # (replaces what the first has prepared)
    assert info["matches"] == 868
    assert np.array_equal(np.concatenate(list(matcher.matches())).astype(np.int64), _expected("golden:mixed.fna", 30)[0])
    assert matcher.all_matches(12).tobytes() == first.tobytes()


def test_refusals(gpu):
    enc, suf, lcp, llv = _engine_tables("golden:equal.fna")
    want = _expected("golden:equal.fna", 20)[0]
    with spm.SuffixPrefixMatches() as f:
        with pytest.raises(_lib.EsaError, match="no index is set"):
            f.prepare(20)
        with pytest.raises(_lib.EsaError, match="nothing is prepared"):
            list(f.matches())
        # arguments only: nothing lies at these addresses
        with pytest.raises(_lib.EsaError, match="entries of 3 bytes, 4 or 8 expected"):
            f.set_index_device(1 << 20, 100, 1 << 21, 3, 1 << 22)
        with pytest.raises(_lib.EsaError, match="no .lcp table is given"):
            f.set_index_device(1 << 20, 100, 1 << 21, 8, None)
        with pytest.raises(_lib.EsaError, match="beyond the limit of a single build"):
            f.set_index_device(1 << 20, (1 << 32) - 4096, 1 << 21, 8, 1 << 22)
        with pytest.raises(_lib.EsaError, match="no index is set"):      # a refused index is none
            f.prepare(20)
        f.set_index(enc, suf, lcp, llv)
        with pytest.raises(_lib.EsaError, match="minimum length of 0"):
            f.prepare(0)
        with pytest.raises(_lib.EsaError, match="nothing is prepared"):
            list(f.matches())
        assert np.array_equal(f.all_matches(20).astype(np.int64), want)
        with pytest.raises(_lib.EsaError, match="at least %d" % LEAST):
            list(f.matches(LEAST - 1))
        with pytest.raises(_lib.EsaError, match="at least %d" % LEAST):
            list(f.matches(0))
        assert np.array_equal(np.concatenate(list(f.matches(LEAST))).astype(np.int64), want)
