"""Irreducible suffix-prefix matches on the device (include/gtamd_spmred.h,
genometools_amd/spmred.py) against the brute force of tests/spmred_reference.py:
every kept record, none sampled, in the stated order, and the figures; and
against the outputs of `gt readjoiner overlap` recorded in
tests/golden/golden_rdjoverlap.json as sorted lines.  The tables come from the
engine, in this process, and are used as 8- and as 4-byte entries.

The shapes are the smallest at which each part can go wrong: a launch of the
decision takes CHUNK pairs (spmred.geometry()), a wave's 64 verdicts are one word
of the bitmap, an emit call takes a capacity of at least LEAST records; step 3
walks 64 entries of .lcp to either side before it searches; .lcp holds a byte 255
from 255 letters on."""
import functools
import hashlib
import json
import os

import numpy as np
import pytest

import oracle_util as ou
import spm_reference as sr
import spmred_reference as rr
from genometools_amd import _lib, esa, spm, spmred

pytestmark = pytest.mark.gpu

CHUNK, LEAST = spmred.geometry()
WIDTHS = [np.uint64, np.uint32]
ODD = 7919                       # a capacity that is no multiple of anything

with open(os.path.join(ou.GOLDEN_DIR, "golden_rdjoverlap.json")) as _f:
    GOLDEN = json.load(_f)


@pytest.fixture(scope="module")
def matcher(gpu):
    with spmred.IrreducibleMatches() as f:
        yield f


def _reads(name):
    kind, _, arg = name.partition(":")
    if kind == "golden":
        return ou.encode_fasta(os.path.join(ou.GOLDEN_DIR, "rdj", arg))
    if kind == "spm":                # duplicates, contained reads, a palindrome, a homopolymer, a tandem repeat
        return ou.encode_fasta(os.path.join(ou.GOLDEN_DIR, "spm", arg))
    if kind == "fan":
        return sr.joined(rr.fan_reads(*map(int, arg.split(",")))[0])
    if kind == "tandem":
        return sr.joined(rr.tandem_reads())
    if kind == "border":
        return sr.joined(rr.border_reads())
    if kind == "implied":
        return sr.joined(rr.short_implied_reads())
    if kind == "wildcards":
        return sr.wildcard_reads()
    if kind == "nomatch":
        return np.random.default_rng(3).integers(0, 4, 300, dtype=np.uint8)
    if kind == "backward":
        # four sequences of which only the last two overlap: read as a mirrored set, a
        # match of two reverse strands, whose image -- between the first two -- is not there
        text = np.random.default_rng(7).integers(0, 4, 200, dtype=np.uint8)
        return sr.joined([text[0:40], text[50:90], text[100:140], text[120:160]])
    raise ValueError(name)


@functools.lru_cache(maxsize=None)
def _sequence(name, mirrored):
    """a named sequence set, the reads alone or on both strands; shared, never written to"""
    enc = _reads(name)
    enc = np.ascontiguousarray(sr.mirrored(enc) if mirrored else enc, dtype=np.uint8).copy()
    enc.setflags(write=False)
    return enc


@functools.lru_cache(maxsize=None)
def _engine_tables(name, mirrored):
    """(enc, suf, lcp, llv) of the engine; shared, never written to"""
    enc = _sequence(name, mirrored)
    with esa.EsaEngine(enc.size, 4) as eng:
        eng.set_sequence(enc)
        eng.run(esa.WANT_SUF | esa.WANT_LCP)
        out = (enc, eng.table(esa.TAB_SUF), eng.table(esa.TAB_LCP), eng.table(esa.TAB_LLV))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _all_matches(name, mirrored, min_len):
    """(rows, transitive) of the brute force: all matches, and which of them are transitive"""
    enc = _sequence(name, mirrored)
    if name.startswith("fan:") and not mirrored and min_len == 20:
        _, rows, trans = rr.fan_reads(*map(int, name[4:].split(",")))       # worked out: tests/test_spmred_core.py
    else:
        rows = sr.brute_force(enc, min_len)[0]
        trans = rr.transitive(enc, rows)
    return rows, trans


@functools.lru_cache(maxsize=None)
def _expected(name, mirrored, min_len, elimtrans=True, filtered=None):
    """(kept records in order, figures) of the brute force; filtered: whether the records are those of a
    mirrored set (as `mirrored` unless given)"""
    rows, trans = _all_matches(name, mirrored, min_len)
    kept, figures = rr.brute_force(_sequence(name, mirrored), min_len, elimtrans,
                                   mirrored if filtered is None else filtered, rows=rows, trans=trans)
    want = rr.in_order(kept, _engine_tables(name, mirrored)[1])
    want.setflags(write=False)
    return want, figures


def _set(matcher, name, mirrored, width=np.uint64):
    enc, suf, lcp, llv = _engine_tables(name, mirrored)
    matcher.set_index(enc, suf.astype(width), lcp, llv)


def _check_info(info, figures, elimtrans=True):
    for key, value in figures.items():
        assert info[key] == value, key
    assert info["device_bytes"] > 0 and info["device_ms"] >= info["spm_ms"] >= 0 and info["decide_ms"] >= 0
    if not elimtrans or figures["matches"] == 0:
        assert info["candidates_examined"] == info["letters_compared"] == info["max_candidates_of_one_pair"] == 0
    else:
        # every pair looks at the read starts of its own interval at least, itself among them
        assert info["candidates_examined"] >= figures["matches"] - figures["transitive_other"] - \
            figures["transitive_same_read"]
        assert 1 <= info["max_candidates_of_one_pair"] <= info["candidates_examined"]


def _agree(matcher, name, mirrored, min_len, width=np.uint64, elimtrans=True, capacity=spmred.DEFAULT_CAPACITY):
    _set(matcher, name, mirrored, width)
    want, figures = _expected(name, mirrored, min_len, elimtrans)
    got = matcher.all_matches(min_len, elimtrans, mirrored, capacity)
    assert got.dtype == np.uint64 and got.shape == want.shape
    assert np.array_equal(got.astype(np.int64), want)
    _check_info(matcher.info(), figures, elimtrans)
    return want, figures


# ---- the reference's outputs ----

@pytest.mark.parametrize("key", sorted(GOLDEN["calls"]))
def test_golden_read_sets_as_sorted_lines(matcher, key):
    """the lines and the closing figures of `gt readjoiner overlap`, every call recorded"""
    assert len(GOLDEN["calls"]) == 12
    name, min_len, elim = key.split("|")
    want = GOLDEN["calls"][key]
    _set(matcher, "golden:" + name, True)
    got = matcher.all_matches(int(min_len), elim == "yes", True)
    text = rr.sorted_text(got.astype(np.int64))
    assert (hashlib.md5(text).hexdigest(), got.shape[0]) == (want["md5"], want["lines"])
    info = matcher.info()
    assert info["contained_sequences"] == 0
    assert rr.opening_lines(want["reads"]) + rr.closing_lines(info, want["reads"], elim == "yes") == want["hash_lines"]
    kept, transitive, per_read = spmred.closing_figures(info, want["reads"])
    assert "= %d" % kept in want["hash_lines"][2] and want["hash_lines"][3].endswith("= " + per_read)
    assert elim == "no" or want["hash_lines"][4].endswith("= %d" % transitive)


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("name,min_len", [("equal.fna", 12), ("equal.fna", 20), ("mixed.fna", 12), ("long.fna", 260)])
def test_golden_read_sets_in_order(matcher, name, min_len, width):
    want, figures = _agree(matcher, "golden:" + name, True, min_len, width)
    assert figures["contained_sequences"] == 0 and figures["kept"] >= 50 and figures["transitive_other"] >= 100
    if name == "long.fna":
        llv = _engine_tables("golden:" + name, True)[3]
        assert llv.shape[0] > 100 and want[:, 2].max() > 255


# ---- the kernels' borders ----

def test_pairs_beyond_one_chunk_of_decisions(matcher):
    """count x count pairs of one interval, count the smallest whose square passes a chunk: two launches of
    the decision, the last word of the bitmap partial; 100 of the pairs transitive"""
    count = int(np.ceil(np.sqrt(CHUNK))) + 1
    name = "fan:%d,100" % count
    want, figures = _agree(matcher, name, False, 20)
    Z = count * count + 200
    assert figures["matches"] == Z > CHUNK and Z % 64 != 0 and (Z - CHUNK) < CHUNK
    assert (figures["transitive_other"], figures["kept"]) == (100, Z - 100)
    info = matcher.info()
    assert info["max_matches_of_one_suffix"] == count and info["max_candidates_of_one_pair"] >= count
    # pieces whose borders fall inside words of the bitmap and beside the chunk's end
    for cursor in (CHUNK - 150, Z - 100 - 65):
        got = next(matcher.matches(LEAST, cursor=cursor))
        assert np.array_equal(got.astype(np.int64), want[cursor:cursor + LEAST])


@pytest.mark.parametrize("width", WIDTHS)
def test_an_interval_wider_than_the_walk_over_lcp(matcher, width):
    """70 x 70 pairs of one interval of 140 suffixes: step 3 searches the text for it"""
    want, figures = _agree(matcher, "fan:70,10", False, 20, width)
    assert (figures["matches"], figures["transitive_other"], figures["kept"]) == (4920, 10, 4910)
    assert matcher.info()["max_width"] >= 140 > 2 * 64 and matcher.info()["search_symbols"] > 0


@pytest.mark.parametrize("width", WIDTHS)
def test_a_read_with_more_terminal_suffixes_than_a_wave_is_wide(matcher, width):
    """a read inside a tandem repeat: 91 terminal suffixes of its own, every one with a wide interval"""
    want, figures = _agree(matcher, "tandem", False, 30, width)
    assert figures["transitive_other"] > 1000
    # (the walk of a pair counts read starts, not the terminal suffixes it passes: the 91 are the input's)
    lengths = {}
    for s, _, k, _, _ in _all_matches("tandem", False, 30)[0].tolist():
        lengths.setdefault(s, set()).add(k)
    assert max(len(v) for v in lengths.values()) > 64 and matcher.info()["letters_compared"] > 0


def test_the_first_hit_is_not_the_longest_overlap(matcher):
    for width in WIDTHS:
        want, figures = _agree(matcher, "border", False, 12, width)
        assert figures["transitive_other"] == 1 and [0, 3, 15, 3] not in want.tolist() and [0, 1, 40, 3] in want.tolist()


def test_a_longer_match_with_another_left_part_proves_nothing(matcher):
    """the implied overlap from r to t is never shorter than the pair's (include/gtamd_spmred.h): a t that
    matches w longer but does not start inside r leaves (r, w) irreducible"""
    for width in WIDTHS:
        want, figures = _agree(matcher, "implied", False, 12, width)
        assert figures["transitive_other"] == 0 and [0, 2, 15, 3] in want.tolist() and [1, 2, 30, 3] in want.tolist()


@pytest.mark.parametrize("name,min_len", [("golden:equal.fna", 12), ("spm:mixed.fna", 12), ("wildcards", 10)])
def test_without_reduction_all_matches_filtered(matcher, name, min_len):
    """ELIMTRANS off: the records of spm.SuffixPrefixMatches, filtered and renumbered, in their order"""
    _set(matcher, name, True)
    got = matcher.all_matches(min_len, elimtrans=False, mirrored=True)
    enc, suf, lcp, llv = _engine_tables(name, True)
    with spm.SuffixPrefixMatches() as every:
        every.set_index(enc, suf, lcp, llv)
        records = every.all_matches(min_len).astype(np.int64)
    K = len(sr.units(enc))
    want = []
    for s, t, k in records.tolist():
        (sn, sd), (pn, pd) = rr.read_of(s, K), rr.read_of(t, K)
        if rr.mirror_kept(sn, sd, pn, pd):
            want.append([sn, pn, k, (2 if sd else 0) | (1 if pd else 0)])
    assert len(want) > 50 and np.array_equal(got.astype(np.int64), np.array(want))
    info = matcher.info()
    assert (info["matches"], info["kept"]) == (records.shape[0], len(want))
    assert info["transitive_same_read"] == info["transitive_other"] == info["candidates_examined"] == 0
    _check_info(info, _expected(name, True, min_len, False)[1], False)


@pytest.mark.parametrize("width", WIDTHS)
def test_reads_on_one_strand(matcher, width):
    """MIRRORED off on an unmirrored set: sequence numbers, both directions set, no filter -- also on a set
    with an odd number of sequences"""
    want, figures = _agree(matcher, "golden:equal.fna", False, 12, width)
    assert len(sr.units(_sequence("golden:equal.fna", False))) % 2 == 1
    assert figures["kept"] > 50 and (want[:, 3] == 3).all()
    _agree(matcher, "golden:mixed.fna", False, 20, width, elimtrans=False)


@pytest.mark.parametrize("name,min_len", [("spm:mixed.fna", 12), ("spm:equal.fna", 20), ("wildcards", 10)])
def test_sets_outside_the_reference_s_contract(matcher, name, min_len):
    """duplicates, contained reads, a palindrome, a homopolymer, a tandem repeat, wildcards: the definition as
    written"""
    for width in WIDTHS:
        want, figures = _agree(matcher, name, True, min_len, width)
    assert figures["transitive_same_read"] + figures["transitive_other"] > 0
    assert (figures["contained_sequences"] > 0) == name.startswith("spm:")


def test_the_three_kinds_of_containment_are_counted(matcher):
    rng = np.random.default_rng(41)
    a, b, c = (rng.integers(0, 4, 40, dtype=np.uint8) for _ in range(3))
    half = rng.integers(0, 4, 15, dtype=np.uint8)
    palindrome = np.concatenate([half, rr.revcomp(half)])
    for reads, count in (([a, b, c], 0), ([a, b, a, c], 4), ([a, b, a[5:35], c], 2), ([a, palindrome, b], 2)):
        enc = rr.mirrored_set(reads)
        t = ou.esa(enc, 4)
        matcher.set_index(enc, t["suf"], t["lcp"], t["llv"])
        info = matcher.prepare(12)
        assert info["contained_sequences"] == count == rr.brute_force(enc, 12)[1]["contained_sequences"]


# ---- the index, the pieces, the refusals ----

def _device_copy(a, skew):
    import torch
    t = torch.empty(a.nbytes + 64, dtype=torch.uint8, device="cuda:0")
    t[skew:skew + a.nbytes] = torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to("cuda:0")
    torch.cuda.synchronize()
    return t, t.data_ptr() + skew


@pytest.mark.parametrize("width", WIDTHS)
def test_index_and_records_in_device_memory(matcher, width):
    import torch
    name, min_len = "golden:mixed.fna", 12
    enc, suf, lcp, llv = _engine_tables(name, True)
    want = _expected(name, True, min_len)[0]
    keep = [_device_copy(enc, 1), _device_copy(suf.astype(width), 8), _device_copy(lcp, 3), _device_copy(llv, 16)]
    matcher.set_index_device(keep[0][1], enc.size, keep[1][1], np.dtype(width).itemsize, keep[2][1],
                             keep[3][1] if llv.size else None, llv.shape[0])
    matcher.prepare(min_len)
    chunks = [c.cpu().numpy().copy() for c in matcher.matches(LEAST, device=True)]
    torch.cuda.synchronize()
    assert len(chunks) == -(-want.shape[0] // LEAST) and np.array_equal(np.concatenate(chunks), want)


def test_index_from_a_live_engine(matcher):
    name, min_len = "golden:long.fna", 260
    enc = _sequence(name, True)
    want, figures = _expected(name, True, min_len)
    with esa.EsaEngine(enc.size, 4) as eng:
        eng.set_sequence(enc)
        eng.run(esa.WANT_SUF | esa.WANT_LCP)
        dev = _device_copy(enc, 0)
        matcher.set_index_engine(eng, dev[1], enc.size)
        got = matcher.all_matches(min_len)
        assert np.array_equal(got.astype(np.int64), want) and got.shape[0] > 8
        _check_info(matcher.info(), figures)
        with pytest.raises(_lib.EsaError, match="not the whole table"):
            matcher.set_index_engine(eng, dev[1], enc.size - 1)
        assert matcher.all_matches(min_len).tobytes() == got.tobytes()     # (the index before is kept)


def test_pieces_of_any_capacity_and_cursors_anywhere(matcher):
    name = "golden:equal.fna"
    _set(matcher, name, True)
    want = _expected(name, True, 12, False)[0]
    kept = want.shape[0]
    assert kept == 933 and kept % 64 != 0
    assert matcher.prepare(12, elimtrans=False)["kept"] == kept
    for capacity in (LEAST, LEAST + 1, ODD):
        chunks = list(matcher.matches(capacity))
        assert [c.shape[0] for c in chunks] == [capacity] * (kept // capacity) + [kept % capacity][:kept % capacity > 0]
        assert np.array_equal(np.concatenate(chunks).astype(np.int64), want)
    # a cursor in the middle, inside a word of the bitmap, at the last record, at the end
    for cursor in (400, 64 * 5 + 17, 1, kept - 1):
        got = np.concatenate(list(matcher.matches(LEAST, cursor=cursor)))
        assert np.array_equal(got.astype(np.int64), want[cursor:])
    assert list(matcher.matches(LEAST, cursor=kept)) == []
    with pytest.raises(_lib.EsaError, match=r"cursor %d is not one of this enumeration \(%d kept matches\)"
                       % (kept + 1, kept)):
        list(matcher.matches(LEAST, cursor=kept + 1))
    # the cursor counts kept records, not pairs: with the reduction the same place is another record
    reduced = _expected(name, True, 12)[0]
    assert matcher.prepare(12)["kept"] == reduced.shape[0] == 190
    assert np.array_equal(next(matcher.matches(LEAST, cursor=100)).astype(np.int64), reduced[100:])
    with pytest.raises(_lib.EsaError, match="cursor 191 is not one"):
        list(matcher.matches(LEAST, cursor=191))


def test_no_pair_and_no_kept_record(matcher):
    for width in WIDTHS:
        want, figures = _agree(matcher, "nomatch", False, 12, width)          # Z = 0
        assert want.shape[0] == 0 and figures["matches"] == 0 and list(matcher.matches()) == []
    # Z = 1, kept = 0: the only match joins two sequences of the second half of the set
    _set(matcher, "backward", False)
    assert matcher.all_matches(12, mirrored=False).astype(np.int64).tolist() == [[2, 3, 20, 3]]
    info = matcher.prepare(12, mirrored=True)
    assert (info["matches"], info["kept"]) == (1, 0) and list(matcher.matches()) == []


def test_two_prepares_on_one_object(matcher):
    _set(matcher, "golden:mixed.fna", True)
    first = matcher.all_matches(12)
    assert matcher.prepare(20, elimtrans=False)["kept"] == 255
    assert matcher.all_matches(12).tobytes() == first.tobytes() and first.shape[0] == 94


def test_refusals(gpu):
    enc, suf, lcp, llv = _engine_tables("golden:equal.fna", False)
    with spmred.IrreducibleMatches() as f:
        with pytest.raises(_lib.EsaError, match="no index is set"):
            f.prepare(20)
        with pytest.raises(_lib.EsaError, match="nothing is prepared"):
            list(f.matches())
        with pytest.raises(_lib.EsaError, match="entries of 3 bytes, 4 or 8 expected"):
            f.set_index_device(1 << 20, 100, 1 << 21, 3, 1 << 22)
        with pytest.raises(_lib.EsaError, match="no .lcp table is given"):
            f.set_index_device(1 << 20, 100, 1 << 21, 8, None)
        f.set_index(enc, suf, lcp, llv)
        with pytest.raises(_lib.EsaError, match="minimum length of 0"):
            f.prepare(0)
        with pytest.raises(_lib.EsaError, match="189 sequences are no mirrored set"):
            f.prepare(12, mirrored=True)
        with pytest.raises(_lib.EsaError, match="nothing is prepared"):
            list(f.matches())
        with pytest.raises(_lib.EsaError, match="flags 4,"):
            f._call_info("prepare", 12, 4)
        assert f.prepare(12, mirrored=False)["kept"] > 0
        with pytest.raises(_lib.EsaError, match="at least %d" % LEAST):
            list(f.matches(LEAST - 1))
