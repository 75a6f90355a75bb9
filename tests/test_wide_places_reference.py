"""tests/wide_places_reference.py, the windowed reference of
tests/test_wide_places_gpu.py, held to the references that expand every record:
on inputs of a few hundred symbols with separators and wildcards its counts sum
to the full reference's record count, and its windows of odd sizes, one behind
the other, are the full reference's records in order -- for the query matches,
the suffix-prefix matches, the tag matches and the maximal pairs.  Every input
has items without a record at the start, in the middle and at the end of the
enumeration, which is asserted.  No device."""
import numpy as np
import pytest

import maxpairs_reference as mp
import oracle_util as ou
import qmatch_reference as qr
import spm_reference as sr
import tagmatch_reference as tr
import wide_places_reference as wide

WINDOWS = (1, 7, 64, 257)          # records or candidates of one window


def _windows(total, size):
    return [(a, min(a + size, total)) for a in range(0, total, size)]


def _has_empty_items_everywhere(counts):
    """an item without a record first, last and between two that have one"""
    some = np.flatnonzero(counts)
    return counts[0] == 0 and counts[-1] == 0 and some.size >= 2 and (counts[some[0]:some[-1]] == 0).any()


def test_places_of_a_window():
    off = wide.offsets_of([0, 3, 0, 0, 2, 1, 0])
    item, k = wide.places(off, 0, 6)
    assert item.tolist() == [1, 1, 1, 4, 4, 5] and k.tolist() == [0, 1, 2, 0, 1, 0]
    item, k = wide.places(off, 2, 4)
    assert item.tolist() == [1, 4] and k.tolist() == [2, 0]
    assert wide.places(off, 3, 3)[0].size == 0 and wide.places(off, 6, 9)[0].size == 0
    item, k = wide.places(off, 5, 100)
    assert item.tolist() == [5] and k.tolist() == [0]


def _subject():
    """420 symbols: random letters over a copy of 60, a separator, a wildcard"""
    enc = np.random.default_rng(5).integers(0, 4, 420, dtype=np.uint8)
    enc[300:360] = enc[20:80]
    enc[150] = 255
    enc[222] = 254
    return enc


def _query(enc):
    """slices of the subject with a wildcard and a separator in front, between
    and behind them: positions without a candidate in all three places"""
    return np.concatenate([[254, 255], enc[30:70], [255], enc[310:350], [254], enc[100:130], [255, 254, 254]]).astype(np.uint8)


@pytest.mark.parametrize("L", [3, 6])
def test_query_matches(L):
    enc = _subject()
    query = _query(enc)
    suf = ou.esa(enc, 4)["suf"]
    want = qr.expected(enc, suf, query, L)
    ref = wide.QueryMatches(enc, suf, query, L)
    assert _has_empty_items_everywhere(ref.counts) and ref.counts.size == query.size
    assert ref.total >= want.shape[0] > 20
    kept, rec = ref.candidates(0, ref.total)
    assert kept.size == ref.total == ref.counts.sum() and np.array_equal(rec, want)
    for size in WINDOWS:
        parts = [ref.candidates(a, b) for a, b in _windows(ref.total, size)]
        assert np.array_equal(np.concatenate([k for k, _ in parts]), kept)
        assert np.array_equal(np.concatenate([r for _, r in parts]), want)
    # the emit calls of the device: chunks of candidates until the room is used up
    for capacity, least in ((8, 4), (37, 4), (64, 64)):
        got, cursor, calls = [], 0, 0
        while cursor < ref.total:
            rec, after = ref.emit_call(cursor, capacity, least)
            assert after > cursor and rec.shape[0] <= capacity
            got.append(rec)
            cursor, calls = after, calls + 1
        assert cursor == ref.total and (calls > 1 or capacity > 8) and np.array_equal(np.concatenate(got), want)


def _short_reads():
    """27 reads of 30 letters, each overlapping the next by 20 (one key holds 32
    letters), with wildcards inside reads and at their ends, a read of wildcards
    only and a duplicate of a read"""
    text = np.random.default_rng(17).integers(0, 4, 300, dtype=np.uint8)
    reads = [text[k:k + 30].copy() for k in range(0, 270, 10)]
    reads[3][12] = 254
    reads[5][0] = 254
    reads[8][29] = 254
    reads[11][[0, 29]] = 254
    reads[14][:] = 254
    reads.append(reads[20].copy())
    return sr.joined(reads)


@pytest.mark.parametrize("L", [4, 10])
def test_suffix_prefix_matches(L):
    enc = _short_reads() if L == 10 else sr.copies(np.array([0, 1, 0, 1, 0, 1, 0], dtype=np.uint8), 5)
    if L == 4:
        enc = np.concatenate([enc, [255, 254, 1, 2, 3, 0, 255], [2, 2, 3, 1, 0, 1]]).astype(np.uint8)
    suf = ou.esa(enc, 4)["suf"]
    rows, terminals, starts = sr.brute_force(enc, L)
    want = sr.in_order(rows, suf)
    ref = wide.SuffixPrefixMatches(enc, suf, L)
    assert (ref.counts.size, ref.read_starts.size) == (terminals, starts)
    assert ref.total == ref.counts.sum() == want.shape[0] > 20
    assert ref.most == np.unique(rows[:, 3], return_counts=True)[1].max() <= ref.max_width
    assert (ref.counts == 0).any() and (ref.counts > 0).any()
    assert np.array_equal(ref.records(0, ref.total), want)
    for size in WINDOWS:
        got = np.concatenate([ref.records(a, b) for a, b in _windows(ref.total, size)])
        assert np.array_equal(got, want)


def test_suffix_prefix_matches_with_empty_items_at_both_ends():
    """terminal suffixes without a read start inside their interval, the first and
    the last of the table among them: `aa`, `ca` and `tt` end two reads each and
    start none, `ac` and `gg` between them end one and start another"""
    A, C, G, T = 0, 1, 2, 3
    enc = sr.joined([[G, T, A, A], [C, G, A, A], [A, C, G, T], [T, G, A, C], [G, T, C, A], [A, G, C, A], [C, T, G, G],
                     [G, G, T, C], [A, G, T, T], [G, C, T, T]])
    suf = ou.esa(enc, 4)["suf"]
    rows, terminals, _ = sr.brute_force(enc, 2)
    want = sr.in_order(rows, suf)
    ref = wide.SuffixPrefixMatches(enc, suf, 2)
    assert ref.counts.size == terminals and _has_empty_items_everywhere(ref.counts)
    assert ref.total == want.shape[0] >= 2
    for size in (1, 2, 3):
        got = np.concatenate([ref.records(a, b) for a, b in _windows(ref.total, size)])
        assert np.array_equal(got, want)


def test_tag_matches_without_differences():
    enc = _subject()
    suf = ou.esa(enc, 4)["suf"]
    absent = np.array([3, 3, 3, 3, 3, 3, 3, 3, 3], dtype=np.uint8)
    tags = [absent, enc[25:33], enc[40:46], absent[:7], enc[25:33], np.array([0, 1, 2, 3, 0, 1, 2, 3, 0, 1, 2], dtype=np.uint8), enc[310:330], absent]
    want, _ = tr.expected(enc, suf, tags, 0, tr.FORWARD)
    ref = wide.ExactTagMatches(enc, suf, tags)
    assert _has_empty_items_everywhere(ref.counts) and ref.counts.size == len(tags)
    assert ref.total == want.shape[0] >= 8 and ref.most >= 2
    assert ref.records(0, ref.total).dtype == np.uint64
    for size in (1, 2, 3, 7):
        got = np.concatenate([ref.records(a, b) for a, b in _windows(ref.total, size)])
        assert np.array_equal(got, want)


@pytest.mark.parametrize("L", [2, 5])
def test_maximal_pairs(L):
    # in front of the subject: AAAAA twice behind the same letter, the first run of the table at L = 5
    enc = np.concatenate([[3, 0, 0, 0, 0, 0, 1, 3, 0, 0, 0, 0, 0, 2, 255], _subject()]).astype(np.uint8)
    suf = ou.esa(enc, 4)["suf"]
    want = mp.table_order(mp.brute_force(enc, L), suf)
    ref = wide.MaximalPairs(enc, suf, L)
    lcpfull = ou.tables_given_sa(enc, suf)["lcpfull"]
    g = mp.segments(enc, suf, lcpfull, L)
    assert (ref.counts.size, ref.segments) == (g["idx"].size, g["seg_first"].size - 1)
    assert np.array_equal(ref.pos, np.asarray(suf).astype(np.int64)[g["idx"]])
    assert ref.total == ref.counts.sum() == want.shape[0] > 50
    assert ref.counts[-1] == 0 and (ref.counts[1:-1] == 0).any()     # (the last of a run never has a record)
    assert L != 5 or ref.counts[0] == 0
    M = ref.counts.size
    assert np.array_equal(ref.records(0, M), want)
    for size in (1, 3, 10):
        got = np.concatenate([ref.records(a, min(a + size, M)) for a in range(0, M, size)])
        assert np.array_equal(got, want)
    # the emit calls of the device: whole items, as many as fit
    for capacity in (ref.most, ref.most + 5, 4 * ref.most):
        got, cursor, calls = [], 0, 0
        while True:
            rec, after = ref.emit_call(cursor, capacity)
            if rec.shape[0] == 0:
                assert after == M
                break
            assert after > cursor and rec.shape[0] <= capacity
            got.append(rec)
            cursor, calls = after, calls + 1
        assert calls > 1 and np.array_equal(np.concatenate(got), want)
