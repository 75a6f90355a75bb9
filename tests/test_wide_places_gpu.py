"""The 64-bit PLACES of the match finders' records, across 2^32: query matches
(genometools_amd/qmatch.py), suffix-prefix matches (spm.py), tag matches
(tagmatch.py, whose window code -- JobWindow, JobOffsets, RecordStage of
csrc/esa_jobs.h -- is that of the local alignments too) and maximal pairs
(maxpairs.py).  Every one of them counts per item, scans the counts in 64 bits
and emits any window of the enumeration by candidate, record or suffix number;
the other suites stay below 2 * 10^7 of these numbers, so a truncation to 32 bits
behind the scan would pass them all.

The prepare steps are O(input) and the emit work is that of the window, so a
highly repetitive text of 0.3 to 1.7 million symbols gives more than 2^32 + 2^24
records or candidates -- asserted first, from the reference alone -- of which a
test emits a few thousand around 2^32 and at the end.  The reference is
tests/wide_places_reference.py: exact counts per item and the records of any
window without expanding the rest, held to the full references by
tests/test_wide_places_reference.py.

Per consumer: the totals of prepare; a window that straddles 2^32 and begins
inside an item (for qmatch also a second launch of the emit call); one that ends
at 2^32, with the cursor there afterwards, and one that begins there; one in the
last tenth of the enumeration that crosses items; the last records, after which a
call writes nothing and leaves the cursor; a cursor beyond the total, refused;
and the straddling window again with 4-byte suffix entries set from device
memory and records written to device memory (the others: 8-byte entries from
host memory, records to host memory).  Every record of a window is compared, in
order.  The cursor of maxpairs counts suffixes in runs, so its windows are whole
suffixes whose records lie around those places.  For tagmatch also one window of
a search with one difference on the same index.

The suffix tables come from the CPU oracle (ou.esa), never from the engine;
nothing had to be shrunk or built on the device for that.

Measured wall times, the 21 tests together 5.5 s on an MI355X host.  What is
shared is made once per consumer and counted with its first test:

                oracle tables   reference   prepare (device)   every later test
    qmatch         0.14 s         0.11 s        1.15 ms           <= 0.01 s
    spm            0.34 s         0.84 s        1.35 ms           <= 0.03 s
    tagmatch       0.34 s         0.19 s        4.43 ms           <= 0.02 s
    maxpairs       0.37 s         0.09 s       23.85 ms           <= 0.06 s

and 0.26 s for the search with one difference, nearly all of it its reference.
On a slower host without a device the oracle took 0.7 to 1.5 s per input and the
reference of spm, the slowest, 3.7 s (a sort of all h-mers for each of the 18
lengths h a terminal suffix can have)."""
import functools
import time

import numpy as np
import pytest

import oracle_util as ou
import tagmatch_reference as tr
import wide_places_reference as wide
from genometools_amd import _lib, maxpairs, qmatch, spm, tagmatch

pytestmark = pytest.mark.gpu

WORD = 1 << 32
BOUND = WORD + (1 << 24)           # every enumeration here has at least this many places
D, E = 3001, 5003                  # places in front of and behind 2^32 of a straddling window
REFUSED = "is not one of this enumeration"


def _timed(what, fn, *args):
    t0 = time.perf_counter()
    out = fn(*args)
    print("%s: %.2f s on the CPU" % (what, time.perf_counter() - t0))
    return out


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def _tables(name, enc):
    t = _timed("oracle tables of %s, %d symbols" % (name, enc.size), ou.esa, enc, 4)
    return _frozen(enc, t["suf"], t["lcp"], t["llv"])


def _device_copy(a, skew=0):
    import torch
    t = torch.empty(a.nbytes + 64, dtype=torch.uint8, device="cuda:0")
    t[skew:skew + a.nbytes] = torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to("cuda:0")
    torch.cuda.synchronize()
    return t, t.data_ptr() + skew


def _calls(emit, capacity, cursor, device=False, only=None):
    """(the chunks of the emit calls from `cursor` on, as int64; the cursor behind
    the last call): until a call writes nothing, or `only` calls"""
    cur = np.array([cursor], dtype=np.uint64)
    chunks = []
    calls = emit(capacity, device, cur)
    for chunk in calls:
        assert len(chunks) < 8, "an enumeration that does not end where it should"
        chunks.append(chunk.cpu().numpy().copy() if device else chunk.astype(np.int64))
        if only is not None and len(chunks) == only:
            calls.close()
            break
    return chunks, int(cur[0])


def _one_call(emit, capacity, cursor, device=False):
    chunks, after = _calls(emit, capacity, cursor, device, only=1)
    assert len(chunks) == 1
    return chunks[0], after


def _same(got, want):
    want = np.asarray(want).astype(np.int64)
    assert got.dtype == np.int64 and got.shape == want.shape
    assert np.array_equal(got, want)


def _begins_inside_an_item(off, place):
    return off[int(np.searchsorted(off, place, side="right")) - 1] < place


# ---- the consumers whose cursor is a record number: spm and tagmatch -------------

def _record_windows(emit, ref, least):
    """what both assert for the windows of the table in the docstring"""
    total, off = ref.total, ref.off
    assert total >= BOUND and least <= D
    # straddle
    assert _begins_inside_an_item(off, WORD - D)
    got, after = _one_call(emit, D + E, WORD - D)
    _same(got, ref.records(WORD - D, WORD + E))
    assert after == WORD + E
    # ends at 2^32, begins at 2^32
    got, after = _one_call(emit, 4097, WORD - 4097)
    _same(got, ref.records(WORD - 4097, WORD))
    assert after == WORD
    got, after = _one_call(emit, 4099, WORD)
    _same(got, ref.records(WORD, WORD + 4099))
    assert after == WORD + 4099
    # wholly above, in the last tenth (where 2^32 lies too), over more than one item
    a = WORD + (total - WORD) // 2
    many = ref.most + 1000
    assert a > WORD and 10 * a >= 9 * total and a + many < total
    assert np.unique(wide.places(off, a, a + many)[0]).size >= 2
    got, after = _one_call(emit, many, a)
    _same(got, ref.records(a, a + many))
    assert after == a + many
    return np.unique(wide.places(off, WORD - D, WORD + E)[0])         # the items of the straddling window


def _record_end(emit, ref):
    """the last records, the call behind them, a cursor beyond"""
    total = ref.total
    chunks, after = _calls(emit, 4096, total - D)
    assert len(chunks) == 1 and after == total
    _same(chunks[0], ref.records(total - D, total))
    assert _calls(emit, 4096, total) == ([], total)
    with pytest.raises(_lib.EsaError, match=REFUSED):
        _calls(emit, 4096, total + 1)


# ---- query matches ----------------------------------------------------------------

def _units(seed, count):
    """`count` units A^8 s, s one of C, G, T"""
    u = np.zeros((count, 9), dtype=np.uint8)
    u[:, 8] = np.random.default_rng(seed).integers(1, 4, count)
    return u.reshape(-1)


@functools.lru_cache(maxsize=None)
def _qmatch_case():
    """Subject and query of 36,000 units A^8 s each, L = 8: the word A^8 of every
    query unit has 36,000 candidates, of which those behind another s are
    records (two thirds); the eight words that hold the s of the unit have about
    12,000 candidates each and no record, the letter in front being A on both
    sides.  The query begins three symbols into its first unit, which puts 2^32
    inside the candidates of a word A^8"""
    enc, suf, _, _ = _tables("qmatch", _units(1, 36000))
    query = _frozen(_units(2, 36000)[3:].copy())[0]
    return enc, suf, query, _timed("reference of qmatch", wide.QueryMatches, enc, suf, query, 8)


@pytest.fixture(scope="module")
def qm(gpu):
    enc, suf, query, ref = _qmatch_case()
    assert suf.dtype == np.uint64
    with qmatch.QueryMatches() as f:
        f.set_index(enc, suf)
        info = f.prepare(query, 8)
        print("qmatch: %d candidates, %d seeds, widest interval %d, prepare %.2f ms on the device"
              % (info["candidates"], info["seeds"], info["max_width"], info["device_ms"]))
        yield f, info, ref


def _qm_expected(ref, cursor, capacity, least):
    """every call until nothing is written: the chunks that hold a record, the cursor"""
    chunks = []
    while True:
        rec, cursor = ref.emit_call(cursor, capacity, least)
        if rec.shape[0] == 0:
            return chunks, cursor
        chunks.append(rec)


def test_qmatch_totals(qm):
    _, info, ref = qm
    assert ref.total >= BOUND and isinstance(ref.total, int)
    assert info["candidates"] == ref.total
    assert (info["positions"], info["seeds"], info["max_width"]) == (ref.counts.size, ref.seeds, ref.most)


def test_qmatch_window_that_straddles(qm):
    f, _, ref = qm
    least = qmatch.geometry()[1]
    a, capacity = WORD - D, 8 * least
    assert _begins_inside_an_item(ref.off, a) and capacity > D
    kept, _ = ref.candidates(a, a + capacity)
    assert kept.any() and not kept.all() and capacity - int(kept.sum()) >= least      # a second launch follows
    before = f.info()["matches"]
    got, after = _one_call(f.emit, capacity, a)
    want, cursor = ref.emit_call(a, capacity, least)
    _same(got, want)
    assert after == cursor > WORD + (capacity - D)
    assert f.info()["matches"] == before + want.shape[0]


def test_qmatch_window_that_ends_at_2_32(qm):
    f, _, ref = qm
    least = qmatch.geometry()[1]
    want, cursor = ref.emit_call(WORD - least, least, least)
    assert cursor == WORD and want.shape[0] > 0            # (a call of the least capacity that keeps a record: one chunk)
    got, after = _one_call(f.emit, least, WORD - least)
    _same(got, want)
    assert after == WORD


def test_qmatch_window_that_begins_at_2_32(qm):
    f, _, ref = qm
    least = qmatch.geometry()[1]
    want, cursor = ref.emit_call(WORD, 5 * least, least)
    assert want.shape[0] > least
    got, after = _one_call(f.emit, 5 * least, WORD)
    _same(got, want)
    assert after == cursor


def test_qmatch_window_wholly_above(qm):
    f, _, ref = qm
    least = qmatch.geometry()[1]
    a = ref.total - ref.total // 20
    assert a > WORD and 10 * a >= 9 * ref.total
    want, cursor = ref.emit_call(a, 40 * least, least)
    assert want.shape[0] > 0 and cursor < ref.total
    assert np.unique(wide.places(ref.off, a, cursor)[0]).size >= 3     # crosses items
    got, after = _one_call(f.emit, 40 * least, a)
    _same(got, want)
    assert after == cursor


def test_qmatch_last_window_and_beyond(qm):
    f, _, ref = qm
    least = qmatch.geometry()[1]
    a = ref.total - 3 * ref.most                           # inside the candidates of the last word A^8
    want, cursor = _qm_expected(ref, a, 16 * least, least)
    assert cursor == ref.total and len(want) >= 1
    chunks, after = _calls(f.emit, 16 * least, a)
    assert after == ref.total and len(chunks) == len(want)
    for got, rec in zip(chunks, want):
        _same(got, rec)
    assert _calls(f.emit, 16 * least, ref.total) == ([], ref.total)
    with pytest.raises(_lib.EsaError, match=REFUSED):
        _calls(f.emit, 16 * least, ref.total + 1)


def test_qmatch_narrow_table_on_the_device(gpu):
    enc, suf, query, ref = _qmatch_case()
    least = qmatch.geometry()[1]
    keep = [_device_copy(enc), _device_copy(suf.astype(np.uint32), 8)]
    with qmatch.QueryMatches() as f:
        f.set_index_device(keep[0][1], enc.size, keep[1][1], 4)
        assert f.prepare(query, 8)["candidates"] == ref.total
        got, after = _one_call(f.emit, 8 * least, WORD - D, device=True)
        want, cursor = ref.emit_call(WORD - D, 8 * least, least)
        _same(got, want)
        assert after == cursor


# ---- suffix-prefix matches --------------------------------------------------------

SPM_READS, SPM_L = (1 << 16, 4200), 8


@functools.lru_cache(maxsize=None)
def _spm_case():
    """Two families of reads P mid P of 25 letters, 65,536 with one P of 8
    letters and 4,200 with another that sorts behind it; the mids are nine
    letters each and all distinct.  At L = 8 the P that ends a read is a terminal
    suffix with every read of its family in its interval: 65,536 suffixes of
    65,536 records, which end at 2^32 exactly, and 4,200 of 4,200.  The other
    half a million terminal suffixes -- ends of a mid with P behind them, shared
    by chance -- have none and stand in front of, between and behind the two
    families, so that the scanned offsets stand still over long stretches, one
    of them at 2^32"""
    rng = np.random.default_rng(3)
    total = sum(SPM_READS)
    P = rng.integers(0, 4, (2, SPM_L), dtype=np.uint8)
    P[:, 0] = [0, 2]
    P = np.repeat(P, SPM_READS, axis=0)[rng.permutation(total)]
    number = rng.permutation(4 ** 9)[:total]
    mid = ((number[:, None] >> (2 * np.arange(9))) & 3).astype(np.uint8)
    reads = np.concatenate([P, mid, P, np.full((total, 1), 255, dtype=np.uint8)], axis=1)
    enc, suf, lcp, llv = _tables("spm", reads.reshape(-1)[:-1].copy())
    return enc, suf, lcp, llv, _timed("reference of spm", wide.SuffixPrefixMatches, enc, suf, SPM_L)


@pytest.fixture(scope="module")
def sp(gpu):
    enc, suf, lcp, llv, ref = _spm_case()
    assert suf.dtype == np.uint64
    with spm.SuffixPrefixMatches() as f:
        f.set_index(enc, suf, lcp, llv)
        info = f.prepare(SPM_L)
        print("spm: %d matches, %d terminal suffixes, %d read starts, prepare %.2f ms on the device"
              % (info["matches"], info["terminal_suffixes"], info["read_starts"], info["device_ms"]))
        yield f, info, ref


def test_spm_totals(sp):
    _, info, ref = sp
    assert ref.total >= BOUND and isinstance(ref.total, int)
    assert info["matches"] == ref.total
    assert (info["terminal_suffixes"], info["read_starts"], info["table_entries"]) == \
        (ref.counts.size, ref.read_starts.size, ref.enc.size + 1)
    assert (info["max_matches_of_one_suffix"], info["max_width"]) == (ref.most, ref.max_width)
    # most terminal suffixes have no record
    assert (ref.counts >= min(SPM_READS)).sum() == sum(SPM_READS) and ref.counts.size > 5 * sum(SPM_READS)


def test_spm_windows_around_2_32(sp):
    f, _, ref = sp
    items = _record_windows(f.matches, ref, spm.geometry()[1])
    # the straddling window: the end of one family, suffixes without a record, the start of the other
    counts = ref.counts[items[0]:items[-1] + 1]
    assert counts[0] > 0 and counts[-1] > 0 and (counts == 0).sum() > 1000


def test_spm_last_window_and_beyond(sp):
    f, _, ref = sp
    _record_end(f.matches, ref)


def test_spm_narrow_table_on_the_device(gpu):
    enc, suf, lcp, llv, ref = _spm_case()
    keep = [_device_copy(enc), _device_copy(suf.astype(np.uint32), 8), _device_copy(lcp, 5), _device_copy(llv, 16)]
    with spm.SuffixPrefixMatches() as f:
        f.set_index_device(keep[0][1], enc.size, keep[1][1], 4, keep[2][1], keep[3][1] if llv.shape[0] else None,
                           llv.shape[0])
        assert f.prepare(SPM_L)["matches"] == ref.total
        got, after = _one_call(f.matches, D + E, WORD - D, device=True)
        _same(got, ref.records(WORD - D, WORD + E))
        assert after == WORD + E


# ---- tag matches ------------------------------------------------------------------

TAG_COPIES = 66000


@functools.lru_cache(maxsize=None)
def _tag_index():
    """66,000 units of one word of 12 random letters and three random letters
    behind it"""
    rng = np.random.default_rng(4)
    word = rng.integers(0, 4, 12, dtype=np.uint8)
    tails = rng.integers(0, 4, (TAG_COPIES, 3), dtype=np.uint8)
    enc, suf, _, _ = _tables("tagmatch", np.concatenate([np.tile(word, (TAG_COPIES, 1)), tails], axis=1).reshape(-1))
    return enc, suf, word


@functools.lru_cache(maxsize=None)
def _tag_case():
    """66,000 tags of 12 letters, read forward, no difference: the word itself,
    which stands at 66,000 places -- but tags 250, 1250, ... and the first and
    the last one stand nowhere, and tags 750, 1750, ... are the end of the word
    with the three letters behind it, at about a thousand places"""
    enc, suf, word = _tag_index()
    absent = word.copy()
    absent[5] = (absent[5] + 1) % 4
    tags = [word] * TAG_COPIES
    for t in range(250, TAG_COPIES, 1000):
        tags[t] = absent
        tags[t + 500] = enc[15 * t + 3:15 * t + 15]
    tags[0] = tags[-1] = absent
    return enc, suf, tags, _timed("reference of tagmatch", wide.ExactTagMatches, enc, suf, tags)


@pytest.fixture(scope="module")
def tm(gpu):
    enc, suf, tags, ref = _tag_case()
    assert suf.dtype == np.uint64
    with tagmatch.TagMatches() as f:
        f.set_index(enc, suf)
        info = f.prepare(tags, 0, tagmatch.FORWARD)
        print("tagmatch: %d matches of %d jobs, prepare %.2f ms on the device"
              % (info["matches"], info["jobs"], info["device_ms"]))
        yield f, info, ref


def test_tagmatch_totals(tm):
    _, info, ref = tm
    assert ref.total >= BOUND and isinstance(ref.total, int)
    assert info["matches"] == ref.total
    assert (info["jobs"], info["max_matches_of_one_job"]) == (ref.counts.size, ref.most)
    assert ref.counts[0] == 0 == ref.counts[-1] and (ref.counts == 0).sum() == 68
    assert ((ref.counts > 0) & (ref.counts < TAG_COPIES // 10)).sum() == 66


def test_tagmatch_windows_around_2_32(tm):
    f, _, ref = tm
    _record_windows(f.records, ref, tagmatch.geometry()[1])
    assert f.info()["emitted"] >= D + E


def test_tagmatch_window_over_jobs_without_and_with_few_records(tm):
    """tag 65,250 stands nowhere and tag 65,750 at few places: the jobs of a window
    from the last records of tag 65,249 on, and one around tag 65,750"""
    f, _, ref = tm
    assert ref.counts[65250] == 0 < ref.counts[65750] < 4001 - 777
    for a in (int(ref.off[65250]) - 1001, int(ref.off[65750]) - 777):
        assert a > WORD
        got, after = _one_call(f.records, 4001, a)
        _same(got, ref.records(a, a + 4001))
        assert after == a + 4001 and np.unique(got[:, 0]).size >= 2


def test_tagmatch_last_window_and_beyond(tm):
    f, _, ref = tm
    _record_end(f.records, ref)


def test_tagmatch_narrow_table_on_the_device(gpu):
    enc, suf, tags, ref = _tag_case()
    keep = [_device_copy(enc), _device_copy(suf.astype(np.uint32), 8)]
    with tagmatch.TagMatches() as f:
        f.set_index_device(keep[0][1], enc.size, keep[1][1], 4)
        assert f.prepare(tags, 0, tagmatch.FORWARD)["matches"] == ref.total
        got, after = _one_call(f.records, D + E, WORD - D, device=True)
        _same(got, ref.records(WORD - D, WORD + E))
        assert after == WORD + E


def test_tagmatch_window_of_a_search_with_one_difference(gpu):
    """two tags, K = 1, on the same index: every place of the word is a match,
    and so are the places one in front of it and behind it; the total stays far
    below 2^32, the windows cross from one job into the next"""
    enc, suf, word = _tag_index()
    other = word.copy()
    other[7] = (other[7] + 2) % 4
    tags = [word, other]
    want, _ = tr.expected(enc, suf, tags, 1, tr.FORWARD)
    first = np.flatnonzero(np.diff(want[:, 0].astype(np.int64))) + 1          # of the second job
    assert first.size == 1 and want.shape[0] > 3 * TAG_COPIES
    with tagmatch.TagMatches() as f:
        f.set_index(enc, suf)
        info = f.prepare(tags, 1, tagmatch.FORWARD)
        print("tagmatch, one difference: %d matches, prepare %.2f ms on the device" % (info["matches"], info["device_ms"]))
        assert info["matches"] == want.shape[0]
        for a in (int(first[0]) - 2001, want.shape[0] - 1501):
            got, after = _one_call(f.records, 4001, a)
            _same(got, want[a:a + 4001])
            assert after == min(a + 4001, want.shape[0])


# ---- maximal pairs ----------------------------------------------------------------

MP_UNITS, MP_L = 100000, 8


@functools.lru_cache(maxsize=None)
def _maxpairs_case():
    """100,000 units l w r: one word w of 8 random letters between two random
    letters.  The suffixes that start with w are one run of 100,000, and three
    pairs in eight of it have different letters in front: 3.75 * 10^9 records;
    the suffixes that start one letter earlier, or inside w, make the other runs"""
    rng = np.random.default_rng(5)
    w = np.tile(rng.integers(0, 4, MP_L, dtype=np.uint8), (MP_UNITS, 1))
    flank = rng.integers(0, 4, (2, MP_UNITS, 1), dtype=np.uint8)
    enc, suf, lcp, llv = _tables("maxpairs", np.concatenate([flank[0], w, flank[1]], axis=1).reshape(-1))
    return enc, suf, lcp, llv, _timed("reference of maxpairs", wide.MaximalPairs, enc, suf, MP_L)


@pytest.fixture(scope="module")
def mx(gpu):
    enc, suf, lcp, llv, ref = _maxpairs_case()
    assert suf.dtype == np.uint64
    with maxpairs.MaxPairs() as f:
        f.set_index(enc, suf, lcp, llv)
        info = f.prepare(MP_L)
        print("maxpairs: %d pairs, %d suffixes in %d runs, at most %d of one suffix, prepare %.2f ms on the device"
              % (info["pairs"], info["run_suffixes"], info["runs"], info["max_pairs_of_one_suffix"], info["device_ms"]))
        yield f, info, ref


def _mp_window(f, ref, k0, capacity, device=False):
    """one call from suffix k0 on against the reference; (k0, the cursor afterwards)"""
    want, cursor = ref.emit_call(k0, capacity)
    assert want.shape[0] > 0
    got, after = _one_call(f.pairs, capacity, k0, device)
    _same(got, want)
    assert after == cursor
    return k0, after


def test_maxpairs_totals(mx):
    _, info, ref = mx
    assert ref.total >= BOUND and isinstance(ref.total, int)
    assert info["pairs"] == ref.total
    assert (info["run_suffixes"], info["runs"], info["segments"]) == (ref.counts.size, ref.runs, ref.segments)
    assert info["max_pairs_of_one_suffix"] == ref.most


def test_maxpairs_windows_around_2_32(mx):
    f, _, ref = mx
    off, capacity = ref.off, 2 * ref.most
    # straddle: from the last suffix whose first record lies below 2^32 - D
    k0 = int(np.searchsorted(off, WORD - D, side="left")) - 1
    k0, k1 = _mp_window(f, ref, k0, capacity)
    assert off[k0] < WORD - D and off[k1] > WORD
    # ends at, and begins at, the border of two suffixes next to 2^32
    border = int(np.argmin(np.abs(off - WORD)))
    assert 0 < off[border] < ref.total and abs(int(off[border]) - WORD) <= ref.most
    k0 = int(np.searchsorted(off, off[border] - ref.most, side="right")) - 1
    room = int(off[border] - off[k0])                      # the records of the suffixes k0 to border - 1, and no more
    assert room >= ref.most and ref.counts[border] > 0
    assert _mp_window(f, ref, k0, room)[1] == border
    assert _mp_window(f, ref, border, capacity)[1] > border
    # wholly above, in the last tenth
    k0 = int(np.searchsorted(off, ref.total - ref.total // 20, side="left"))
    assert off[k0] > WORD and 10 * int(off[k0]) >= 9 * ref.total
    assert _mp_window(f, ref, k0, capacity)[1] >= k0 + 2


def test_maxpairs_last_window_and_beyond(mx):
    f, _, ref = mx
    M, capacity = ref.counts.size, 2 * ref.most
    k0 = int(np.searchsorted(ref.off, ref.total - D, side="right")) - 1
    chunks, after = _calls(f.pairs, capacity, k0)
    assert len(chunks) == 1 and after == M
    _same(chunks[0], ref.records(k0, M))
    assert chunks[0].shape[0] == ref.total - ref.off[k0] >= D
    assert _calls(f.pairs, capacity, M) == ([], M)
    with pytest.raises(_lib.EsaError, match=REFUSED):
        _calls(f.pairs, capacity, M + 1)


def test_maxpairs_narrow_table_on_the_device(gpu):
    enc, suf, lcp, llv, ref = _maxpairs_case()
    keep = [_device_copy(enc), _device_copy(suf.astype(np.uint32), 8), _device_copy(lcp, 5), _device_copy(llv, 16)]
    with maxpairs.MaxPairs() as f:
        f.set_index_device(keep[0][1], enc.size, keep[1][1], 4, keep[2][1], keep[3][1] if llv.shape[0] else None,
                           llv.shape[0])
        assert f.prepare(MP_L)["pairs"] == ref.total
        k0 = int(np.searchsorted(ref.off, WORD - D, side="left")) - 1
        k0, k1 = _mp_window(f, ref, k0, 2 * ref.most, device=True)
        assert ref.off[k0] < WORD < ref.off[k1]
