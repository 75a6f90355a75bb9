"""Approximate matches of short tags through a packed index on the device
(include/gtamd_pcktag.h, tagmatch.TagMatches.set_index_packed over
pck.PackedIndexReader) against the brute force of tests/tagmatch_reference.py:
every record, none sampled.  The index is the suite's: the engine on the subject
in reverse read mode, PackedIndex.build_from_esa, then a reader opened from the
resident builder or from the host image.  The order inside one (tag, strand) is
the header's, not that of the suffix table, so both sides are sorted by dbstart
there; the window tests compare the device with itself, record for record.

The shapes are the smallest at which each part can go wrong: a child of at most
64 rows is finished by single walks and a wider one becomes a level, a successful
child is located 64 rows at a time, a 2-bit line holds 192 rows and a counter
block of the byte rows 64, the decode works in tiles of 16384 rows."""
import functools
import os

import numpy as np
import pytest

import oracle_util as ou
import tagmatch_reference as tr
from genometools_amd import _lib, esa, pck, tagmatch
from genometools_amd.tagmatch import BEST, FORWARD, REVCOMP, WITH_WILDCARDS

pytestmark = pytest.mark.gpu

WAVES, LEAST, LEVELS = tagmatch.geometry()
BOTH = FORWARD | REVCOMP
WILDCARD, SEPARATOR = 254, 255
SUITE = dict(bsize=10, blbuck=8, locfreq=32, sprank=True)
DNA = ["Atinsert.fna", "Duplicate.fna", "Random.fna", "RandomN.fna", "TTT-small.fna", "trna_glutamine.fna"]
UNIT = np.array([3, 3, 0, 1, 2, 3, 0, 0, 1, 3, 2, 2], dtype=np.uint8)


@pytest.fixture(scope="module")
def tools(gpu):
    with pck.PackedIndex() as builder, pck.PackedIndexReader() as reader, pck.PackedIndexReader() as second, \
            tagmatch.TagMatches() as matcher, tagmatch.TagMatches() as plain:
        yield dict(builder=builder, reader=reader, second=second, matcher=matcher, plain=plain)


# ---- subjects ----

def _random(n, sigma, seed):
    return np.random.default_rng(seed).integers(0, sigma, n, dtype=np.uint8)


def _with_specials(n, sigma, seed):
    """random letters with specials at both ends, in the middle and here and there"""
    enc = _random(n, sigma, seed)
    rng = np.random.default_rng(seed + 1)
    if n >= 8:
        at = rng.integers(0, n, max(2, n // 40))
        enc[at] = rng.choice([WILDCARD, SEPARATOR], at.size)
        enc[0], enc[n - 1] = WILDCARD, SEPARATOR
        enc[n // 2:n // 2 + 3] = [WILDCARD, SEPARATOR, WILDCARD]
    return enc


def _run_of(occurrences):
    """t, a run of A in which A^12 occurs `occurrences` times, t and a tail without A"""
    return np.concatenate([[3], np.zeros(12 + occurrences - 1, dtype=np.uint8), [3], _random(40, 3, 5) + 1]).astype(np.uint8)


def _copies(full, eleven=0, ten=0, seed=7):
    """`full` copies of UNIT, `eleven` of its first 11 letters and `ten` of its first
    10, each followed by a letter that is not the next one of UNIT and by a context
    of its own over a, c, g in which UNIT's first two letters (t t) never occur"""
    rng = np.random.default_rng(seed)
    parts = []
    for cut, count in ((12, full), (11, eleven), (10, ten)):
        for k in range(count):
            stop = [(int(UNIT[cut]) + 1 + k % 2) % 3] if cut < 12 else []     # (a, c or g, and not UNIT[cut])
            parts.append(np.concatenate([UNIT[:cut], stop, rng.integers(0, 3, 17), [k % 3]]).astype(np.uint8))
    order = rng.permutation(len(parts))
    return np.concatenate([parts[i] for i in order]).astype(np.uint8)


def _occurrences(enc, word):
    if len(word) > enc.size:
        return 0
    hit = np.ones(enc.size - len(word) + 1, dtype=bool)
    for k, c in enumerate(word):
        hit &= enc[k:enc.size - len(word) + 1 + k] == c
    return int(hit.sum())


def _cut(enc, at, m):
    tag = enc[at:at + m].copy()
    tag[tag >= 254] = 1
    return tag


def _edited(tag, edits, seed, sigma=4):
    rng = np.random.default_rng(seed)
    tag = list(tag)
    for _ in range(edits):
        at, what = int(rng.integers(len(tag))), int(rng.integers(3))
        if what == 0:
            tag[at] = (tag[at] + 1 + int(rng.integers(sigma - 1))) % sigma
        elif what == 1 and len(tag) < 64:
            tag.insert(at, int(rng.integers(sigma)))
        elif len(tag) > 4:
            del tag[at]
    return np.array(tag, dtype=np.uint8)


def _mixed_tags(enc, count, seed, sigma=4, lengths=(5, 8, 12, 13, 20, 31, 40, 63, 64)):
    rng = np.random.default_rng(seed)
    tags = []
    for k in range(count):
        m = int(rng.choice([x for x in lengths if x < enc.size]))
        tag = _cut(enc, int(rng.integers(0, enc.size - m)), m)
        if k % 3 == 1:
            tag = _edited(tag, 1 + k % 2, seed + k, sigma)
        elif k % 3 == 2 and k % 2 and sigma == 4:
            tag = tr.revcomp(tag)
        tags.append(tag)
    return tags


# ---- the index and the comparison ----

def _open(tools, enc, sigma=4, kw=SUITE, which="reader", host=False):
    """the packed index of the reversed subject, open in tools[which]"""
    if sigma == 20:      # (as `gt packedindex mkindex` falls back to block size 3 over 20 letters)
        kw = dict(kw, bsize=3)
    with esa.EsaEngine(enc.size, sigma) as eng:
        eng.set_readmode(1)
        eng.set_sequence(enc)
        eng.run(esa.WANT_SUF | esa.WANT_BWT)
        tools["builder"].build_from_esa(eng, **kw)
        if host:
            return tools[which].open(tools["builder"].image())
        return tools[which].open_builder(tools["builder"])


def _sorted(records):
    """one (tag, strand) after the other, each by dbstart"""
    return records[np.lexsort((records[:, 1], records[:, 0]))]


@functools.lru_cache(maxsize=None)
def _expected_cached(key, K, flags):
    enc, tags = _expected_cached.inputs[key]
    return tr.expected(enc, np.arange(enc.size + 1), tags, K, flags)      # (this "table" sorts by position)


_expected_cached.inputs = {}


def _expected(enc, tags, K, flags, key=None):
    if key is None:
        return tr.expected(enc, np.arange(enc.size + 1), tags, K, flags)
    _expected_cached.inputs[key] = (enc, tags)
    return _expected_cached(key, K, flags)


def _agree(tools, enc, tags, K, flags=BOTH, key=None, emit=True):
    """the matcher, whose index is set, against the brute force; the sorted records"""
    matcher = tools["matcher"]
    want, best = _expected(enc, tags, K, flags, key)
    info = matcher.prepare(tags, K, flags)
    assert info["matches"] == want.shape[0], (info["matches"], want.shape[0])
    assert np.array_equal(matcher.best_k(), best)
    strands = 2 if flags & BOTH == BOTH else 1
    assert info["jobs"] == strands * len(tags)
    per_job = np.bincount(want[:, 0].astype(np.int64)) if want.shape[0] else np.zeros(1, dtype=np.int64)
    assert info["max_matches_of_one_job"] == per_job.max()
    if not emit:
        return want
    chunks = list(matcher.records())
    got = np.concatenate(chunks) if chunks else np.zeros((0, 3), dtype=np.uint64)
    assert got.dtype == np.uint64 and got.shape == want.shape
    # ascending tag, forward before reverse complement: that part of the order is fixed
    assert np.array_equal(got[:, 0], want[:, 0])
    got = _sorted(got)
    differ = np.flatnonzero((got != want).any(axis=1))
    assert differ.size == 0, (differ[:5], got[differ[:5]], want[differ[:5]])
    assert matcher.info()["emitted"] == want.shape[0]
    return want


# ---- 1: the six DNA fixtures ----

@functools.lru_cache(maxsize=None)
def _fixture(name, protein=False):
    enc = ou.encode_fasta(ou.fixture_path(name), protein)
    letters = tr.PROTEIN if protein else tr.DNA
    tags = [tr.encode_tag(t, letters) for t in tr.read_tags([os.path.join(ou.GOLDEN_DIR, "tagmatch", name + ".tags.fna")])]
    enc.setflags(write=False)
    return enc, tags


@pytest.mark.parametrize("name", DNA)
def test_the_six_dna_fixtures(tools, name):
    enc, tags = _fixture(name)
    assert tags[-1].size == 1
    tools["matcher"].set_index_packed(_open(tools, enc))
    total = _agree(tools, enc, tags, 0, key=(name, "all")).shape[0]
    for K, flags in ((1, BOTH), (2, BOTH), (2, BOTH | BEST), (1, FORWARD), (1, REVCOMP)):
        total += _agree(tools, enc, tags[:-1], K, flags, key=(name, "but one")).shape[0]
    # (RandomN.fna holds wildcards only, TTT-small.fna seven symbols)
    assert total >= {"RandomN.fna": 0, "TTT-small.fna": 50}.get(name, 100)
    if name == DNA[0]:
        with pytest.raises(_lib.EsaError, match="tag number %d of length 1; tags must be longer" % (len(tags) - 1)):
            tools["matcher"].prepare(tags, 1)


# ---- 2: locate flavours ----

FLAVOURS = [dict(), dict(locbitmap=True), dict(locfreq=1, sprank=True), dict(locfreq=7, locbitmap=True, sprank=True),
            dict(bsize=1, blbuck=1), dict(locfreq=0)]


@pytest.mark.parametrize("name", ["Atinsert.fna", "RandomN.fna"])
@pytest.mark.parametrize("kw", FLAVOURS, ids=lambda kw: "-".join("%s%s" % (k[:3], int(v)) for k, v in kw.items()) or "defaults")
def test_locate_flavours(tools, name, kw):
    enc, tags = _fixture(name)
    reader = _open(tools, enc, kw=kw)
    assert reader.info()["locate_interval"] == kw.get("locfreq", 16)
    tools["matcher"].set_index_packed(reader)
    least = 20 if name == "Atinsert.fna" else 0          # (RandomN.fna holds wildcards only)
    if kw.get("locfreq", 16):
        assert _agree(tools, enc, tags[:-1], 1, key=(name, "but one")).shape[0] >= least
        return
    # no locate information: the counts are there, the records are not
    want = _agree(tools, enc, tags[:-1], 1, key=(name, "but one"), emit=False)
    assert want.shape[0] >= least
    with pytest.raises(_lib.EsaError, match="no locate information"):
        list(tools["matcher"].records())
    assert tools["matcher"].info()["emitted"] == 0


# ---- 3: widths of a successful child, and of the children above it ----

@pytest.mark.parametrize("occurrences", [1, 63, 64, 65, 489])
def test_width_of_the_successful_child(tools, occurrences):
    """the 12-mer occurs 1, 63, 64, 65 and 489 times: the batches of the locate.  In
    a run of one letter (K = 1 and 2: the children above succeed, wider by the
    neighbours of the run's ends) and as copies in contexts of their own."""
    unit = np.zeros(12, dtype=np.uint8)
    for enc, word in ((_run_of(occurrences), unit), (_copies(occurrences), UNIT)):
        assert _occurrences(enc, word) == occurrences
        tools["matcher"].set_index_packed(_open(tools, enc))
        assert _agree(tools, enc, [word], 0, FORWARD).shape[0] == occurrences
        _agree(tools, enc, [word, word[:11], _edited(word, 1, 3)], 1)
        _agree(tools, enc, [word, np.roll(word, 1)], 2, FORWARD)


@pytest.mark.parametrize("eleven", [1, 64, 65])
def test_width_of_the_child_above_the_successful_one(tools, eleven):
    """UNIT[:11] occurs in 1, 64 and 65 rows, 30 of them go on with UNIT[11] (none
    where there is one row): with K = 0 the child at depth 11 is finished by single
    walks up to 64 rows and becomes a level from 65, and every child above it is
    wider than 64.  The figures of the walk say which it was."""
    full = 30 if eleven > 1 else 0
    enc = _copies(full, eleven - full, 70)
    widths = [_occurrences(enc, UNIT[:d]) for d in range(13)]
    assert widths[11] == eleven and widths[12] == full and min(widths[1:11]) > 64
    tools["matcher"].set_index_packed(_open(tools, enc))
    assert _agree(tools, enc, [UNIT], 0, FORWARD).shape[0] == full
    info = tools["matcher"].info()
    if eleven <= 64:
        assert (info["levels_pushed"], info["single_walks"]) == (10, eleven)
    else:
        assert (info["levels_pushed"], info["single_walks"]) == (11, 0)
    # one non-empty child a level on this path, but at the root, where a, c, g and t begin
    assert info["children_examined"] >= info["levels_pushed"] + 1
    _agree(tools, enc, [UNIT, UNIT[:11], _edited(UNIT, 1, 4)], 1)
    _agree(tools, enc, [UNIT, _edited(UNIT, 2, 5)], 2)


# ---- 4: deep and wide ----

def test_levels_stay_wide_down_to_the_last_depth(tools):
    enc = np.zeros(500, dtype=np.uint8)
    tools["matcher"].set_index_packed(_open(tools, enc))
    for m in (63, 64):
        for K in (0, 2):
            want = _agree(tools, enc, [np.zeros(m, dtype=np.uint8)], K, FORWARD)
            info = tools["matcher"].info()
            # A^d has 501 - d > 64 rows at every depth d below the successful one, m - K
            assert want.shape[0] == 500 - (m - K) + 1 and info["levels_pushed"] == m - K - 1 and info["single_walks"] == 0
    assert _agree(tools, enc, [np.zeros(1, dtype=np.uint8), np.ones(1, dtype=np.uint8)], 0).shape[0] == 500


# ---- 5: lines and counter rows ----

@pytest.mark.parametrize("rows", [191, 192, 193, 385, 16385])
def test_line_borders_two_bit(tools, rows):
    """bounds in one line, in two lines, a flagged line, the tile border of the decode"""
    enc = _with_specials(rows - 1, 4, rows)
    tools["matcher"].set_index_packed(_open(tools, enc))
    lengths = (5, 8, 12, 13, 20, 31, 40, 63, 64) if rows > 1000 else (3, 4, 5, 8, 12, 31)
    for K in (0, 1, 2):
        want = _agree(tools, enc, _mixed_tags(enc, 40, rows + K, lengths=lengths), K)
        assert want.shape[0] >= 10


def test_two_letters(tools):
    enc = _with_specials(700, 2, 9)
    tools["matcher"].set_index_packed(_open(tools, enc, sigma=2))
    for K in (0, 2):
        assert _agree(tools, enc, _mixed_tags(enc, 30, 11, sigma=2, lengths=(5, 8, 12, 20, 31)), K, FORWARD).shape[0] > 30
    with pytest.raises(_lib.EsaError, match="GTAMD_TAGMATCH_REVCOMP.*4 letters"):
        tools["matcher"].prepare([np.zeros(5, dtype=np.uint8)], 1, BOTH)


@pytest.mark.parametrize("sigma", [5, 20])
@pytest.mark.parametrize("rows", [63, 64, 65, 129, 40000])
def test_byte_rows_and_their_counter_blocks(tools, sigma, rows):
    enc = _with_specials(rows - 1, sigma, rows + sigma)
    tools["matcher"].set_index_packed(_open(tools, enc, sigma=sigma))
    lengths = (5, 8, 12, 13, 20, 31, 40, 63, 64) if rows > 1000 else (3, 4, 5, 8)
    for K in (0, 1, 2):
        want = _agree(tools, enc, _mixed_tags(enc, 30, rows + K, sigma, lengths), K, FORWARD)
        assert want.shape[0] >= 5


def test_protein_fixture(tools):
    enc, tags = _fixture("sw100K1.fsa", True)
    tools["matcher"].set_index_packed(_open(tools, enc, sigma=20))
    assert _agree(tools, enc, tags, 0, FORWARD, key=("protein", "all")).shape[0] > 10
    assert _agree(tools, enc, tags[:-1], 1, FORWARD, key=("protein", "but one")).shape[0] > 10


# ---- 6: windows ----

def _window_cases():
    run = np.zeros(4000, dtype=np.uint8)
    yield run, [np.zeros(12, dtype=np.uint8), np.zeros(5, dtype=np.uint8)], 1
    enc = _with_specials(3000, 4, 41)
    yield enc, _mixed_tags(enc, 60, 3, lengths=(5, 6, 8, 12, 20)), 2


@pytest.mark.parametrize("case", [0, 1])
def test_pieces_of_any_capacity_and_any_cursor(tools, case):
    enc, tags, K = list(_window_cases())[case]
    matcher = tools["matcher"]
    matcher.set_index_packed(_open(tools, enc))
    _agree(tools, enc, tags, K)
    info = matcher.prepare(tags, K)
    whole = np.concatenate(list(matcher.records()))
    assert whole.shape[0] == info["matches"] > 2000
    assert np.array_equal(np.concatenate(list(matcher.records())), whole)       # two full enumerations
    for capacity in (LEAST, LEAST + 1, 1000):
        chunks = list(matcher.records(capacity))
        assert [c.shape[0] for c in chunks[:-1]] == [capacity] * (len(chunks) - 1) and len(chunks) > 2
        assert np.array_equal(np.concatenate(chunks), whole), capacity
    # a cursor in the middle of the job with the most records, and one on its first record
    tagword = np.bincount(whole[:, 0].astype(np.int64)).argmax()
    first = int(np.flatnonzero(whole[:, 0] == tagword)[0])
    many = int((whole[:, 0] == tagword).sum())
    for cursor in (first + many // 2, first + 1, first, whole.shape[0] - 1):
        piece = next(matcher.records(100, cursor=cursor))
        assert np.array_equal(piece, whole[cursor:cursor + 100]), cursor
    assert list(matcher.records(100, cursor=whole.shape[0])) == []
    with pytest.raises(_lib.EsaError, match="cursor %d is not one of this enumeration" % (whole.shape[0] + 1)):
        list(matcher.records(100, cursor=whole.shape[0] + 1))
    with pytest.raises(_lib.EsaError, match="at least %d" % LEAST):
        list(matcher.records(LEAST - 1))
    import torch
    chunks = [c.cpu().numpy().copy() for c in matcher.records(1000, device=True)]
    torch.cuda.synchronize()
    assert np.array_equal(np.concatenate(chunks).astype(np.uint64), whole)


# ---- 7: two ways to the same image ----

def test_a_reader_opened_from_the_builder_and_one_from_the_host_image(tools):
    enc = _with_specials(5000, 4, 77)
    tags = _mixed_tags(enc, 40, 5)
    matcher = tools["matcher"]
    matcher.set_index_packed(_open(tools, enc))
    first = matcher.all_records(tags, 2)
    matcher.set_index_packed(_open(tools, enc, which="second", host=True))
    assert first.shape[0] > 100 and np.array_equal(matcher.all_records(tags, 2), first)


# ---- 8: against the matcher on the suffix table ----

def test_against_the_matcher_on_the_suffix_table(tools):
    """2^20 random symbols, 2000 tags of 32 letters with one random difference,
    every second one reverse-complemented, K = 1"""
    import torch
    n, count, m = 1 << 20, 2000, 32
    enc = _random(n, 4, 2026)
    rng = np.random.default_rng(8)
    tags = []
    for k, at in enumerate(rng.integers(0, n - m, count)):
        tag = _edited(enc[at:at + m], 1, 1000 + k)
        tags.append(tr.revcomp(tag) if k % 2 else tag)
    dev = torch.from_numpy(enc).to("cuda:0")
    with esa.EsaEngine(n, 4) as eng:
        eng.set_sequence_device(dev.data_ptr(), n)
        eng.run(esa.WANT_SUF)
        tools["plain"].set_index_engine(eng, dev.data_ptr(), n)
        want = tools["plain"].all_records(tags, 1)
        want_k = tools["plain"].best_k()
    tools["matcher"].set_index_packed(_open(tools, enc))
    got = tools["matcher"].all_records(tags, 1)
    assert want.shape[0] >= count and np.array_equal(_sorted(got), _sorted(want))
    assert np.array_equal(got[:, 0], want[:, 0]) and np.array_equal(tools["matcher"].best_k(), want_k)


# ---- 9: refusals and switching ----

def test_refusals(tools):
    enc = _with_specials(2000, 4, 3)
    tag = _cut(enc, 5, 12)
    with tagmatch.TagMatches() as f, pck.PackedIndexReader() as closed:
        with pytest.raises(_lib.EsaError, match="packed index reader has no image open"):
            f.set_index_packed(closed)
        with pytest.raises(_lib.EsaError, match="no index is set"):
            f.prepare([tag], 1)
        reader = _open(tools, enc)
        raw = tools["builder"].image()
        f.set_index_packed(reader)
        want = f.all_records([tag], 1)
        assert want.shape[0] >= 1
        with pytest.raises(_lib.EsaError, match="GTAMD_TAGMATCH_WITH_WILDCARDS is not taken with a packed index"):
            f.prepare([tag], 1, BOTH | WITH_WILDCARDS)
        # (refused for its flags before anything is touched: what was prepared stands)
        assert np.array_equal(np.concatenate(list(f.records())), want)
        # the reader loses its image: refused until it holds one again
        f.prepare([tag], 1)
        with pytest.raises(_lib.EsaError, match="packed index reader: "):
            reader.open(raw[:-1])
        with pytest.raises(_lib.EsaError, match="no image open any more"):
            f.prepare([tag], 1)
        with pytest.raises(_lib.EsaError, match="no image open any more"):
            list(f.records())
        with pytest.raises(_lib.EsaError, match="packed index reader has no image open"):
            f.set_index_packed(reader)
        reader.open(raw)
        assert np.array_equal(f.all_records([tag], 1), want)
    five = _with_specials(300, 5, 4)
    tools["matcher"].set_index_packed(_open(tools, five, sigma=5))
    with pytest.raises(_lib.EsaError, match="GTAMD_TAGMATCH_REVCOMP.*4 letters.*has 5"):
        tools["matcher"].prepare([_cut(five, 9, 6)], 1, BOTH)
    with pytest.raises(_lib.EsaError, match="tag number 0 holds a symbol that is no letter"):
        tools["matcher"].prepare([np.array([0, 1, 5, 2], dtype=np.uint8)], 1, FORWARD)


def test_a_reader_opened_again_since_prepare(tools):
    """the places of the jobs and K' are of the image that prepare walked: emit,
    to host or to device memory, refuses the reader once it was opened again, be
    it on the same bytes; K' stays readable, and a new prepare is of the new image"""
    enc = _with_specials(2000, 4, 3)
    tag = _cut(enc, 5, 12)
    with tagmatch.TagMatches() as f:
        reader = _open(tools, enc)
        raw = tools["builder"].image()
        f.set_index_packed(reader)
        want = f.all_records([tag], 1)
        best = f.best_k()
        assert want.shape[0] >= 1 and best.tolist() == [1]
        f.prepare([tag], 1)
        reader.open(raw)
        for device in (False, True):
            with pytest.raises(_lib.EsaError, match="tag matches: the packed index reader was opened again since "
                                                    "gtamd_tagmatch_prepare: what was prepared is of the image before"):
                list(f.records(device=device))
        assert np.array_equal(f.best_k(), best) and f.info()["emitted"] == 0
        assert np.array_equal(f.all_records([tag], 1), want)


def test_tables_are_not_held_to_the_image_of_a_reader(tools):
    """the object goes from the reader to tables: however often the reader is
    opened after that, before or after the prepare, emit gives the records of the tables"""
    enc = _with_specials(2000, 4, 3)
    tag = _cut(enc, 5, 12)
    suf = ou.esa(enc, 4)["suf"]
    want, _ = tr.expected(enc, suf, [tag], 1)
    assert want.shape[0] >= 1
    with tagmatch.TagMatches() as f:
        reader = _open(tools, enc)
        raw = tools["builder"].image()
        f.set_index_packed(reader)
        f.prepare([tag], 1)
        f.set_index(enc, suf)
        reader.open(raw)
        f.prepare([tag], 1)
        reader.open(raw)
        reader.open(raw)
        assert np.array_equal(np.concatenate(list(f.records())), want)


def test_switching_between_a_suffix_table_and_a_packed_index(tools):
    """on one object, in both directions: the records of the suffix table are those
    of tests/test_tagmatch_gpu.py's small subject, in its order, before and after"""
    enc = _random(200, 4, 41)
    enc[70:72] = WILDCARD
    enc[120] = SEPARATOR
    suf = ou.esa(enc, 4)["suf"]
    tags = [_cut(enc, 20, 5), _random(5, 4, 5), _cut(enc, 100, 30)]
    want, best = tr.expected(enc, suf, tags, 2)
    wild, _ = tr.expected(enc, suf, tags, 2, BOTH | WITH_WILDCARDS)
    assert wild.shape[0] >= want.shape[0] > 50
    matcher = tools["matcher"]
    reader = _open(tools, enc)
    for _ in range(2):
        matcher.set_index_packed(reader)
        assert np.array_equal(_sorted(matcher.all_records(tags, 2)), _sorted(want))
        matcher.set_index(enc, suf)
        assert np.array_equal(matcher.all_records(tags, 2), want) and np.array_equal(matcher.best_k(), best)
        assert np.array_equal(matcher.all_records(tags, 2, BOTH | WITH_WILDCARDS), wild)
