"""Local alignments through a packed index on the device
(include/gtamd_pcklocali.h, locali.LocalAlignments.set_index_packed over
pck.PackedIndexReader) against the statement per start position of
tests/locali_reference.py: every record, none sampled.  The index is the
suite's: the engine on the subject in reverse read mode,
PackedIndex.build_from_esa, then a reader opened from the resident builder or
from the host image.  The order inside a query is the header's, not that of the
suffix table, so both sides are sorted by dbstart there; the window tests compare
the device with itself, record for record.

The shapes are the smallest at which each part can go wrong: a job walks the q
letters of its code before its interval (matches shallower than q, codes without
an interval), a child of one row is finished alone and a wider one becomes a
level, a successful child is located 64 rows at a time, a column is computed 64
rows a step, a 2-bit line holds 192 rows and a counter block of the byte rows
64, the decode works in tiles of 16384 rows."""
import functools
import os

import numpy as np
import pytest

import locali_golden as lg
import locali_reference as lr
import oracle_util as ou
from genometools_amd import _lib, esa, locali, pck

pytestmark = pytest.mark.gpu

WAVES, LEAST, LONGEST, STACK = locali.geometry()
WILDCARD, SEPARATOR = 254, 255
SUITE = dict(bsize=10, blbuck=8, locfreq=32, sprank=True)
DNA = ["Atinsert.fna", "Duplicate.fna", "Random.fna", "RandomN.fna", "TTT-small.fna", "trna_glutamine.fna"]
UNIT = np.array([3, 3, 0, 1, 2, 3, 0, 0, 1, 3, 2, 2], dtype=np.uint8)
ONE = (1, -1, -1)
STRICT = (1, -2, -2)          # random alignments die early: the reference stays quick
GENEROUS = (2, -1, -1)


@pytest.fixture(scope="module")
def tools(gpu):
    with pck.PackedIndex() as builder, pck.PackedIndexReader() as reader, pck.PackedIndexReader() as second, \
            locali.LocalAlignments() as aligner, locali.LocalAlignments() as plain:
        yield dict(builder=builder, reader=reader, second=second, aligner=aligner, plain=plain)


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
    query = enc[at:at + m].copy()
    query[query >= 254] = 1
    return query


def _edited(query, edits, seed, sigma=4):
    rng = np.random.default_rng(seed)
    query = list(query)
    for _ in range(edits):
        at, what = int(rng.integers(len(query))), int(rng.integers(3))
        if what == 0:
            query[at] = (query[at] + 1 + int(rng.integers(sigma - 1))) % sigma
        elif what == 1:
            query.insert(at, int(rng.integers(sigma)))
        elif len(query) > 4:
            del query[at]
    return np.array(query, dtype=np.uint8)


def _mixed_queries(enc, count, seed, sigma=4, lengths=(8, 13, 20, 31, 40, 64, 90)):
    rng = np.random.default_rng(seed)
    queries = []
    for k in range(count):
        m = int(rng.choice([x for x in lengths if x < enc.size]))
        query = _cut(enc, int(rng.integers(0, enc.size - m)), m)
        if k % 3:
            query = _edited(query, 1 + k % 4, seed + k, sigma)
        queries.append(query)
    return queries


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
    """one query after the other, each by dbstart"""
    return records[np.lexsort((records[:, 1], records[:, 0]))]


@functools.lru_cache(maxsize=None)
def _brute_one(enc_key, query, scores, T):
    """the records of one query (as bytes) with query number 0, by dbstart; shared"""
    enc = _brute_one.subjects[enc_key]
    found = lr.matches_of_query(enc, np.frombuffer(query, dtype=np.uint8), *scores, T=T)
    rec = np.array([(0, p, found[p][0] | found[p][1] << 32, found[p][2] | found[p][3] << 32) for p in sorted(found)],
                   dtype=np.uint64).reshape(-1, 4)
    rec.setflags(write=False)
    return rec


_brute_one.subjects = {}


def _brute(enc, queries, scores, T):
    key = (enc.size, hash(enc.tobytes()))
    _brute_one.subjects[key] = enc
    parts = []
    for number, query in enumerate(queries):
        rec = _brute_one(key, np.ascontiguousarray(query, dtype=np.uint8).tobytes(), tuple(scores), T).copy()
        rec[:, 0] = number
        parts.append(rec)
    return np.concatenate(parts) if parts else np.zeros((0, 4), dtype=np.uint64)


def _esa_path(tools, enc, sigma, queries, scores, T):
    """the records of the aligner on the suffix table, each query by dbstart"""
    tools["plain"].set_index(enc, ou.esa(enc, sigma)["suf"], sigma)
    return _sorted(tools["plain"].all_records(queries, T, *scores))


def _same(got, want):
    assert got.dtype == np.uint64 and got.shape == want.shape, (got.shape, want.shape)
    differ = np.flatnonzero((got != want).any(axis=1))
    assert differ.size == 0, (differ[:5], got[differ[:5]], want[differ[:5]])


def _agree(tools, enc, queries, T, scores=STRICT, sigma=4, brute=True, esa_too=False, stack_words=0,
           cut_depth=locali.AUTO, capacity=locali.DEFAULT_CAPACITY):
    """the aligner, whose index is set, against the brute force (and the -esa path); the sorted records and the info"""
    aligner = tools["aligner"]
    aligner.set_limits(stack_words, cut_depth)
    raw = aligner.all_records(queries, T, *scores, capacity=capacity)
    aligner.set_limits()
    info = aligner.info()
    got = _sorted(raw)
    assert np.array_equal(got[:, 0], raw[:, 0])           # ascending query: that part of the order is fixed
    if brute:
        _same(got, _brute(enc, queries, scores, T))
    if esa_too:
        _same(got, _esa_path(tools, enc, sigma, queries, scores, T))
    assert info["groups"] == sigma ** info["cut_depth"] and info["jobs"] == len(queries) * info["groups"]
    assert info["matches"] == info["emitted"] == got.shape[0]
    return got, info


# ---- 1: the fixtures ----

@functools.lru_cache(maxsize=None)
def _fixture(name, protein=False):
    enc = ou.encode_fasta(ou.fixture_path(name), protein)
    queries = lg.read_queries([os.path.join(lg.QUERYDIR, name + ".queries.fna")], protein)
    enc.setflags(write=False)
    return enc, queries


@pytest.mark.parametrize("name", DNA + ["sw100K1.fsa"])
def test_the_fixtures(tools, name):
    """each fixture with its queries at three thresholds under match 2, mismatch -1,
    gapextend -1: against the brute force and against the -esa path on the device.
    The protein subject has byte rows and their 64-row counter blocks."""
    protein = name == "sw100K1.fsa"
    sigma = 20 if protein else 4
    enc, queries = _fixture(name, protein)
    assert queries[-1].size == 1 and any((q == WILDCARD).any() for q in queries)
    tools["aligner"].set_index_packed(_open(tools, enc, sigma))
    total = 0
    for T in (20, 30, 60):
        total += _agree(tools, enc, queries, T, GENEROUS, sigma, esa_too=True)[0].shape[0]
    # (RandomN.fna holds wildcards only, TTT-small.fna seven symbols)
    assert total >= {"RandomN.fna": 0, "TTT-small.fna": 0}.get(name, 5)


# ---- 2: cut depths, and matches shallower than q ----

def test_every_cut_depth_gives_the_same_records(tools):
    enc = _with_specials(3000, 4, 41)
    queries = _mixed_queries(enc, 5, 9)
    tools["aligner"].set_index_packed(_open(tools, enc))
    first = None
    for cut_depth, q in ((0, 0), (1, 1), (2, 2), (locali.AUTO, 6), (8, 8), (16, 8)):
        got, info = _agree(tools, enc, queries, 9, cut_depth=cut_depth)
        assert info["cut_depth"] == q and info["groups"] == 4 ** q
        first = got if first is None else first
        assert got.shape[0] > 20 and np.array_equal(got, first)


@pytest.mark.parametrize("cut_depth", [0, 1, 2, 3, locali.AUTO, 8])
def test_matches_shallower_than_the_cut_depth(tools, cut_depth):
    """queries of 1, 2 and 3 letters with T = 1 and T = m: every match has at most m
    <= 3 letters (T = 1: one), fewer than the q of most of these cut depths, so it is
    the job whose other letters are 0 that gives it.  The subject has no g: the
    query g has no match, and the codes with a g have no interval."""
    enc = _with_specials(700, 2, 9)
    enc[enc == 1] = 3
    queries = [np.array(q, dtype=np.uint8) for q in ([0], [3], [2], [0, 3], [3, 3], [0, 2], [3, 0, 3], [0, 0, 0], [2, 3, 0])]
    tools["aligner"].set_index_packed(_open(tools, enc))
    for scores in (ONE, GENEROUS):
        got, info = _agree(tools, enc, queries, 1 * scores[0], scores, cut_depth=cut_depth)
        letters = int((enc < 4).sum())
        # T = match: a start position matches a query as soon as its first letter occurs in it
        assert (got[:, 0] == 0).sum() == int((enc == 0).sum()) and (got[:, 0] == 2).sum() == 0
        assert (got[:, 0] == 3).sum() == letters and info["cut_depth"] == {locali.AUTO: 6}.get(cut_depth, cut_depth)
        for m in (2, 3):
            some = [q for q in queries if q.size == m]
            got, _ = _agree(tools, enc, some, m * scores[0], scores, cut_depth=cut_depth)
            assert (got[:, 0] == 0).sum() == _occurrences(enc, some[0]) > 0 and (got[:, 0] == 2).sum() == 0


# ---- 3: the width of a child ----

def _exact_walk(enc, query):
    """(levels pushed, children examined, rows finished alone, the strings that were
    levels) of the walk from one root when a mismatch or a gap costs more than the
    whole query gives and T = m: a column has a cell > 0 exactly while the letters
    taken are a piece of the query, and its largest cell is their number.  enc holds
    letters only, so a string has as many rows as occurrences."""
    text, q, m = bytes(enc), bytes(query), len(query)
    rows = {}
    for d in range(1, m + 2):
        for at in range(len(text) - d + 1):
            w = text[at:at + d]
            if d == 1 or w[:-1] in q:
                rows[w] = rows.get(w, 0) + 1
    levels, children, alone, todo = [], 0, 0, [b""]
    while todo:
        s = todo.pop()
        for c in range(4):
            w = s + bytes([c])
            width = rows.get(w, 0)
            if width == 0:
                continue
            children += 1
            if width == 1:
                alone += 1
            elif w in q and len(w) < m:
                levels.append(w)
                todo.append(w)
    return len(levels), children, alone, levels


@pytest.mark.parametrize("eleven", [1, 2, 64, 65])
def test_width_of_a_live_child(tools, eleven):
    """UNIT[:11] occurs in 1, 2, 64 and 65 rows, of which 0, 1, 30 and 30 go on with
    UNIT[11].  Under match 1, mismatch and gapextend -12 and T = 12 the walk from one
    root is that of the pieces of UNIT (_exact_walk): a child of one row goes on
    alone, a wider one whose letters are a piece of UNIT is a level -- UNIT[:11]
    among them but where it is one row -- and the figures of the walk say so."""
    full = {1: 0, 2: 1}.get(eleven, 30)
    enc = _copies(full, eleven - full, 70)
    widths = [_occurrences(enc, UNIT[:d]) for d in range(13)]
    assert widths[11] == eleven and widths[12] == full and min(widths[1:11]) > 64
    tools["aligner"].set_index_packed(_open(tools, enc))
    got, info = _agree(tools, enc, [UNIT], 12, (1, -12, -12), cut_depth=0)
    levels, children, alone, which = _exact_walk(enc, UNIT)
    assert got.shape[0] == full and (bytes(UNIT[:11]) in which) == (eleven > 1) and bytes(UNIT[:10]) in which
    assert (info["levels_pushed"], info["children_examined"], info["single_walks"]) == (levels, children, alone)
    assert info["jobs_finished_alone"] == 0 and levels >= 10 and alone >= (eleven == 1)
    _agree(tools, enc, [UNIT, UNIT[:11], _edited(UNIT, 1, 4)], 9, ONE)
    _agree(tools, enc, [UNIT, _edited(UNIT, 2, 5)], 8, GENEROUS, esa_too=True)


@pytest.mark.parametrize("occurrences", [1, 63, 64, 65, 129])
def test_width_of_the_successful_child(tools, occurrences):
    """the 12-mer occurs 1, 63, 64, 65 and 129 times: the batches of the locate.  In a
    run of one letter and as copies in contexts of their own; with T below 12 wider
    children succeed, with T = 14 none of these"""
    unit = np.zeros(12, dtype=np.uint8)
    for enc, word in ((_run_of(occurrences), unit), (_copies(occurrences), UNIT)):
        assert _occurrences(enc, word) == occurrences
        tools["aligner"].set_index_packed(_open(tools, enc))
        for cut_depth in (0, locali.AUTO):
            got, _ = _agree(tools, enc, [word, _edited(word, 1, 3)], 12, ONE, cut_depth=cut_depth)
            assert (got[:, 0] == 0).sum() >= occurrences
        _agree(tools, enc, [word, word[:11]], 9, ONE)
        _agree(tools, enc, [word], 14, ONE)
        got, _ = _agree(tools, enc, [word], 22, (2, -3, -2), capacity=LEAST)
        assert got.shape[0] >= occurrences


def test_levels_stay_wide_down_to_the_last_depth(tools):
    enc = np.zeros(500, dtype=np.uint8)
    tools["aligner"].set_index_packed(_open(tools, enc))
    for m in (63, 65):
        got, info = _agree(tools, enc, [np.zeros(m, dtype=np.uint8)], m - 2, ONE, cut_depth=0)
        # A^d has 501 - d > 64 rows at every depth d below the successful one, m - 2
        assert got.shape[0] == 500 - (m - 2) + 1 and info["levels_pushed"] == m - 3 and info["single_walks"] == 0
    assert _agree(tools, enc, [np.zeros(1, dtype=np.uint8), np.ones(1, dtype=np.uint8)], 1)[0].shape[0] == 500


# ---- 4: the ends of the text and the specials ----

def test_ends_and_specials(tools):
    enc = _random(3000, 4, 41)
    enc[700:705] = WILDCARD
    enc[1800] = WILDCARD
    enc[[1200, 1201, 2500]] = SEPARATOR
    n = enc.size
    queries = [_cut(enc, 1188, 12),          # ends on the last letter before the separators at 1200
               _cut(enc, 1189, 12),          # one letter before T is reached it runs into them: no match at 1189
               _cut(enc, 690, 16),           # runs into the wildcards at 700
               _cut(enc, n - 10, 10),        # ends on the last letter of the subject
               _cut(enc, 0, 11),             # begins at position 0
               _cut(enc, 1202, 9)]           # starts behind a separator
    queries[1][11] = (queries[1][10] + 1) % 4
    tools["aligner"].set_index_packed(_open(tools, enc))
    for T in (12, 10, 9, 5):
        got, _ = _agree(tools, enc, queries, T, ONE, esa_too=T == 9)
        _, dbstart, dblen, _, _, _ = locali.unpack(got)
        if T == 12:
            assert ((got[:, 0] == 0) & (dbstart == 1188) & (dblen == 12)).any()
            assert not ((got[:, 0] == 1) & (dbstart == 1189)).any()
        if T == 10:
            assert ((got[:, 0] == 3) & (dbstart == n - 10) & (dblen == 10)).any()
            assert ((got[:, 0] == 4) & (dbstart == 0) & (dblen == 10)).any()
    for seed, size in ((3, 2000), (4, 37), (5, 9)):
        enc = _with_specials(size, 4, seed)          # specials at both ends, in the middle and scattered
        tools["aligner"].set_index_packed(_open(tools, enc))
        for T in (1, 4, 8):
            _agree(tools, enc, _mixed_queries(enc, 6, seed, lengths=(3, 8, 13, 20)) + [_cut(enc, 1, 6)], T, ONE)


def test_subjects_shorter_than_the_query_and_subjects_of_specials(tools):
    query = _random(40, 4, 3)
    for enc in (_random(10, 4, 1), _random(1, 4, 2), np.array([WILDCARD, SEPARATOR] * 20, dtype=np.uint8),
                np.array([SEPARATOR], dtype=np.uint8)):
        tools["aligner"].set_index_packed(_open(tools, enc))
        for T in (1, 3):
            _agree(tools, enc, [query, query[:2]], T, ONE, esa_too=True)


# ---- 5: the stack ----

def test_the_smallest_stack(tools):
    """the smallest stack holds the root alone, so every child is finished row by row"""
    enc = _with_specials(3000, 4, 41)
    queries = _mixed_queries(enc, 4, 7) + [_cut(enc, 100, 129)]
    tools["aligner"].set_index_packed(_open(tools, enc))
    for stack_words in (STACK, STACK + 70, 700):
        got, info = _agree(tools, enc, queries, 12, stack_words=stack_words, cut_depth=1)
        assert got.shape[0] > 4 and info["stack_words"] == stack_words
        assert info["jobs_finished_alone"] > 0 and info["single_walks"] > 1000
        if stack_words == STACK:
            assert info["levels_pushed"] == 0
    roomy = _agree(tools, enc, queries, 12, cut_depth=1)[1]
    assert roomy["jobs_finished_alone"] == 0 and roomy["levels_pushed"] > 0


@pytest.mark.parametrize("cut_depth", [0, 1])
def test_the_default_stack_runs_out_by_itself(tools, cut_depth):
    """The subject holds a piece of 120 letters twice and the query of 129 letters
    begins with it; T = 200 is reached 100 letters down the path the two copies
    share, and with match 2, mismatch -1, gapextend -1 nearly every row of a column
    is > 0, so a level takes some m words: the default stack, 32 columns and 4096
    words, is full long before, and the children from there on are finished row by
    row.  A stack of 2^20 words holds the whole path and gives the same records."""
    rng = np.random.default_rng(44)
    piece = rng.integers(0, 4, 120, dtype=np.uint8)
    enc = np.concatenate([rng.integers(0, 4, 100), piece, [0], rng.integers(0, 4, 100), piece, [1],
                          rng.integers(0, 4, 50)]).astype(np.uint8)
    query = np.concatenate([piece, _random(9, 4, 46)])
    tools["aligner"].set_index_packed(_open(tools, enc))
    got, info = _agree(tools, enc, [query], 200, GENEROUS, cut_depth=cut_depth)
    assert info["stack_words"] == 32 * 192 + 4096 and info["jobs_finished_alone"] > 0 and info["levels_pushed"] > 50
    _, dbstart, dblen, _, _, _ = locali.unpack(got)
    for at in (100, 100 + 120 + 1 + 100):
        assert ((dbstart == at) & (dblen == 100)).any()
    wide, info = _agree(tools, enc, [query], 200, GENEROUS, stack_words=1 << 20, cut_depth=cut_depth)
    assert info["stack_words"] == 1 << 20 and info["jobs_finished_alone"] == 0 and np.array_equal(wide, got)


# ---- 6: long queries ----

def test_query_lengths_around_the_chunks(tools):
    """queries of 65, 129, 193 and 1000 letters, cut from the subject, with one
    replacement and one deletion: columns of two to sixteen chunks"""
    enc = _random(1500, 4, 41)
    queries = []
    for k, m in enumerate((65, 129, 193, 1000)):
        query = _cut(enc, 40 + 61 * k, m + 1)
        query[m // 3] = (query[m // 3] + 1) % 4
        queries.append(np.delete(query, 2 * m // 3))
    tools["aligner"].set_index_packed(_open(tools, enc))
    got, info = _agree(tools, enc, queries, 30, STRICT, esa_too=True)
    number, _, _, _, qstart, qlen = locali.unpack(got)
    assert [q.size for q in queries] == [65, 129, 193, 1000] and info["levels_pushed"] > 0
    assert all((number == k).any() for k in range(4)) and ((number == 3) & (qstart + qlen > 900)).any()


def test_the_longest_query(tools):
    """LONGEST letters over a, c, g with match 1; the subject holds one piece of it
    once, with a replacement and a deletion, between runs of t, which the query
    lacks: the start positions outside the piece end with their first column, so the
    reference has the ten or so columns of the piece alone to compute"""
    query = _random(LONGEST, 3, 47)
    piece = np.delete(query[9000:9060].copy(), 40)
    piece[20] = 3
    enc = np.concatenate([np.full(100, 3), piece, [SEPARATOR], np.full(50, 3)]).astype(np.uint8)
    tools["aligner"].set_index_packed(_open(tools, enc))
    got, info = _agree(tools, enc, [query, query[:5].copy()], 10, STRICT, esa_too=True)
    number, dbstart, dblen, _, qstart, _ = locali.unpack(got)
    assert LONGEST == 16384 and info["stack_words"] == 32 * LONGEST + 4096
    assert ((number == 0) & (dbstart == 100) & (dblen == 10) & (qstart == 9000)).any()


# ---- 7: locate flavours ----

FLAVOURS = [SUITE, dict(), dict(locbitmap=True), dict(locfreq=1, sprank=True), dict(locfreq=7, locbitmap=True, sprank=True),
            dict(locfreq=0)]


@pytest.mark.parametrize("kw", FLAVOURS, ids=lambda kw: "-".join("%s%s" % (k[:3], int(v)) for k, v in kw.items()) or "defaults")
def test_locate_flavours(tools, kw):
    """the suite's image, the defaults, a bitmap of the marked rows, every row marked;
    the second and the third without stored ranks, on a subject with
    wildcards; and an image without locate information"""
    enc = _with_specials(2500, 4, 13)
    queries = _mixed_queries(enc, 8, 3)
    reader = _open(tools, enc, kw=kw)
    assert reader.info()["locate_interval"] == kw.get("locfreq", 16)
    tools["aligner"].set_index_packed(reader)
    want = _brute(enc, queries, STRICT, 8)
    assert want.shape[0] > 20
    if kw.get("locfreq", 16):
        _agree(tools, enc, queries, 8)
        return
    # no locate information: the counts are there, the records are not
    info = tools["aligner"].prepare(queries, 8, *STRICT)
    assert info["matches"] == want.shape[0]
    assert info["max_matches_of_one_job"] <= np.bincount(want[:, 0].astype(np.int64)).max()
    with pytest.raises(_lib.EsaError, match="no locate information"):
        list(tools["aligner"].records())
    assert tools["aligner"].info()["emitted"] == 0


# ---- 8: lines and counter rows ----

@pytest.mark.parametrize("rows", [191, 192, 193, 16383, 16385])
def test_line_borders(tools, rows):
    """bounds in one line, in two lines, a flagged line, the tile border of the decode"""
    enc = _with_specials(rows - 1, 4, rows)
    tools["aligner"].set_index_packed(_open(tools, enc))
    for T, scores in ((7, STRICT), (10, ONE)):
        got, _ = _agree(tools, enc, _mixed_queries(enc, 8, rows + T, lengths=(8, 13, 20, 31)), T, scores)
        assert got.shape[0] > 0


@pytest.mark.parametrize("sigma", [5, 20])
@pytest.mark.parametrize("rows", [64, 65, 129, 4000])
def test_byte_rows_and_their_counter_blocks(tools, sigma, rows):
    enc = _with_specials(rows - 1, sigma, rows + sigma)
    tools["aligner"].set_index_packed(_open(tools, enc, sigma=sigma))
    queries = _mixed_queries(enc, 8, rows, sigma, lengths=(3, 5, 8, 13, 20))
    for T, cut_depth in ((3, locali.AUTO), (5, 1)):
        got, _ = _agree(tools, enc, queries, T, ONE, sigma, cut_depth=cut_depth)
        assert got.shape[0] > 0


# ---- 9: windows ----

def _window_cases():
    run = np.zeros(4000, dtype=np.uint8)
    yield run, [np.zeros(12, dtype=np.uint8), np.zeros(5, dtype=np.uint8)], 5, ONE, 0
    enc = _with_specials(3000, 4, 41)
    yield enc, _mixed_queries(enc, 12, 3), 4, STRICT, locali.AUTO


@pytest.mark.parametrize("case", [0, 1])
def test_pieces_of_any_capacity_and_any_cursor(tools, case):
    enc, queries, T, scores, cut_depth = list(_window_cases())[case]
    aligner = tools["aligner"]
    aligner.set_index_packed(_open(tools, enc))
    _agree(tools, enc, queries, T, scores, cut_depth=cut_depth)
    aligner.set_limits(0, cut_depth)
    info = aligner.prepare(queries, T, *scores)
    aligner.set_limits()
    whole = np.concatenate(list(aligner.records()))
    assert whole.shape[0] == info["matches"] > 2000
    assert np.array_equal(np.concatenate(list(aligner.records())), whole)       # two full enumerations
    assert LEAST < 65
    for capacity in (LEAST, 65, 1000):
        chunks = list(aligner.records(capacity))
        assert [c.shape[0] for c in chunks[:-1]] == [capacity] * (len(chunks) - 1) and len(chunks) > 2
        assert np.array_equal(np.concatenate(chunks), whole), capacity
    # a cursor in the middle of the query with the most records, one on its first record, the end
    number = np.bincount(whole[:, 0].astype(np.int64)).argmax()
    first = int(np.flatnonzero(whole[:, 0] == number)[0])
    many = int((whole[:, 0] == number).sum())
    for capacity in (LEAST, 65, 1000):
        for cursor in (0, first + many // 2, first + 1, first, whole.shape[0] // 2, whole.shape[0] - 1):
            piece = next(aligner.records(capacity, cursor=cursor))
            assert np.array_equal(piece, whole[cursor:cursor + capacity]), (capacity, cursor)
        assert list(aligner.records(capacity, cursor=whole.shape[0])) == []
    with pytest.raises(_lib.EsaError, match="cursor %d is not one of this enumeration" % (whole.shape[0] + 1)):
        list(aligner.records(100, cursor=whole.shape[0] + 1))
    with pytest.raises(_lib.EsaError, match="at least %d" % LEAST):
        list(aligner.records(LEAST - 1))
    import torch
    chunks = [c.cpu().numpy().copy() for c in aligner.records(1000, device=True)]
    torch.cuda.synchronize()
    assert np.array_equal(np.concatenate(chunks).astype(np.uint64), whole)


# ---- 10: refusals and replacement ----

def test_refusals(tools):
    enc = _with_specials(2000, 4, 3)
    query = _cut(enc, 5, 12)
    with locali.LocalAlignments() as f, pck.PackedIndexReader() as closed:
        with pytest.raises(_lib.EsaError, match="packed index reader has no image open"):
            f.set_index_packed(closed)
        with pytest.raises(_lib.EsaError, match="no index is set"):
            f.prepare([query], 5)
        reader = _open(tools, enc)
        raw = tools["builder"].image()
        f.set_index_packed(reader)
        with pytest.raises(_lib.EsaError, match="nothing is prepared"):
            list(f.records())
        want = _brute(enc, [query], STRICT, 9)
        assert want.shape[0] >= 1 and np.array_equal(_sorted(f.all_records([query], 9, *STRICT)), want)
        with pytest.raises(_lib.EsaError, match="neither a letter of the alphabet of 4 letters nor the wildcard"):
            f.prepare([np.array([0, 1, 255, 2], dtype=np.uint8)], 5)
        # the reader loses its image: refused until it holds one again
        f.prepare([query], 9, *STRICT)
        with pytest.raises(_lib.EsaError, match="packed index reader: "):
            reader.open(raw[:-1])
        with pytest.raises(_lib.EsaError, match="no image open any more"):
            f.prepare([query], 9, *STRICT)
        with pytest.raises(_lib.EsaError, match="no image open any more"):
            list(f.records())
        with pytest.raises(_lib.EsaError, match="packed index reader has no image open"):
            f.set_index_packed(reader)
        reader.open(raw)
        assert np.array_equal(_sorted(f.all_records([query], 9, *STRICT)), want)
        # the reader is opened on another image: what was prepared is not of it, a new prepare is
        other = _with_specials(700, 4, 5)
        _open(tools, other)
        with pytest.raises(_lib.EsaError, match="opened again since gtamd_locali_prepare"):
            list(f.records())
        again = _brute(other, [query], STRICT, 4)
        assert again.shape[0] >= 1 and np.array_equal(_sorted(f.all_records([query], 4, *STRICT)), again)


def test_switching_between_a_suffix_table_and_a_packed_index(tools):
    """on one object, in both directions: the records of the suffix table in its
    order, those of the packed index sorted, right each time"""
    enc = _random(600, 4, 41)
    enc[70:72] = WILDCARD
    enc[120] = SEPARATOR
    suf = ou.esa(enc, 4)["suf"]
    queries = [_cut(enc, 20, 9), _random(7, 4, 5), _edited(_cut(enc, 100, 30), 2, 1)]
    want = lr.records(enc, suf, queries, *ONE, T=6)
    assert want.shape[0] > 20
    aligner = tools["aligner"]
    reader = _open(tools, enc)
    for _ in range(2):
        aligner.set_index_packed(reader)
        assert np.array_equal(_sorted(aligner.all_records(queries, 6, *ONE)), _sorted(want))
        aligner.set_index(enc, suf)
        assert np.array_equal(aligner.all_records(queries, 6, *ONE), want)


def test_a_reader_opened_from_the_builder_and_one_from_the_host_image(tools):
    enc = _with_specials(5000, 4, 77)
    queries = _mixed_queries(enc, 10, 5)
    aligner = tools["aligner"]
    aligner.set_index_packed(_open(tools, enc))
    first = aligner.all_records(queries, 8, *STRICT)
    aligner.set_index_packed(_open(tools, enc, which="second", host=True))
    assert first.shape[0] > 30 and np.array_equal(aligner.all_records(queries, 8, *STRICT), first)


def test_an_image_the_reference_wrote(tools):
    """tests/golden/pcktagmatch/trna_glutamine.bdx, written by `gt packedindex mkindex
    ... -dir rev`: the records of the -esa path on trna_glutamine.fna"""
    enc, queries = _fixture("trna_glutamine.fna")
    with open(os.path.join(ou.GOLDEN_DIR, "pcktagmatch", "trna_glutamine.bdx"), "rb") as f:
        tools["second"].open(f.read())
    tools["aligner"].set_index_packed(tools["second"])
    total = 0
    for T, scores in ((14, (1, -3, -2)), (25, (1, -3, -2)), (30, GENEROUS)):
        got = _sorted(tools["aligner"].all_records(queries, T, *scores))
        _same(got, _esa_path(tools, enc, 4, queries, scores, T))
        _same(got, _brute(enc, queries, scores, T))
        total += got.shape[0]
    assert total > 20


# ---- 11: against the aligner on the suffix table ----

def test_against_the_aligner_on_the_suffix_table(tools):
    """2^20 random symbols in which eight pieces of 60 letters are planted four times
    each, edited; the eight pieces as queries"""
    import torch
    n = 1 << 20
    enc = _random(n, 4, 2026)
    rng = np.random.default_rng(8)
    queries = []
    for k in range(8):
        piece = _random(60, 4, 100 + k)
        queries.append(piece)
        for c in range(4):
            copy = _edited(piece, c, 1000 + 4 * k + c)
            at = int(rng.integers(0, n - 100))
            enc[at:at + copy.size] = copy
    dev = torch.from_numpy(enc).to("cuda:0")
    with esa.EsaEngine(n, 4) as eng:
        eng.set_sequence_device(dev.data_ptr(), n)
        eng.run(esa.WANT_SUF)
        tools["plain"].set_index_engine(eng, dev.data_ptr(), n)
        want = tools["plain"].all_records(queries, 24, 1, -3, -2)
    tools["aligner"].set_index_packed(_open(tools, enc))
    got = tools["aligner"].all_records(queries, 24, 1, -3, -2)
    assert want.shape[0] >= 32 and np.array_equal(_sorted(got), _sorted(want))
    assert np.array_equal(got[:, 0], want[:, 0])
