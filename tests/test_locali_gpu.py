"""Local alignments on the device (include/gtamd_locali.h,
genometools_amd/locali.py) against the statement per suffix of
tests/locali_reference.py: every record, none sampled, in the order of the
header.  The subjects have a few thousand symbols at most, so that the
reference, which knows no table, no band and no chunk, is the judge.

The shapes are the smallest at which each part can go wrong: a column is
computed 64 rows a step (queries of 63, 64, 65, 127, 128, 129 letters), the
shared search probes 64 places a round and a successful child is given 64
suffixes at a time (children of 1, 2, 64 and 65 suffixes), a workgroup has WAVES
waves, an emit call takes at least LEAST records, a stack of STACK words holds
the root of a walk alone.

Beyond 129 letters: queries of 191, 192, 193, 320 and 1000 letters (columns of
up to sixteen chunks, bands far from row 1); two copies of a piece under
generous scores, for which the default stack runs out by itself at some
depth and the rest of the path is finished suffix by suffix; the longest
query there is, LONGEST letters, with matches that begin in row 0 and above
row 16000; exact copies that score all but the whole 16 bits of a cell; a
child of more than 64 * 64 suffixes."""
import functools

import numpy as np
import pytest

import locali_reference as lr
import oracle_util as ou
from genometools_amd import _lib, esa, locali

pytestmark = pytest.mark.gpu

WAVES, LEAST, LONGEST, STACK = locali.geometry()
WIDTHS = [np.uint64, np.uint32]
ONE = (1, -1, -1)
STRICT = (1, -2, -2)          # random alignments die early: the reference stays quick
TAIL = np.array([3, 0, 3, 3, 1, 3, 2, 3, 3, 0, 1, 3], dtype=np.uint8)      # the end of the longest query


@pytest.fixture(scope="module")
def aligner(gpu):
    with locali.LocalAlignments() as f:
        yield f


def _random(n, sigma, seed):
    return np.random.default_rng(seed).integers(0, sigma, n, dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def _subject(name):
    """(enc, suf, sigma) of a named subject; shared, never written to"""
    kind, _, arg = name.partition(":")
    sigma = 4
    if kind == "random":                 # two wildcard runs, separators, a letter at n - 1
        enc = _random(int(arg), 4, 41)
        if enc.size > 2600:
            enc[700:705] = 254
            enc[1800:1801] = 254
            for at in (1200, 1201, 2500):
                enc[at:at + 1] = 255
    elif kind == "binary":
        enc, sigma = _random(int(arg), 2, 42), 2
        enc[[150, 151]] = 254
        enc[400] = 255
    elif kind == "protein":
        enc, sigma = _random(int(arg), 20, 43), 20
        enc[[300, 301]] = 254
        enc[900] = 255
    elif kind == "copies":               # w copies of one 12-mer, each in a context of its own
        rng = np.random.default_rng(int(arg))
        unit = np.array([3, 3, 0, 1, 2, 3, 0, 0, 1, 3, 2, 2], dtype=np.uint8)
        enc = np.concatenate([np.concatenate([unit, rng.integers(0, 3, 19, dtype=np.uint8), [k % 3]])
                              for k in range(int(arg))]).astype(np.uint8)
    elif kind == "short":                # sequences of 1 to 6 letters between separators, and some wildcards
        rng = np.random.default_rng(int(arg))
        parts = []
        for k in range(int(arg)):
            parts += [rng.integers(0, 4, 1 + k % 6, dtype=np.uint8), [254 if k % 11 == 3 else 255]]
        enc = np.concatenate(parts).astype(np.uint8)[:-1]
    elif kind == "run":
        enc = np.zeros(int(arg), dtype=np.uint8)
    elif kind == "twice":                # two copies of one piece of `arg` letters, an a behind one and a c behind the other
        rng = np.random.default_rng(44)
        piece = rng.integers(0, 4, int(arg), dtype=np.uint8)
        enc = np.concatenate([rng.integers(0, 4, 100), piece, [0], rng.integers(0, 4, 100), piece, [1],
                              rng.integers(0, 4, 50)]).astype(np.uint8)
    elif kind == "tiny":                 # 28 symbols: TAIL whole in one sequence, its first 7 letters in the other
        enc = np.concatenate([_random(5, 3, 45), TAIL, [255], TAIL[:7], [1, 3, 3]]).astype(np.uint8)
    elif kind == "specials":
        enc = np.full(int(arg), 254, dtype=np.uint8)
        enc[::7] = 255
    else:
        raise ValueError(name)
    enc = enc.copy()
    suf = ou.esa(enc, sigma)["suf"]
    enc.setflags(write=False)
    suf.setflags(write=False)
    return enc, suf, sigma


@functools.lru_cache(maxsize=None)
def _reference(name, query, scores, T):
    """the records of one query (as bytes) with query number 0; shared"""
    enc, suf, _ = _subject(name)
    rec = lr.records(enc, suf, [np.frombuffer(query, dtype=np.uint8)], *scores, T=T)
    rec.setflags(write=False)
    return rec


def _expected(name, queries, scores, T):
    parts = []
    for number, query in enumerate(queries):
        rec = _reference(name, np.ascontiguousarray(query, dtype=np.uint8).tobytes(), tuple(scores), T).copy()
        rec[:, 0] = number
        parts.append(rec)
    return np.concatenate(parts) if parts else np.zeros((0, 4), dtype=np.uint64)


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


def _cut(enc, at, m):
    query = enc[at:at + m].copy()
    query[query >= 254] = 1
    return query


def _agree(aligner, name, queries, T, scores=STRICT, width=np.uint64, capacity=locali.DEFAULT_CAPACITY, set_index=True,
           stack_words=0, cut_depth=locali.AUTO):
    enc, suf, sigma = _subject(name)
    if set_index:
        aligner.set_index(enc, suf.astype(width), sigma)
    aligner.set_limits(stack_words, cut_depth)
    want = _expected(name, queries, scores, T)
    got = aligner.all_records(queries, T, *scores, capacity=capacity)
    aligner.set_limits()
    assert got.dtype == np.uint64 and got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(got, want)
    info = aligner.info()
    assert info["jobs"] == len(queries) * info["groups"] and info["matches"] == info["emitted"] == want.shape[0]
    assert info["max_matches_of_one_job"] <= max(np.bincount(want[:, 0].astype(np.int64)).max() if want.size else 0, 0)
    return want, info


def _device_copy(a, skew):
    import torch
    t = torch.empty(a.nbytes + 64, dtype=torch.uint8, device="cuda:0")
    t[skew:skew + a.nbytes] = torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to("cuda:0")
    torch.cuda.synchronize()
    return t, t.data_ptr() + skew


def _mixed_queries(enc, count, seed, sigma=4):
    rng = np.random.default_rng(seed)
    queries = []
    for k in range(count):
        m = int(rng.choice([8, 13, 20, 31, 40, 64, 90]))
        query = _cut(enc, int(rng.integers(0, enc.size - m)), m)
        if k % 3:
            query = _edited(query, 1 + k % 4, seed + k, sigma)
        queries.append(query)
    return queries


# ---- index sources and widths ----

@pytest.mark.parametrize("width", WIDTHS)
def test_index_in_host_memory(aligner, width):
    enc = _subject("random:3000")[0]
    want, info = _agree(aligner, "random:3000", _mixed_queries(enc, 10, 1), 10, width=width)
    assert want.shape[0] > 10 and info["levels_pushed"] > 0 and info["single_walks"] > 0


@pytest.mark.parametrize("width", WIDTHS)
def test_index_queries_and_records_in_device_memory(aligner, width):
    enc, suf, _ = _subject("random:3000")
    queries = _mixed_queries(enc, 6, 2)
    symbols, offsets = locali.pack_queries(queries)
    for skew in (0, 3):
        keep = [_device_copy(enc, skew), _device_copy(suf.astype(width), 8), _device_copy(symbols, skew + 1),
                _device_copy(offsets, 16)]
        aligner.set_index_device(keep[0][1], enc.size, keep[1][1], np.dtype(width).itemsize)
        aligner.prepare_device(keep[2][1], keep[3][1], len(queries), 8, *STRICT)
        chunks = [c.cpu().numpy().copy() for c in aligner.records(LEAST, device=True)]
        got = np.concatenate(chunks).astype(np.uint64)
        assert np.array_equal(got, _expected("random:3000", queries, STRICT, 8)) and got.shape[0] > LEAST
        del keep


def test_index_from_a_live_engine(aligner):
    enc, suf, sigma = _subject("random:3000")
    queries = _mixed_queries(enc, 5, 3)
    want = _expected("random:3000", queries, STRICT, 10)
    with esa.EsaEngine(enc.size, sigma) as eng:
        eng.set_sequence(enc)
        eng.run(esa.WANT_SUF)
        dev = _device_copy(enc, 0)
        aligner.set_index_engine(eng, dev[1], enc.size)
        got = aligner.all_records(queries, 10, *STRICT)
        assert np.array_equal(got, want) and got.shape[0] > 5
        with pytest.raises(_lib.EsaError, match="not the whole table"):
            aligner.set_index_engine(eng, dev[1], enc.size - 1)


# ---- the column: the cases of the core test through the walk ----

@pytest.mark.parametrize("scores", [ONE, (2, -1, -1), (3, -2, -2), (5, -3, -1), (1, -2, -3)])
def test_query_lengths_around_the_chunks(aligner, scores):
    """queries of every length at which the chunks of a column change, cut from
    the subject and edited, one with a wildcard; a threshold that most of a query
    reaches, so that walks go deep, and two letters, so that equal candidates abound"""
    enc = _subject("binary:600")[0]
    queries = []
    for k, m in enumerate((1, 2, 63, 64, 65, 127, 128, 129)):
        query = _edited(_cut(enc, 17 * k + 5, m), m // 20, k, 2) if m > 2 else _cut(enc, 5, m)
        if m == 65:
            query[30] = 254
        queries.append(query)
    want, _ = _agree(aligner, "binary:600", queries, 24 * scores[0], scores)
    assert want.shape[0] > 100
    short = [q for q in queries if q.size <= 2]
    assert _agree(aligner, "binary:600", short, scores[0], scores, set_index=False)[0].shape[0] > 300     # depth 1
    assert _agree(aligner, "binary:600", short, 2 * scores[0], scores, set_index=False)[0].shape[0] > 50


def test_a_delete_run_across_the_chunks(aligner):
    """one letter of the query matches in row 60 (and in row 63); with a cheap gap
    the Delete chain runs down through rows 64 and 65, and T is reached there"""
    enc = _subject("random:300")[0]
    for row, match, second, T in ((60, 10, 65, 12), (63, 4, 66, 6)):
        query = np.zeros(129, dtype=np.uint8)
        query[:] = 254
        query[row - 1] = enc[100]
        query[second - 1] = enc[101]         # ... a Replace on top of the chain, where it is still > 0
        want, _ = _agree(aligner, "random:300", [query], T, (match, -1, -1))
        low, high = np.uint64(0xffffffff), np.uint64(32)
        assert want.shape[0] > 0 and ((want[:, 3] & low) + (want[:, 3] >> high) > 64).any()


def test_the_deepest_walk(aligner):
    """match 5, gapextend -1, m = 4: four matches, then an insertion per column
    down to a score of 1 at depth 23, with T out of reach; and within reach at
    the last depth"""
    enc = np.concatenate([np.zeros(4, dtype=np.uint8), np.ones(40, dtype=np.uint8)])
    suf = ou.esa(enc, 4)["suf"]
    query = np.zeros(4, dtype=np.uint8)
    aligner.set_index(enc, suf)
    for T, count in ((21, 0), (20, 1)):
        got = aligner.all_records([query], T, 5, -3, -1)
        assert np.array_equal(got, lr.records(enc, suf, [query], 5, -3, -1, T)) and got.shape[0] == count
    assert lr.max_depth(4, 5, -1) == 23


# ---- queries beyond 129 letters ----

def _ceil64(m):
    return (m + 63) // 64 * 64


@pytest.mark.parametrize("width", WIDTHS)
def test_query_lengths_around_the_later_chunks(aligner, width):
    """queries of 191, 192, 193, 320 and 1000 letters, cut from the subject, with
    one replacement and one deletion: columns of three to sixteen chunks, bands
    that lie far from row 1.  The reference takes 0.45 s for a query of 192
    letters, 0.9 s for 320 and 4.1 s for 1000 (one core of the build machine)."""
    enc = _subject("random:1500")[0]
    queries = []
    for k, m in enumerate((191, 192, 193, 320, 1000)):
        query = _cut(enc, 40 + 61 * k, m + 1)
        query[m // 3] = (query[m // 3] + 1) % 4
        queries.append(np.delete(query, 2 * m // 3))
    want, info = _agree(aligner, "random:1500", queries, 30, STRICT, width=width)
    number, _, _, _, qstart, qlen = locali.unpack(want)
    assert [q.size for q in queries] == [191, 192, 193, 320, 1000] and info["levels_pushed"] > 0
    assert all((number == k).any() for k in range(5)) and ((number == 4) & (qstart + qlen > 900)).any()


@pytest.mark.parametrize("cut_depth", [0, 1])
@pytest.mark.parametrize("piece,m,scores", [(120, 129, (2, -1, -1)), (120, 192, (2, -1, -1)), (230, 260, ONE)])
def test_the_default_stack_runs_out_by_itself(aligner, piece, m, scores, cut_depth):
    """The subject holds a piece twice and the query begins with it; T = 200 is
    reached 200 / match symbols down the path the two copies share, and with
    these scores nearly every row of a column is > 0, so a level takes some m
    words.  The default stack, 32 columns and 4096 words, is full long before:
    the children from there on are finished suffix by suffix, without any
    set_limits.  A stack of 2^20 words holds the whole path and gives the same
    records.  The reference takes 1.7 s, 3.2 s and 6.1 s."""
    name = "twice:%d" % piece
    query = np.concatenate([_subject(name)[0][100:100 + piece], _random(m - piece, 4, 46)])
    want, info = _agree(aligner, name, [query], 200, scores, stack_words=0, cut_depth=cut_depth)
    assert info["stack_words"] == 32 * _ceil64(m) + 4096
    assert info["jobs_finished_alone"] > 0
    assert info["levels_pushed"] > 50
    _, dbstart, dblen, _, _, _ = locali.unpack(want)
    for at in (100, 100 + piece + 1 + 100):
        assert ((dbstart == at) & (dblen == 200 // scores[0])).any()
    info = _agree(aligner, name, [query], 200, scores, stack_words=1 << 20, cut_depth=cut_depth, set_index=False)[1]
    assert info["stack_words"] == 1 << 20 and info["jobs_finished_alone"] == 0
    # the device's own records of the two stacks, one against the other
    got = []
    for stack_words in (0, 1 << 20):
        aligner.set_limits(stack_words, cut_depth)
        got.append(aligner.all_records([query], 200, *scores))
    aligner.set_limits()
    assert np.array_equal(got[0], got[1]) and got[0].shape == want.shape


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("scores,T,count", [(ONE, 10, 4), ((3, -2, -1), 30, 8), ((3, -2, -2), 20, 13)])
def test_the_longest_query(aligner, scores, T, count, width):
    """LONGEST letters over a, c, g with the 12 letters of TAIL at the end and its
    first five as letters 5 to 9, behind the five letters the subject begins
    with, so that ten letters are equal and T = 10 is reached from row 0; the subject holds TAIL and its first seven letters, so matches begin in
    row 0 and in the last rows a cell can name.
    A second query of 5 letters follows in the same call: the columns are sized
    from the longest query, not from the last.  The statement finds 4, 8 and 13
    records, one of each from row 0 (four with the last scores: rows 0 to 3).
    The reference takes 4.6 to 8.1 s a
    threshold, shared by the two widths."""
    query = _random(LONGEST, 3, 47)
    query[-12:] = TAIL
    query[:5] = _subject("tiny")[0][:5]           # the subject begins as the query does: ten equal letters
    query[5:10] = TAIL[:5]
    queries = [query, TAIL[:5].copy()]
    want, info = _agree(aligner, "tiny", queries, T, scores, width=width)
    number, _, _, _, qstart, _ = locali.unpack(want)
    assert LONGEST == 16384 and info["stack_words"] == 32 * LONGEST + 4096 and want.shape[0] == count
    assert ((number == 0) & (qstart > 16000)).any() and ((number == 0) & (qstart < 16)).any()
    _agree(aligner, "tiny", queries, T, scores, capacity=LEAST, set_index=False)


@pytest.mark.parametrize("match,m", [(2047, 32), (1023, 64), (511, 128), (32767, 2)])
def test_the_top_of_a_cell(aligner, match, m):
    """exact copies that score 65504, 65472, 65408 and 65534, all but the whole
    16 bits of a cell, under a threshold equal to that, and under one above it,
    which nothing reaches.  The reference takes 0.03 to 1.6 s a call."""
    enc = _subject("random:300")[0]
    query = _cut(enc, 150, m)
    whole = match * m
    want, _ = _agree(aligner, "random:300", [query], whole, (match, -1, -1))
    _, dbstart, dblen, score, qstart, qlen = locali.unpack(want)
    assert 65400 < whole <= 65535 and want.shape[0] > 0 and (score == whole).all()
    assert ((dbstart == 150) & (dblen == m) & (qstart == 0) & (qlen == m)).any()
    assert _agree(aligner, "random:300", [query], whole + 1, (match, -1, -1), set_index=False)[0].shape[0] == 0


def test_a_child_wider_than_64_times_64(aligner):
    """A^4200 as one group: the child of the root has 4200 suffixes, more than two
    rounds of 64 probes tell apart, so the search for its right bound takes a third"""
    queries = [np.zeros(12, dtype=np.uint8), np.zeros(5, dtype=np.uint8)]
    want, info = _agree(aligner, "run:4200", queries, 5, ONE, cut_depth=0)
    assert info["groups"] == 1 and want.shape[0] == 2 * 4196 and info["max_matches_of_one_job"] == 4196


# ---- the width of a child ----

@pytest.mark.parametrize("copies", [1, 2, 64, 65])
def test_width_of_the_successful_child(aligner, copies):
    """the 12-mer occurs `copies` times: with T = 12 its interval at depth 12 is the
    successful child, that wide; with T = 9 shorter prefixes are, and with T = 14 none"""
    name = "copies:%d" % copies
    unit = _subject(name)[0][:12].copy()
    for T in (12, 9, 14):
        want, _ = _agree(aligner, name, [unit, _edited(unit, 1, 3)], T, ONE, set_index=T == 12)
        if T == 12:
            assert (want[:, 0] == 0).sum() >= copies
    want, _ = _agree(aligner, name, [unit], 22, (2, -3, -2), set_index=False)
    assert want.shape[0] >= copies


# ---- the cut of the table into groups ----

@pytest.mark.parametrize("cut_depth", [0, 1, 3, 16, locali.AUTO])
def test_sequences_shorter_than_the_cut_depth(aligner, cut_depth):
    """sequences of 1 to 6 letters: most suffixes end before the deepest cut, and a
    match at depth 2 or 3 takes suffixes of every length from there on"""
    enc = _subject("short:400")[0]
    queries = [np.array(q, dtype=np.uint8) for q in ([0, 1], [2, 2, 3], [1, 0, 3, 2, 1, 1], [3])]
    for T in (1, 2, 3, 5):
        want, info = _agree(aligner, "short:400", queries, T, ONE, set_index=T == 1, cut_depth=cut_depth)
        assert (want.shape[0] > 50) == (T < 5)
        if cut_depth != locali.AUTO:
            assert info["cut_depth"] == min(cut_depth, 8) and (info["groups"] == 1) == (cut_depth == 0)
    groups = info["groups"]
    assert cut_depth in (0, locali.AUTO) or groups > 4


def test_the_groups_of_every_cut_depth_give_the_same_records(aligner):
    enc = _subject("random:3000")[0]
    queries = _mixed_queries(enc, 5, 9)
    seen = []
    for q in range(0, 9):
        want, info = _agree(aligner, "random:3000", queries, 9, set_index=q == 0, cut_depth=q)
        seen.append(info["groups"])
    assert seen[0] == 1 and seen[1] == 5 and all(a <= b for a, b in zip(seen, seen[1:])) and seen[-1] > 1000


def test_one_query_and_a_thousand(aligner):
    """eight queries, each 125 times: the records of a query do not depend on how
    many there are, nor on the cut depth that their number chooses"""
    enc = _subject("random:3000")[0]
    eight = _mixed_queries(enc, 8, 4)
    want, info = _agree(aligner, "random:3000", eight[:1], 9)
    assert info["cut_depth"] > 3 and want.shape[0] > 0
    thousand = [eight[k % 8] for k in range(1000)]
    many, info = _agree(aligner, "random:3000", thousand, 9, set_index=False)
    assert info["cut_depth"] < 4 and 1000 % WAVES == 0
    assert np.array_equal(many[many[:, 0] == 0][:, 1:], want[:, 1:])
    assert np.array_equal(many[many[:, 0] == 992][:, 1:], want[:, 1:])
    assert _agree(aligner, "random:3000", thousand[:3], 9, set_index=False)[0].shape[0] > 0


def test_no_query(aligner):
    assert _agree(aligner, "random:3000", [], 5)[0].shape == (0, 4)
    assert list(aligner.records(LEAST)) == []


# ---- alphabets ----

def test_two_letters(aligner):
    enc = _subject("binary:600")[0]
    want, _ = _agree(aligner, "binary:600", _mixed_queries(enc, 8, 5, 2), 17, ONE)
    assert want.shape[0] > 8


def test_twenty_letters(aligner):
    enc = _subject("protein:2000")[0]
    queries = [_cut(enc, 100, 12), _edited(_cut(enc, 500, 30), 2, 1, 20), _cut(enc, 290, 14), _random(5, 20, 2),
               _cut(enc, 890, 25)]
    for T, scores in ((8, STRICT), (3, ONE), (15, (2, -1, -2))):
        want, info = _agree(aligner, "protein:2000", queries, T, scores, set_index=T == 8)
        assert want.shape[0] >= 4 and info["cut_depth"] == 3


# ---- the ends and the specials ----

def test_ends_and_specials(aligner):
    enc = _subject("random:3000")[0]
    n = enc.size
    queries = [_cut(enc, 1188, 12),          # ends on the last letter before the separators at 1200
               _cut(enc, 1190, 14),          # would have to pass them
               _cut(enc, 690, 16),           # runs into the wildcards at 700
               _cut(enc, n - 10, 10),        # ends at n - 1
               _cut(enc, 1202, 9)]           # starts behind a separator
    for T in (12, 9, 5):
        _agree(aligner, "random:3000", queries, T, ONE, set_index=T == 12)


def test_subject_shorter_than_the_query_and_subjects_of_specials(aligner):
    query = _random(40, 4, 3)
    for name in ("random:10", "random:1", "specials:50", "specials:1"):
        for T in (1, 3):
            _agree(aligner, name, [query, query[:2]], T)


# ---- emit in pieces ----

def test_pieces_of_any_capacity(aligner):
    """A^2000 and the queries A^12 and A^5 with T = 5: nearly every position matches,
    in one job when the table is one group; in pieces of the smallest capacity,
    of 1000 and in one"""
    queries = [np.zeros(12, dtype=np.uint8), np.zeros(5, dtype=np.uint8)]
    whole, info = _agree(aligner, "run:2000", queries, 5, ONE, cut_depth=0)
    assert info["max_matches_of_one_job"] == 1996 > 30 * LEAST and whole.shape[0] == 2 * 1996
    for capacity in (LEAST, 1000):
        aligner.prepare(queries, 5, *ONE)
        chunks = list(aligner.records(capacity))
        assert [c.shape[0] for c in chunks[:-1]] == [capacity] * (len(chunks) - 1)
        assert np.array_equal(np.concatenate(chunks), whole)
    with pytest.raises(_lib.EsaError, match="a capacity of %d records is too small: a capacity of at least %d"
                                            % (LEAST - 1, LEAST)):
        list(aligner.records(LEAST - 1))


def test_pieces_of_the_smallest_capacity_over_many_jobs(aligner):
    enc = _subject("random:3000")[0]
    queries = _mixed_queries(enc, 9, 6)
    want, _ = _agree(aligner, "random:3000", queries, 6, capacity=LEAST)
    assert want.shape[0] > 5 * LEAST


# ---- no silent loss ----

@pytest.mark.parametrize("stack_words", [STACK, STACK + 70, 700])
def test_a_stack_too_small_for_the_walk(aligner, stack_words):
    """the smallest stack holds the root alone, so every child is finished
    suffix by suffix in the text; a larger one runs out further down"""
    enc = _subject("random:3000")[0]
    queries = _mixed_queries(enc, 4, 7) + [_cut(enc, 100, 129)]
    want, info = _agree(aligner, "random:3000", queries, 12, stack_words=stack_words, cut_depth=1)
    assert want.shape[0] > 4 and info["stack_words"] == stack_words
    assert info["jobs_finished_alone"] > 0 and info["single_walks"] > 3000
    if stack_words == STACK:
        assert info["levels_pushed"] == 0 and info["jobs_finished_alone"] == info["jobs"] - len(queries)
    roomy = _agree(aligner, "random:3000", queries, 12, set_index=False, cut_depth=1)[1]
    assert roomy["jobs_finished_alone"] == 0 and roomy["levels_pushed"] > 0


# ---- tables that are not an index ----

@pytest.mark.parametrize("width", WIDTHS)
def test_tables_that_are_no_index(aligner, width):
    """plain data: the loop bounds of the walk make them harmless; the calls
    return, the records are unspecified"""
    enc = _subject("random:3000")[0]
    queries = _mixed_queries(enc, 6, 8) + [np.zeros(3, dtype=np.uint8)]
    top = np.iinfo(width).max
    shuffled = np.random.default_rng(1).permutation(enc.size + 1).astype(width)
    beyond = _subject("random:3000")[1].astype(width)
    beyond[::5] = top
    beyond[1::7] = enc.size + 3
    for suf in (shuffled, beyond, np.zeros(enc.size + 1, dtype=width), np.full(enc.size + 1, top, dtype=width)):
        aligner.set_index(enc, suf)
        for T in (3, 10):
            info = aligner.prepare(queries, T)
            total = sum(c.shape[0] for c in aligner.records(1000))
            assert total == info["matches"] <= len(queries) * (enc.size + 1)


# ---- what is refused ----

def test_refusals(gpu):
    enc, suf, _ = _subject("random:3000")
    query = _cut(enc, 5, 12)
    with locali.LocalAlignments() as f:
        with pytest.raises(_lib.EsaError, match="no index is set"):
            f.prepare([query], 5)
        with pytest.raises(_lib.EsaError, match="nothing is prepared"):
            list(f.records())
        with pytest.raises(_lib.EsaError, match="entries of 3 bytes, 4 or 8 expected"):
            f.set_index_device(1 << 20, 100, 1 << 21, 3)
        with pytest.raises(_lib.EsaError, match="beyond the limit of a single build"):
            f.set_index_device(1 << 20, (1 << 32) - 4096, 1 << 21, 8)
        with pytest.raises(_lib.EsaError, match="alphabet of 33 letters"):
            f.set_index(enc, suf, 33)
        f.set_index(enc, suf)
        for scores in ((0, -1, -1), (1, 0, -1), (1, -1, 0), (1, 1, -1), (-1, -1, -1), (40000, -1, -1), (1, -1, -40000)):
            with pytest.raises(_lib.EsaError, match="scores match %d, mismatch %d, gapextend %d; match must be in" % scores):
                f.prepare([query], 5, *scores)
        with pytest.raises(_lib.EsaError, match="a threshold of 0, at least 1 expected"):
            f.prepare([query], 0)
        with pytest.raises(_lib.EsaError, match="query number 1 of length %d; queries must not be longer than %d"
                                                % (LONGEST + 1, LONGEST)):
            f.prepare([query, _random(LONGEST + 1, 4, 1)], 5)
        with pytest.raises(_lib.EsaError, match="query number 2 of length 1024 with a match score of 64 can reach a score "
                                                "above 65535"):
            f.prepare([query, query, _random(1024, 4, 1)], 5, 64, -1, -1)
        with pytest.raises(_lib.EsaError, match="query number 0 is empty"):
            f.prepare([query[:0], query], 5)
        with pytest.raises(_lib.EsaError, match="neither a letter of the alphabet of 4 letters nor the wildcard"):
            f.prepare([np.array([0, 1, 255, 2], dtype=np.uint8)], 5)
        with pytest.raises(_lib.EsaError, match="neither a letter"):
            f.prepare([np.array([0, 4, 2], dtype=np.uint8)], 5)
        with pytest.raises(_lib.EsaError, match="a stack of %d words" % (STACK - 1)):
            f.set_limits(STACK - 1)
        with pytest.raises(_lib.EsaError, match="a cut depth of 17"):
            f.set_limits(0, 17)
        with pytest.raises(_lib.EsaError, match="nothing is prepared"):      # a refused prepare is none
            list(f.records())
        want = lr.records(enc, suf, [query], *STRICT, T=9)
        assert np.array_equal(f.all_records([query], 9, *STRICT), want) and want.shape[0] > 0
