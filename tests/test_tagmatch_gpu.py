"""Approximate matches of short tags on the device (include/gtamd_tagmatch.h,
genometools_amd/tagmatch.py) against the brute force of
tests/tagmatch_reference.py: every record, none sampled, in the order of the
header.  The subjects have at most a few thousand symbols, so that the brute
force, which knows no table, is the judge.

The shapes are the smallest at which each part can go wrong: the lanes of a wave
take 64 suffixes at once (a child of at most 64 suffixes is finished by single
walks, a wider one becomes a level; the shared search probes 64 places a round),
a workgroup takes WAVES jobs, an emit call at least LEAST records."""
import functools

import numpy as np
import pytest

import oracle_util as ou
import tagmatch_reference as tr
from genometools_amd import _lib, esa, tagmatch
from genometools_amd.tagmatch import BEST, FORWARD, REVCOMP, WITH_WILDCARDS

pytestmark = pytest.mark.gpu

WAVES, LEAST, LEVELS = tagmatch.geometry()
WIDTHS = [np.uint64, np.uint32]
BOTH = FORWARD | REVCOMP


@pytest.fixture(scope="module")
def matcher(gpu):
    with tagmatch.TagMatches() as f:
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
        enc[700:705] = 254
        enc[1800:1801] = 254
        for at in (1200, 1201, 2500):
            enc[at:at + 1] = 255
    elif kind == "run":                  # one letter
        enc = np.zeros(int(arg), dtype=np.uint8)
    elif kind == "tandem":               # acg acg acg ...
        enc = np.tile(np.array([0, 1, 2], dtype=np.uint8), int(arg) // 3 + 1)[:int(arg)]
    elif kind == "runof":                # t, then a run of A in which A^12 occurs `arg` times, then t and a tail
        enc = np.concatenate([[3], np.zeros(12 + int(arg) - 1, dtype=np.uint8), [3], _random(40, 3, 5) + 1]).astype(np.uint8)
    elif kind == "tandemof":             # the same with acg acg ...: (acg)^4 occurs `arg` times
        enc = np.concatenate([[3], np.tile(np.array([0, 1, 2], dtype=np.uint8), 4 + int(arg) - 1), [3],
                              _random(40, 4, 6)]).astype(np.uint8)
    elif kind == "copies":               # w copies of one 12-mer, each in a context of its own
        rng = np.random.default_rng(int(arg))
        unit = np.array([3, 3, 0, 1, 2, 3, 0, 0, 1, 3, 2, 2], dtype=np.uint8)
        enc = np.concatenate([np.concatenate([unit, rng.integers(0, 3, 19, dtype=np.uint8), [k % 3]])
                              for k in range(int(arg))]).astype(np.uint8)
    elif kind == "protein":
        enc, sigma = _random(int(arg), 20, 43), 20
        enc[[300, 301]] = 254
        enc[900] = 255
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


def _cut(enc, at, m):
    tag = enc[at:at + m].copy()
    tag[tag >= 254] = 1
    return tag


def _agree(matcher, name, tags, K, flags=BOTH, width=np.uint64, capacity=tagmatch.DEFAULT_CAPACITY, set_index=True):
    enc, suf, sigma = _subject(name)
    if set_index:
        matcher.set_index(enc, suf.astype(width), sigma)
    want, best = tr.expected(enc, suf, tags, K, flags)
    got = matcher.all_records(tags, K, flags, capacity)
    assert got.dtype == np.uint64 and got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(got, want)
    assert np.array_equal(matcher.best_k(), best)
    info = matcher.info()
    strands = 2 if flags & BOTH == BOTH else 1
    assert info["jobs"] == strands * len(tags) and info["matches"] == info["emitted"] == want.shape[0]
    per_job = np.bincount(want[:, 0].astype(np.int64)) if want.shape[0] else np.zeros(1, dtype=np.int64)
    assert info["max_matches_of_one_job"] == per_job.max()
    return want


# ---- index sources and widths ----

def _device_copy(a, skew):
    import torch
    t = torch.empty(a.nbytes + 64, dtype=torch.uint8, device="cuda:0")
    t[skew:skew + a.nbytes] = torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to("cuda:0")
    torch.cuda.synchronize()
    return t, t.data_ptr() + skew


def _mixed_tags(enc, count, seed):
    rng = np.random.default_rng(seed)
    tags = []
    for k in range(count):
        m = int(rng.choice([5, 8, 12, 13, 20, 31, 40, 63, 64]))
        at = int(rng.integers(0, enc.size - m))
        tag = _cut(enc, at, m)
        if k % 3 == 1:
            tag = _edited(tag, 1 + k % 2, seed + k)
        elif k % 3 == 2 and k % 2:
            tag = tr.revcomp(tag)
        tags.append(tag)
    return tags


@pytest.mark.parametrize("width", WIDTHS)
def test_index_in_host_memory(matcher, width):
    enc, _, _ = _subject("random:3000")
    want = _agree(matcher, "random:3000", _mixed_tags(enc, 40, 1), 2, width=width)
    assert want.shape[0] > 100


@pytest.mark.parametrize("width", WIDTHS)
def test_index_tags_and_records_in_device_memory(matcher, width):
    import torch
    enc, suf, _ = _subject("random:3000")
    tags = _mixed_tags(enc, 30, 2)
    want, _ = tr.expected(enc, suf, tags, 1)
    symbols, offsets = tagmatch.pack_tags(tags)
    for skew in (0, 3):
        keep = [_device_copy(enc, skew), _device_copy(suf.astype(width), 8), _device_copy(symbols, skew + 1),
                _device_copy(offsets, 16)]
        matcher.set_index_device(keep[0][1], enc.size, keep[1][1], np.dtype(width).itemsize)
        matcher.prepare_device(keep[2][1], keep[3][1], len(tags), 1)
        chunks = [c.cpu().numpy().copy() for c in matcher.records(LEAST, device=True)]
        torch.cuda.synchronize()
        assert len(chunks) > 1 and np.array_equal(np.concatenate(chunks).astype(np.uint64), want)
        assert np.array_equal(np.concatenate(list(matcher.records(LEAST))), want)


def test_index_from_a_live_engine(matcher):
    enc, suf, sigma = _subject("random:3000")
    tags = _mixed_tags(enc, 20, 3)
    want, _ = tr.expected(enc, suf, tags, 1)
    with esa.EsaEngine(enc.size, sigma) as eng:
        eng.set_sequence(enc)
        eng.run(esa.WANT_SUF)
        dev = _device_copy(enc, 0)
        matcher.set_index_engine(eng, dev[1], enc.size)
        got = matcher.all_records(tags, 1)
        assert np.array_equal(got, want) and got.shape[0] > 20
        with pytest.raises(_lib.EsaError, match="not the whole table"):
            matcher.set_index_engine(eng, dev[1], enc.size - 1)


# ---- tag lengths and K ----

@pytest.mark.parametrize("K", [0, 1, 2, 3])
def test_tag_lengths(matcher, K):
    enc, _, _ = _subject("random:3000")
    tags = []
    for m in (1, 2, 12, 63, 64):
        if m > K:
            tags += [_cut(enc, 40, m), _edited(_cut(enc, 900, m), K, m) if m > 4 else _cut(enc, 3, m),
                     _cut(enc, 2436, m), _cut(enc, enc.size - m, m), tr.revcomp(_cut(enc, 1500, m))]
    want = _agree(matcher, "random:3000", tags, K)
    assert want.shape[0] >= len(tags) // 2


def test_nearly_every_position_matches(matcher):
    """K = m - 1: a start matches as soon as one tag letter shows up"""
    enc = _subject("random:200")[0]
    for m in (2, 5, 64):
        want = _agree(matcher, "random:200", [_cut(enc, 20, m), _random(m, 4, m)], m - 1)
        assert want.shape[0] > 300


# ---- batch sizes ----

def test_no_tag_and_one_tag(matcher):
    assert _agree(matcher, "random:3000", [], 1).shape == (0, 3)
    assert list(matcher.records(LEAST)) == []
    enc = _subject("random:3000")[0]
    assert _agree(matcher, "random:3000", [_cut(enc, 77, 14)], 1).shape[0] >= 1


def test_three_hundred_tags_of_mixed_lengths(matcher):
    enc = _subject("random:3000")[0]
    want = _agree(matcher, "random:3000", _mixed_tags(enc, 300, 4), 1)
    assert want.shape[0] > 300 and 300 % WAVES == 0 and (2 * 300 + 1) % WAVES


# ---- strand flags ----

@pytest.mark.parametrize("flags", [FORWARD, REVCOMP, BOTH])
def test_strands(matcher, flags):
    enc = _subject("random:3000")[0]
    tags = _mixed_tags(enc, 31, 5)
    want = _agree(matcher, "random:3000", tags, 1, flags)
    seen = set((want[:, 0] & np.uint64(1)).tolist())
    assert seen == {0: {0}, 1: {1}, 2: {0, 1}}[flags - 1]


# ---- widths of a successful child, deep wide levels ----

@pytest.mark.parametrize("copies", [1, 63, 64, 65, 130])
def test_width_of_the_successful_child(matcher, copies):
    """the 12-mer occurs `copies` times: with K = 0 its interval at depth 12 is the
    successful child, that wide; with K = 1 the children on the way are"""
    name = "copies:%d" % copies
    enc = _subject(name)[0]
    unit = enc[:12].copy()
    want = _agree(matcher, name, [unit], 0, FORWARD)
    assert want.shape[0] == copies
    _agree(matcher, name, [unit, _edited(unit, 1, 9), unit[:11]], 1)


@pytest.mark.parametrize("kind,unit", [("runof", [0] * 12), ("tandemof", [0, 1, 2] * 4)])
@pytest.mark.parametrize("occurrences", [1, 63, 64, 65, 489])
def test_width_of_the_successful_child_in_a_run_and_a_tandem_repeat(matcher, kind, unit, occurrences):
    """A tag of at most 64 letters occurs at least 437 times in 500 equal letters, so
    the narrow children come from shorter runs: a run of A (500 letters for 489
    occurrences) and a repeat of acg, each cut so that the 12-mer occurs 1, 63, 64,
    65 and 489 times.  With K = 0 its interval at depth 12 is the successful child,
    that wide; with K = 1 and 2 the children above it succeed, wider by the
    neighbours of the run's ends."""
    name = "%s:%d" % (kind, occurrences)
    unit = np.array(unit, dtype=np.uint8)
    want = _agree(matcher, name, [unit], 0, FORWARD)
    assert want.shape[0] == occurrences
    _agree(matcher, name, [unit, unit[:11], _edited(unit, 1, 3)], 1)
    _agree(matcher, name, [unit, np.roll(unit, 1)], 2, FORWARD)


@pytest.mark.parametrize("name", ["run:500", "tandem:500"])
def test_levels_stay_wide_down_to_the_last_depth(matcher, name):
    enc = _subject(name)[0]
    for m, K in ((30, 2), (64, 3), (64, 0)):
        tags = [_cut(enc, 0, m), _cut(enc, 1, m), _edited(_cut(enc, 2, m), 1, m)]
        want = _agree(matcher, name, tags, K, FORWARD)
        info = matcher.info()
        assert want.shape[0] > 128 and info["levels_pushed"] >= m - K - 1


def test_a_child_wider_than_64_times_64(matcher):
    """A^4200: the child of the root has more suffixes than two rounds of 64
    probes tell apart, so the search for its right bound takes a third (the
    brute force needs 10 ms for this subject)"""
    tags = [np.zeros(12, dtype=np.uint8), np.zeros(5, dtype=np.uint8)]
    for K in (0, 1):
        want = _agree(matcher, "run:4200", tags, K, set_index=K == 0)
        assert want.shape[0] >= 4189 + 4196 and matcher.info()["max_matches_of_one_job"] >= 4196


# ---- ends and specials ----

def test_ends_and_specials(matcher):
    enc = _subject("random:3000")[0]
    n = enc.size
    tags = [_cut(enc, 1188, 12),          # ends on the last letter before the separators at 1200
            _cut(enc, n - 12, 12),        # ends at n - 1
            np.concatenate([enc[1190:1200], [0, 1]]).astype(np.uint8),   # would need two more symbols there
            np.concatenate([enc[n - 10:], [2, 3]]).astype(np.uint8),
            _cut(enc, 690, 20),           # runs into the wildcards at 700
            _cut(enc, 695, 20), _cut(enc, 1795, 12)]
    exact = _agree(matcher, "random:3000", tags, 0, FORWARD)
    assert {(0, 1188), (2, n - 12)} <= {(int(r[0]), int(r[1])) for r in exact}
    plain = _agree(matcher, "random:3000", tags, 2)
    wild = _agree(matcher, "random:3000", tags, 2, BOTH | WITH_WILDCARDS)
    assert wild.shape[0] > plain.shape[0]


def test_subject_shorter_than_the_tag_and_subjects_of_specials(matcher):
    tag = _random(40, 4, 3)
    for name in ("random:10", "random:1", "specials:50", "specials:1"):
        for flags in (BOTH, BOTH | WITH_WILDCARDS):
            _agree(matcher, name, [tag, tag[:3]], 2, flags)
    matcher.set_index(np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.uint64))
    assert matcher.all_records([tag], 1).shape == (0, 3)
    assert _agree(matcher, "random:10", [tag], 39).shape[0] > 0


# ---- another alphabet ----

def test_twenty_letters_forward_only(matcher):
    enc = _subject("protein:2000")[0]
    tags = [_cut(enc, 100, 12), _edited(_cut(enc, 500, 30), 2, 1, 20), _cut(enc, 290, 14), _random(5, 20, 2)]
    for K, flags in ((0, FORWARD), (2, FORWARD), (2, FORWARD | WITH_WILDCARDS), (2, FORWARD | BEST)):
        _agree(matcher, "protein:2000", tags, K, flags)
    for flags in (REVCOMP, BOTH):
        with pytest.raises(_lib.EsaError, match="GTAMD_TAGMATCH_REVCOMP.*4 letters"):
            matcher.prepare(tags, 1, flags)
    enc4 = _subject("random:3000")[0]
    matcher.set_index(enc4, _subject("random:3000")[1], 4)
    with pytest.raises(_lib.EsaError, match="tag number 1 holds a symbol that is no letter"):
        matcher.prepare([_cut(enc4, 0, 12), np.array([0, 1, 7, 2], dtype=np.uint8)], 1)


# ---- best ----

def test_best(matcher):
    enc = _subject("random:3000")[0]
    base = _cut(enc, 2000, 30)
    one = base.copy()
    one[10] = (one[10] + 1) % 4
    two = one.copy()
    two[20] = (two[20] + 2) % 4
    tags = [base, one, two, _random(30, 4, 77), tr.revcomp(one), _cut(enc, 100, 12)]
    for flags in (BOTH | BEST, FORWARD | BEST, REVCOMP | BEST):
        _agree(matcher, "random:3000", tags, 2, flags)
    _agree(matcher, "random:3000", tags, 2, BOTH | BEST)
    assert matcher.best_k().tolist() == [0, 1, 2, tagmatch.NO_K, 1, 0]
    _agree(matcher, "random:3000", tags, 2, BOTH)
    assert matcher.best_k().tolist() == [2, 2, 2, tagmatch.NO_K, 2, 2]


# ---- emit windows ----

def test_pieces_of_any_capacity(matcher):
    """A^4000, the tags A^12 and A^5 with K = 1: nearly every position matches on the
    forward strand, none on the other; in pieces of the smallest capacity, of 1000
    and in one"""
    enc, suf, _ = _subject("run:4000")
    tags = [np.zeros(12, dtype=np.uint8), np.zeros(5, dtype=np.uint8)]
    want = _agree(matcher, "run:4000", tags, 1)
    assert matcher.info()["max_matches_of_one_job"] > 3000
    for capacity in (LEAST, 1000, LEAST + 13):
        matcher.prepare(tags, 1)
        chunks = list(matcher.records(capacity))
        assert [c.shape[0] for c in chunks[:-1]] == [capacity] * (len(chunks) - 1) and len(chunks) > 3
        assert np.array_equal(np.concatenate(chunks), want)
    with pytest.raises(_lib.EsaError, match="at least %d" % LEAST):
        list(matcher.records(LEAST - 1))
    import torch
    chunks = [c.cpu().numpy().copy() for c in matcher.records(1000, device=True)]
    torch.cuda.synchronize()
    assert np.array_equal(np.concatenate(chunks).astype(np.uint64), want)


def test_two_prepares_on_one_object(matcher):
    enc = _subject("random:3000")[0]
    a, b = _mixed_tags(enc, 50, 6), _mixed_tags(enc, 9, 7)
    first = _agree(matcher, "random:3000", a, 2)
    second = _agree(matcher, "random:3000", b, 1, set_index=False)
    assert first.shape[0] != second.shape[0]
    assert np.array_equal(_agree(matcher, "random:3000", a, 2, set_index=False), first)


# ---- tables that are not an index ----

@pytest.mark.parametrize("width", WIDTHS)
def test_tables_that_are_no_index(matcher, width):
    """plain data: the loop bounds of the walk make them harmless; the calls
    return, the records are unspecified"""
    enc = _subject("random:3000")[0]
    tags = _mixed_tags(enc, 20, 8) + [np.zeros(3, dtype=np.uint8)]
    top = np.iinfo(width).max
    shuffled = np.random.default_rng(1).permutation(enc.size + 1).astype(width)
    beyond = _subject("random:3000")[1].astype(width)
    beyond[::5] = top
    beyond[1::7] = enc.size + 3
    for suf in (shuffled, beyond, np.zeros(enc.size + 1, dtype=width), np.full(enc.size + 1, top, dtype=width)):
        matcher.set_index(enc, suf)
        for flags in (BOTH, BOTH | WITH_WILDCARDS):
            info = matcher.prepare(tags, 2, flags)
            total = sum(c.shape[0] for c in matcher.records(1000))
            assert total == info["matches"] <= info["jobs"] * (enc.size + 1)


# ---- what is refused ----

def test_refusals(gpu):
    enc, suf, _ = _subject("random:3000")
    tag = _cut(enc, 5, 12)
    with tagmatch.TagMatches() as f:
        with pytest.raises(_lib.EsaError, match="no index is set"):
            f.prepare([tag], 1)
        with pytest.raises(_lib.EsaError, match="nothing is prepared"):
            list(f.records())
        with pytest.raises(_lib.EsaError, match="entries of 3 bytes, 4 or 8 expected"):
            f.set_index_device(1 << 20, 100, 1 << 21, 3)
        with pytest.raises(_lib.EsaError, match="beyond the limit of a single build"):
            f.set_index_device(1 << 20, (1 << 32) - 4096, 1 << 21, 8)
        with pytest.raises(_lib.EsaError, match="alphabet of 33 letters"):
            f.set_index(enc, suf, 33)
        f.set_index(enc, suf)
        with pytest.raises(_lib.EsaError, match="at least one strand"):
            f.prepare([tag], 1, BEST)
        with pytest.raises(_lib.EsaError, match="at least one strand"):
            f.prepare([tag], 1, BOTH | 16)
        with pytest.raises(_lib.EsaError, match="WITH_WILDCARDS is taken only with K > 0"):
            f.prepare([tag], 0, BOTH | WITH_WILDCARDS)
        with pytest.raises(_lib.EsaError, match="tag number 1 of length 65; tags must not be longer than 64"):
            f.prepare([tag, _random(65, 4, 1)], 1)
        with pytest.raises(_lib.EsaError, match="tag number 2 of length 2; tags must be longer than the allowed "
                                                r"number of errors \(which is 2\)"):
            f.prepare([tag, tag, tag[:2]], 2)
        with pytest.raises(_lib.EsaError, match="tag number 0 is empty"):
            f.prepare([tag[:0], tag], 1)
        with pytest.raises(_lib.EsaError, match="a wildcard in a tag is refused"):
            f.prepare([np.array([0, 1, 254, 2], dtype=np.uint8)], 1)
        with pytest.raises(_lib.EsaError, match="nothing is prepared"):      # a refused prepare is none
            list(f.records())
        want, _ = tr.expected(enc, suf, [tag], 1)
        assert np.array_equal(f.all_records([tag], 1), want)
