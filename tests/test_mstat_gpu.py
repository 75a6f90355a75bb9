"""Matching statistics and minimum unique prefixes on the device
(include/gtamd_mstat.h, genometools_amd/mstat.py) against the brute force of
tests/mstat_reference.py: every query position, every value, none sampled.  The
suffix tables come from the CPU oracle, never from the engine, except where the
engine's resident table is what is tested.

Sizes: T = query positions of one workgroup, W = symbols of one wide
comparison, WMIN = symbols from which it is used (mstat.geometry()).

One statement of the issue this file does NOT follow: "query T^(n+1) has mu = 0
everywhere" over the subject T^n.  By the issue's own definition, and in the
reference (`gt uniquesub` prints `0 4` and `1 4` for TTTTT against TTTT), the
prefix T^n of positions 0 and 1 occurs exactly once: mu = n there, 0 behind."""
import functools
import threading

import numpy as np
import pytest

import mstat_reference as mr
import oracle_util as ou
from genometools_amd import esa, mstat

pytestmark = pytest.mark.gpu

T, W, WMIN = mstat.geometry()
WILDCARD, SEPARATOR = 254, 255
DNA = ["Atinsert.fna", "Duplicate.fna", "Random-Small.fna", "Random.fna", "Random159.fna",
       "Random160.fna", "RandomN.fna", "TTT-small.fna", "trna_glutamine.fna"]


@pytest.fixture(scope="module")
def searcher(gpu):
    with mstat.MatchStats() as s:
        assert (s.TILE, s.WORD, s.WORD_MIN) == (T, W, WMIN)
        yield s


def _random(n, sigma, seed):
    return np.random.default_rng(seed).integers(0, sigma, n, dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def _subject(name):
    """(enc, sigma, suffix table of the oracle); shared, never written to"""
    kind, _, arg = name.partition(":")
    v = int(arg) if arg else 0
    if kind == "planted":          # two separators and a wildcard run
        enc, sigma = _random(5000, 4, 21), 4
        enc[1000:1005] = WILDCARD
        enc[[2000, 3500]] = SEPARATOR
    elif kind == "run":
        enc, sigma = np.full(v, 3, dtype=np.uint8), 4
    elif kind == "twoletters":     # a subject over two of the four letters
        enc, sigma = _random(v, 2, 22) * 2, 4
        enc[v // 2] = SEPARATOR
    elif kind == "protein":
        enc, sigma = _random(v, 20, 23), 20
        enc[np.random.default_rng(24).integers(0, v, 12)] = WILDCARD
        enc[v // 3] = SEPARATOR
    elif kind == "binary":         # a two-letter alphabet, as a symbol map gives
        enc, sigma = _random(v, 2, 25), 2
        enc[v // 4:v // 4 + 2] = WILDCARD
    elif kind == "copy":           # the second half is a copy of the first
        half = _random(v // 2, 4, 26)
        enc, sigma = np.concatenate([half, half]), 4
    else:
        raise KeyError(name)
    suf = ou.esa(enc, sigma)["suf"]
    enc.setflags(write=False)
    suf.setflags(write=False)
    return enc, sigma, suf


def _agree(s, query, want, max_len=0):
    """both questions for one query against (ms, w, mu)"""
    ms, w, mu = want
    length, pos = s.matstat(query, max_len)
    unique = s.uniquesub(query, max_len)
    assert length.dtype == np.uint32 and pos.dtype == np.uint64 and unique.dtype == np.uint32
    if max_len == 0:
        assert np.array_equal(length, ms), np.flatnonzero(length != ms)[:5]
        assert np.array_equal(pos, w), np.flatnonzero(pos != w)[:5]
        assert np.array_equal(unique, mu), np.flatnonzero(unique != mu)[:5]
    else:
        assert np.array_equal(length, mr.capped(ms, max_len))
        exact = ms <= max_len
        assert np.array_equal(pos[exact], w[exact])
        assert np.array_equal(unique, mr.capped(mu, max_len))


def _against_brute_force(s, name, query, max_len=0):
    enc, sigma, suf = _subject(name)
    query = np.ascontiguousarray(query, dtype=np.uint8)
    s.set_index(enc, suf, sigma)
    _agree(s, query, mr.brute_force(enc, suf, query), max_len)


# ---- the nine fixtures, pairwise ----------------------------------------------

def _device_copy(a, skew):
    import torch
    t = torch.empty(a.nbytes + 64, dtype=torch.uint8, device="cuda:0")
    t[skew:skew + a.nbytes] = torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to("cuda:0")
    torch.cuda.synchronize()
    return t, t.data_ptr() + skew


@pytest.mark.parametrize("how", ["host64", "host32", "device64", "device32", "engine"])
@pytest.mark.parametrize("subject", DNA)
def test_fixtures_pairwise(searcher, subject, how):
    enc, suf = mr.encoded(subject, False), mr.suffix_table(subject, False)
    keep = []
    if how.startswith("host"):
        searcher.set_index(enc, suf.astype(np.uint32 if how == "host32" else np.uint64), 4)
    elif how.startswith("device"):
        width = np.uint32 if how == "device32" else np.uint64
        keep = [_device_copy(enc, 3), _device_copy(suf.astype(width), 8)]       # (not multiples of 16)
        searcher.set_index_device(keep[0][1], enc.size, keep[1][1], np.dtype(width).itemsize, 4)
    else:
        eng = esa.EsaEngine(enc.size, 4)
        eng.set_sequence(enc)
        eng.run(esa.WANT_SUF)
        keep = [eng, _device_copy(enc, 0)]
        searcher.set_index_engine(eng, keep[1][1], enc.size)
    try:
        for query in DNA:
            if query != subject:
                _agree(searcher, mr.encoded(query, False), mr.expected(subject, query, False))
    finally:
        if how == "engine":
            keep[0].close()


def test_device_queries_and_outputs(searcher):
    """query and both outputs in device memory, the witness left out"""
    import torch
    enc, suf = mr.encoded("Atinsert.fna", False), mr.suffix_table("Atinsert.fna", False)
    query = mr.encoded("Random159.fna", False)
    ms, w, mu = mr.expected("Atinsert.fna", "Random159.fna", False)
    searcher.set_index(enc, suf, 4)
    q = _device_copy(query, 5)
    length = torch.zeros(query.size, dtype=torch.int32, device="cuda:0")
    pos = torch.zeros(query.size, dtype=torch.int64, device="cuda:0")
    searcher.matstat_device(q[1], query.size, length.data_ptr(), pos.data_ptr())
    assert np.array_equal(length.cpu().numpy(), ms) and np.array_equal(pos.cpu().numpy(), w)
    length.zero_()
    searcher.matstat_device(q[1], query.size, length.data_ptr(), None)
    assert np.array_equal(length.cpu().numpy(), ms)
    searcher.uniquesub_device(q[1], query.size, length.data_ptr())
    assert np.array_equal(length.cpu().numpy(), mu)
    info = searcher.info()
    assert info["positions"] == query.size and info["symbols_compared"] > query.size
    assert info["device_ms"] > 0 and info["device_bytes"] >= enc.size + 8 * suf.size


# ---- planted lengths ----------------------------------------------------------------

LENGTHS = sorted({1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257,
                  WMIN - 1, WMIN, WMIN + 1, W - 1, W, W + 1})


@pytest.mark.parametrize("first_offset", [0, 17])
def test_planted_lengths(searcher, first_offset):
    """copies of subject substrings from offsets 0..33 (every alignment of the word
    comparison on the subject's side; the query's side moves with the lengths), each
    followed in turn by a letter that differs, a wildcard, a separator, the end"""
    enc, _, _ = _subject("planted")
    parts, offset, follow = [], first_offset, 0
    for rounds in range(2):
        for length in LENGTHS:
            copy = enc[offset:offset + length]
            assert (copy < 254).all()
            after = [[(int(enc[offset + length]) + 1) % 4], [WILDCARD], [SEPARATOR]][follow % 3]
            parts += [copy, np.array(after, dtype=np.uint8)]
            offset, follow = (offset + 1) % 34, follow + 1
    parts.append(enc[offset:offset + 257])          # ... and the query's end
    query = np.concatenate(parts)
    _against_brute_force(searcher, "planted", query)
    _against_brute_force(searcher, "planted", query, max_len=W)


def test_matches_into_the_subjects_end_a_separator_and_a_wildcard(searcher):
    enc, _, _ = _subject("planted")
    n = enc.size
    tail = _random(30, 4, 31)
    query = np.concatenate([enc[n - 40:], tail, [SEPARATOR], enc[n - 1:], tail, [SEPARATOR],
                            enc[1960:2000], tail, [WILDCARD], enc[975:1000], tail,
                            enc[n - 300:]]).astype(np.uint8)
    _against_brute_force(searcher, "planted", query)
    enc, sigma, suf = _subject("planted")
    length, pos = searcher.matstat(query)
    assert length[0] == 40 and pos[0] == n - 40                       # (40 letters are unique here)
    assert length[-300] == 300 and pos[-300] == n - 300 and length[-1] >= 1


def test_letters_the_subject_lacks_and_empty_queries(searcher):
    enc, sigma, suf = _subject("twoletters:600")
    query = np.concatenate([enc[10:40], [1, 3, 1], enc[100:130], [3]]).astype(np.uint8)
    _against_brute_force(searcher, "twoletters:600", query)
    length, _ = searcher.matstat(query)
    assert length[30:33].tolist() == [0, 0, 0] and length[-1] == 0
    # nothing to do
    length, pos = searcher.matstat(np.zeros(0, dtype=np.uint8))
    assert length.size == 0 and pos.size == 0 and searcher.info()["positions"] == 0
    # only specials
    query = np.array([SEPARATOR, WILDCARD, SEPARATOR], dtype=np.uint8)
    _agree(searcher, query, (np.zeros(3, dtype=np.int64),) * 3)


@pytest.mark.parametrize("m", [1, T - 1, T + 1, 3 * T - 1, 3 * T + 1])
def test_query_lengths_around_the_tile(searcher, m):
    enc, _, _ = _subject("planted")
    query = np.concatenate([enc[50:50 + m // 2], _random(m - m // 2, 4, 32 + m)])
    assert query.size == m
    _against_brute_force(searcher, "planted", query)


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 1000])
def test_runs_of_one_letter(searcher, n):
    """subject T^n: the suffix at 0 is the first of the table, and of every interval"""
    enc, sigma, suf = _subject("run:%d" % n)
    assert suf[0] == 0
    searcher.set_index(enc, suf, sigma)
    zeros = np.zeros
    # query T^n
    want_ms = np.arange(n, 0, -1)
    want_mu = zeros(n, dtype=np.int64)
    want_mu[0] = n
    _agree(searcher, enc, (want_ms, zeros(n, dtype=np.int64), want_mu))
    # query T^(n+1): the first two positions hold T^n, which occurs once
    query = np.full(n + 1, 3, dtype=np.uint8)
    want_ms = np.minimum(np.arange(n + 1, 0, -1), n)
    want_mu = zeros(n + 1, dtype=np.int64)
    want_mu[:2] = n
    _agree(searcher, query, (want_ms, zeros(n + 1, dtype=np.int64), want_mu))
    if n <= 65:
        for q in (enc, query):
            _agree(searcher, q, mr.brute_force(enc, suf, q))


@pytest.mark.parametrize("name,sigma", [("protein:3000", 20), ("binary:2000", 2)])
def test_other_alphabets(searcher, name, sigma):
    enc, _, _ = _subject(name)
    n = enc.size
    rng = np.random.default_rng(41)
    query = np.concatenate([enc[7:300], rng.integers(0, sigma, 200, dtype=np.uint8), [WILDCARD],
                            enc[n - 100:], enc[n // 3 - 20:n // 3 + 20]]).astype(np.uint8)
    _against_brute_force(searcher, name, query)
    _against_brute_force(searcher, name, query, max_len=5)


# ---- skew -----------------------------------------------------------------------------------

def test_a_query_that_is_a_copy_of_its_subject(searcher):
    """20 000 symbols, the second half a copy of the first: the matches sum to about
    10^8 symbols.  Exact without a cap; with max_len = 20 equal to min(value, 21),
    and matstat looks at far fewer symbols.  uniquesub does not: every position of
    the first half has two occurrences of its 21 letters, and only the whole
    comparison tells mu = 0 from mu > 20 (the `reruns` of the info)."""
    enc, sigma, suf = _subject("copy:20000")
    want = mr.brute_force(enc, suf, enc)
    ms, w, mu = want
    assert ms[0] == 20000 and mu[0] == 10001 and ms.sum() > 10 ** 8 and mu[10000:].max() == 0
    searcher.set_index(enc, suf, sigma)
    _agree(searcher, enc, want)
    searcher.matstat(enc)
    uncapped = searcher.info()["symbols_compared"]
    assert uncapped > ms.sum()
    _agree(searcher, enc, want, max_len=20)
    searcher.matstat(enc, 20)
    info = searcher.info()
    assert info["symbols_compared"] < 40 * 21 * enc.size < uncapped // 5 and info["reruns"] == 0
    searcher.uniquesub(enc, 20)
    rest = enc.size - np.arange(enc.size)
    assert searcher.info()["reruns"] == np.count_nonzero((ms >= 21) & ((mu == 0) | (mu > 21)) & (rest > 21))


# ---- refusals: none reaches a kernel --------------------------------------------------------------

def test_refusals(searcher):
    import torch
    enc, sigma, suf = _subject("planted")
    with mstat.MatchStats() as fresh:
        with pytest.raises(esa.EsaError, match="no index is set"):
            fresh.matstat(enc[:10])
        with pytest.raises(esa.EsaError, match="no index is set"):
            fresh.uniquesub(enc[:10])
        with pytest.raises(esa.EsaError, match="entries of 3 bytes, 4 or 8 expected"):
            fresh.set_index_device(1 << 20, 100, 1 << 21, 3, 4)
        # arguments only: nothing of that size exists
        limit = (1 << 32) - 4096
        with pytest.raises(esa.EsaError, match="beyond the limit of a single build"):
            fresh.set_index_device(1 << 20, limit, 1 << 21, 8, 4)
        with pytest.raises(esa.EsaError, match="1 to 253 expected"):
            fresh.set_index_device(1 << 20, 100, 1 << 21, 8, 254)
        with pytest.raises(esa.EsaError, match="no index is set"):      # a refused index is none
            fresh.matstat(enc[:10])
    d_enc = torch.from_numpy(enc.copy()).to("cuda:0")
    torch.cuda.synchronize()
    with esa.EsaEngine(enc.size, 4) as eng:
        eng.set_sequence(enc)
        eng.run(esa.WANT_SUF)
        with pytest.raises(esa.EsaError, match="not the whole table"):
            searcher.set_index_engine(eng, d_enc.data_ptr(), enc.size - 1)


def test_a_part_build_is_refused(searcher):
    """two contexts build the two slices of one table: neither is an index"""
    import torch
    import thread_comm as tc
    enc, sigma, suf = _subject("planted")
    d_enc = torch.from_numpy(enc.copy()).to("cuda:0")
    torch.cuda.synchronize()
    shared, lock, said, errors = tc.ThreadComm(2), threading.Lock(), [None, None], []

    def worker(r):
        try:
            with esa.EsaEngine(enc.size, sigma) as eng:
                eng.set_sequence(enc)
                eng.set_part(r, 2, shared.view(r))
                eng.run(esa.WANT_SUF)
                with lock:                     # (one thread at a time per searcher)
                    try:
                        searcher.set_index_engine(eng, d_enc.data_ptr(), enc.size)
                    except esa.EsaError as e:
                        said[r] = str(e)
        except Exception as e:   # noqa: BLE001
            errors.append((r, repr(e)))
            shared.barrier.abort()

    threads = [threading.Thread(target=worker, args=(r,)) for r in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for r in range(2):
        assert said[r] is not None and "not the whole table" in said[r] and \
            "the slices of a build in parts are not searched" in said[r], said
