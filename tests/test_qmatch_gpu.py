"""Maximal exact matches of a query on the device (include/gtamd_qmatch.h,
genometools_amd/qmatch.py) against the brute force of tests/qmatch_reference.py:
every record, none sampled, in the reference's order.  The suffix tables come
from the engine, in this process, as 8- and as 4-byte entries.

The shapes are the smallest at which each part can go wrong: a workgroup takes
T query positions in the interval pass and T candidates in the emit passes, an
emit call takes chunks of at least LEAST candidates (qmatch.geometry()).  The
second level of each -- more than 65,536 query positions, more than 2^24
candidates in one emit call, a table of more than one upload piece -- is in
tests/test_scale_gpu.py."""
import functools
import math
import threading

import numpy as np
import pytest

import qmatch_reference as qr
from genometools_amd import _lib, esa, qmatch
from test_qmatch_host import QUERY, SUBJECT, _coded

pytestmark = pytest.mark.gpu

T, LEAST = qmatch.geometry()
WIDTHS = [np.uint64, np.uint32]


@pytest.fixture(scope="module")
def matcher(gpu):
    with qmatch.QueryMatches() as f:
        yield f


def _random(n, sigma, seed):
    return np.random.default_rng(seed).integers(0, sigma, n, dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def _subject(name):
    """(enc, sigma) of a named subject; shared, never written to"""
    kind, _, arg = name.partition(":")
    if kind == "fixture":
        enc, sigma = qr.encoded(arg, arg.endswith(".fsa")), 20 if arg.endswith(".fsa") else 4
    elif kind == "random":               # a wildcard run, two separators
        enc, sigma = _random(int(arg), 4, 41), 4
        enc[700:705] = 254
        enc[[1200, 1201]] = 255
    elif kind == "run":
        enc, sigma = np.zeros(int(arg), dtype=np.uint8), 4
    elif kind == "hand":
        enc, sigma = _coded(SUBJECT), 4
    else:
        raise ValueError(name)
    enc = enc.copy()
    enc.setflags(write=False)
    return enc, sigma


@functools.lru_cache(maxsize=None)
def _engine_suf(name):
    enc, sigma = _subject(name)
    with esa.EsaEngine(enc.size, sigma) as eng:
        eng.set_sequence(enc)
        eng.run(esa.WANT_SUF)
        suf = eng.table(esa.TAB_SUF)
    suf.setflags(write=False)
    return suf


def _set(matcher, name, width=np.uint64):
    enc, suf = _subject(name)[0], _engine_suf(name)
    matcher.set_index(enc, suf.astype(width))
    return enc, suf


def _check_info(info, want, m, n, min_len):
    """the figures after all records have been given, and the two derived bounds"""
    assert info["positions"] == m and info["matches"] == want.shape[0]
    assert info["seeds"] <= info["candidates"] and info["matches"] <= info["candidates"]
    assert (info["candidates"] == 0) == (info["max_width"] == 0) == (info["seeds"] == 0)
    # an extension looks at the len - L letters behind the seed and at the symbol that
    # ends it; a search makes at most ceil(log2 N) comparisons of at most L symbols and
    # the one that ends it, twice a position
    assert info["extension_symbols"] <= int((want[:, 2] - min_len + 1).sum())
    assert info["search_symbols"] <= m * (2 * math.ceil(math.log2(n + 1)) + 2) * (min_len + 1)


def _agree(matcher, name, query, min_len, width=np.uint64, capacity=qmatch.DEFAULT_CAPACITY, mode="fwd"):
    enc, suf = _set(matcher, name, width)
    want = qr.expected(enc, suf, query, min_len, mode)
    got = matcher.all_matches(query, min_len, mode, capacity)
    assert got.dtype == np.uint64 and got.shape == want.shape
    assert np.array_equal(got.astype(np.int64), want)
    _check_info(matcher.info(), want, len(query), enc.size, min_len)
    return want


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("m", [T + 3, T, 3 * T + 1])
def test_queries_around_the_tile_size(matcher, m, width):
    enc, _ = _subject("random:3000")
    query = np.concatenate([enc[100:100 + m // 2], _random(m - m // 2 - 40, 4, 5), enc[2960:]])
    query[30] = (query[30] + 1) % 4
    assert query.size == m
    assert _agree(matcher, "random:3000", query, 8, width).shape[0] > 3


@pytest.mark.parametrize("width", WIDTHS)
def test_one_seed_over_many_chunks_and_calls(matcher, width):
    """A^5000 against A^24, L = 16: nine seeds of 4985 occurrences each.  All of
    query position 0 are left-maximal, of the others only the one at p = 0, the
    first of its interval.  With the smallest capacity four calls fill up; the
    chunk of the fifth reaches into position 1; each of the next seven goes
    through chunk after chunk without a record until it meets the one of its
    position, which leaves less room than a chunk needs; the last finds none"""
    enc, suf = _set(matcher, "run:5000", width)
    query = np.zeros(24, dtype=np.uint8)
    want = qr.expected(enc, suf, query, 16)
    assert want.shape[0] == 4985 + 8
    info = matcher.prepare(query, 16)
    assert (info["seeds"], info["max_width"], info["candidates"]) == (9, 4985, 9 * 4985) and 4985 > 4096
    with pytest.raises(_lib.EsaError, match="at least %d" % LEAST):
        list(matcher.emit(LEAST - 1))
    chunks = list(matcher.emit(LEAST))                 # (the refusal has left the object usable)
    sizes = [c.shape[0] for c in chunks]
    full = 4985 // LEAST
    assert LEAST == 1024 and LEAST - (4985 - full * LEAST) >= 1     # (what the sizes below are worked out for)
    assert sizes == [LEAST] * full + [4985 - full * LEAST + 1] + [1] * 7 and len(sizes) > 3
    assert np.array_equal(np.concatenate(chunks).astype(np.int64), want)
    _check_info(matcher.info(), want, 24, 5000, 16)
    # any capacity gives the same records
    assert np.array_equal(matcher.all_matches(query, 16, capacity=LEAST + 77).astype(np.int64), want)
    assert np.array_equal(matcher.all_matches(query, 16).astype(np.int64), want)


def test_minimum_length_one(matcher):
    enc, _ = _subject("random:3000")
    query = np.concatenate([enc[650:760], [255], _random(150, 4, 6), [254, 254], enc[:40]]).astype(np.uint8)
    for width in WIDTHS:
        want = _agree(matcher, "random:3000", query, 1, width, capacity=50000)     # (several calls)
    assert want.shape[0] > 100000


def test_minimum_length_beyond_every_unit(matcher):
    enc, _ = _set(matcher, "random:3000")
    query = np.concatenate([enc[10:20], [255], enc[40:50], [255], enc[2990:]]).astype(np.uint8)
    info = matcher.prepare(query, 11)
    assert (info["seeds"], info["candidates"], info["max_width"]) == (0, 0, 0)
    assert list(matcher.emit()) == [] and matcher.info()["matches"] == 0
    assert matcher.all_matches(query, 10).shape[0] >= 3


@pytest.mark.parametrize("width", WIDTHS)
def test_a_long_planted_copy(matcher, width):
    enc, _ = _subject("random:3000")
    query = _random(1000, 4, 7)
    query[300:700] = enc[2000:2400]
    query[299], query[700] = (enc[1999] + 1) % 4, (enc[2400] + 1) % 4
    want = _agree(matcher, "random:3000", query, 300, width)
    assert want.tolist() == [[2000, 300, 400]]
    assert matcher.info()["extension_symbols"] == 101


@pytest.mark.parametrize("width", WIDTHS)
def test_matches_that_touch_the_ends_and_the_specials(matcher, width):
    """the text worked by hand in tests/test_qmatch_host.py, and copies from around
    the wildcards, the separators and both ends of a larger subject"""
    want = _agree(matcher, "hand", _coded(QUERY), 4, width)
    assert want.tolist() == [[0, 0, 4], [6, 7, 5], [7, 18, 4], [17, 25, 5], [29, 25, 5], [12, 33, 4]]
    enc, _ = _subject("random:3000")
    query = np.concatenate([enc[:40], [255], enc[680:720], [254], enc[1180:1230], enc[2960:], [255], enc[:30],
                            enc[2970:]]).astype(np.uint8)
    for min_len in (1, 20, 12):
        want = _agree(matcher, "random:3000", query, min_len, width)
    touched = {(p, p + l) for p, _, l in want.tolist()}
    assert any(a == 0 for a, _ in touched) and any(b == enc.size for _, b in touched)
    assert any(b == 700 for _, b in touched) and any(a == 705 for a, _ in touched) and any(b == 1200 for _, b in touched)


def test_protein(matcher):
    query = qr.encoded("sw100K2.fsa", True)
    for width in WIDTHS:
        assert _agree(matcher, "fixture:sw100K1.fsa", query, 4, width).shape[0] == 388
    assert _agree(matcher, "fixture:sw100K1.fsa", query, 4, mode="rev").shape[0] == 426


@pytest.mark.parametrize("mode", ["rev", "rcl"])
def test_reverse_and_reverse_complement(matcher, mode):
    query = qr.encoded("Atinsert.fna")
    want = _agree(matcher, "fixture:Duplicate.fna", query, 8, mode=mode)
    assert want.shape[0] == (56 if mode == "rev" else 82)
    # the index against itself, as the tool's -r / -p without -q asks
    enc = _subject("fixture:Duplicate.fna")[0]
    _agree(matcher, "fixture:Duplicate.fna", enc, 8, np.uint32, mode=mode)


def _device_copy(a, skew):
    import torch
    t = torch.empty(a.nbytes + 64, dtype=torch.uint8, device="cuda:0")
    t[skew:skew + a.nbytes] = torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to("cuda:0")
    torch.cuda.synchronize()
    return t, t.data_ptr() + skew


@pytest.mark.parametrize("width", WIDTHS)
def test_index_query_and_records_in_device_memory(matcher, width):
    """every alignment of the sequences' first symbols; the records left on the
    device and copied are those given to the host"""
    import torch
    name, min_len = "fixture:Atinsert.fna", 8
    enc, suf = _subject(name)[0], _engine_suf(name)
    query = qr.encoded("Atinsert_seqrange_3-7.fna")
    want = qr.expected(enc, suf, query, min_len)
    assert want.shape[0] == 543
    for skew in (0, 1, 2, 3):
        keep = [_device_copy(enc, skew), _device_copy(suf.astype(width), 8), _device_copy(query, (skew + 1) % 4)]
        matcher.set_index_device(keep[0][1], enc.size, keep[1][1], np.dtype(width).itemsize)
        matcher.prepare_device(keep[2][1], query.size, min_len)
        chunks = [c.cpu().numpy().copy() for c in matcher.emit(LEAST, device=True)]
        torch.cuda.synchronize()
        assert len(chunks) >= 1 and np.array_equal(np.concatenate(chunks), want)
        matcher.prepare_device(keep[2][1], query.size, min_len)
        assert np.array_equal(np.concatenate(list(matcher.emit(LEAST))).astype(np.int64), want)


def test_two_prepares_on_one_object(matcher):
    enc, suf = _set(matcher, "random:3000")
    a = np.concatenate([enc[5:400], _random(300, 4, 8)])
    b = np.concatenate([_random(100, 4, 9), enc[1500:1600]])
    first = matcher.all_matches(a, 8)
    matcher.prepare(a, 8)
    info = matcher.prepare(b, 10)                 # (replaces what the first has prepared)
    assert info["positions"] == b.size and info["matches"] == 0
    assert np.array_equal(np.concatenate(list(matcher.emit())).astype(np.int64), qr.expected(enc, suf, b, 10))
    again = matcher.all_matches(a, 8)
    assert again.tobytes() == first.tobytes() and np.array_equal(first.astype(np.int64), qr.expected(enc, suf, a, 8))


def test_index_from_a_live_engine(matcher):
    name = "fixture:Atinsert.fna"
    enc, sigma = _subject(name)
    query = qr.encoded("Duplicate.fna")
    with esa.EsaEngine(enc.size, sigma) as eng:
        eng.set_sequence(enc)
        eng.run(esa.WANT_SUF)
        dev = _device_copy(enc, 0)
        matcher.set_index_engine(eng, dev[1], enc.size)
        got = matcher.all_matches(query, 8)
        assert np.array_equal(got.astype(np.int64), qr.expected(enc, _engine_suf(name), query, 8)) and got.shape[0] == 68
        with pytest.raises(_lib.EsaError, match="not the whole table"):
            matcher.set_index_engine(eng, dev[1], enc.size - 1)
        assert matcher.all_matches(query, 8).tobytes() == got.tobytes()     # (the index before is kept)
        eng.run(esa.WANT_LCP)
        with pytest.raises(_lib.EsaError, match="did not produce"):
            matcher.set_index_engine(eng, dev[1], enc.size)


def test_refusals(gpu):
    enc, suf = _subject("random:3000")[0], _engine_suf("random:3000")
    query = enc[100:300]
    want = qr.expected(enc, suf, query, 8)
    with qmatch.QueryMatches() as f:
        with pytest.raises(_lib.EsaError, match="no index is set"):
            f.prepare(query, 8)
        with pytest.raises(_lib.EsaError, match="nothing is prepared"):
            list(f.emit())
        with pytest.raises(_lib.EsaError, match="entries of 3 bytes, 4 or 8 expected"):
            f.set_index_device(1 << 20, 100, 1 << 21, 3)
        # arguments only: nothing of that size exists
        with pytest.raises(_lib.EsaError, match="beyond the limit of a single build"):
            f.set_index_device(1 << 20, (1 << 32) - 4096, 1 << 21, 8)
        with pytest.raises(_lib.EsaError, match="no index is set"):      # a refused index is none
            f.prepare(query, 8)
        f.set_index(enc, suf)
        with pytest.raises(_lib.EsaError, match="minimum length of 0"):
            f.prepare(query, 0)
        with pytest.raises(_lib.EsaError, match="nothing is prepared"):
            list(f.emit())
        assert np.array_equal(f.all_matches(query, 8).astype(np.int64), want)
        with pytest.raises(_lib.EsaError, match="at least %d" % LEAST):
            list(f.emit(LEAST - 1))
        with pytest.raises(_lib.EsaError, match="at least %d" % LEAST):
            list(f.emit(0))
        assert np.array_equal(np.concatenate(list(f.emit(LEAST))).astype(np.int64), want)


def test_a_part_build_is_refused(matcher):
    """two contexts build the two slices of one table: neither is an index"""
    import torch
    import thread_comm as tc
    enc, sigma = _subject("random:3000")
    query = enc[100:300]
    _set(matcher, "random:3000")
    before = matcher.all_matches(query, 8)
    d_enc = torch.from_numpy(enc.copy()).to("cuda:0")
    torch.cuda.synchronize()
    shared, lock, said, errors = tc.ThreadComm(2), threading.Lock(), [None, None], []

    def worker(r):
        try:
            with esa.EsaEngine(enc.size, sigma) as eng:
                eng.set_sequence(enc)
                eng.set_part(r, 2, shared.view(r))
                eng.run(esa.WANT_SUF)
                with lock:                     # (one thread at a time per matcher)
                    try:
                        matcher.set_index_engine(eng, d_enc.data_ptr(), enc.size)
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
    assert matcher.all_matches(query, 8).tobytes() == before.tobytes() and before.shape[0] >= 1
