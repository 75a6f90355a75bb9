"""Maximal pairs on the device (include/gtamd_maxpairs.h,
genometools_amd/maxpairs.py) against the brute force of
tests/maxpairs_reference.py: every record, none sampled, as sorted records and
in table order.  The tables come from the engine, in this process.

The shapes are the smallest at which each part can go wrong: a select pass
takes 1024 items a workgroup, a walk 256 entries; .lcp holds a byte 255 from
255 letters on.  The second level of each -- more than 65,536 run suffixes, more
than 4096 select tiles, a table of more than one upload piece -- is in
tests/test_scale_gpu.py."""
import functools

import numpy as np
import pytest

import maxpairs_reference as mp
from genometools_amd import _lib, esa, maxpairs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def finder(gpu):
    with maxpairs.MaxPairs() as f:
        yield f


@functools.lru_cache(maxsize=None)
def _engine_tables(name):
    """(enc, suf, lcp, llv) of the engine for a subject of maxpairs_reference;
    shared, never written to"""
    enc, sigma = (mp.encoded(*_fixture(name)), 20 if _fixture(name)[1] else 4) if name.startswith("fixture:") \
        else mp.subject(name)
    with esa.EsaEngine(enc.size, sigma) as eng:
        eng.set_sequence(enc)
        eng.run(esa.WANT_SUF | esa.WANT_LCP)
        out = (enc, eng.table(esa.TAB_SUF), eng.table(esa.TAB_LCP), eng.table(esa.TAB_LLV))
    for a in out:
        a.setflags(write=False)
    return out


def _fixture(name):
    parts = name.split(":")
    return parts[1], len(parts) > 2


def _set(finder, name, width=np.uint64):
    enc, suf, lcp, llv = _engine_tables(name)
    finder.set_index(enc, suf.astype(width), lcp, llv)
    return enc, suf


def _check(finder, info, rec, want, suf):
    """the records and the figures of one prepare against the expected records"""
    assert rec.dtype == np.uint64 and rec.shape == (want.shape[0], 3)
    rec = rec.astype(np.int64)
    assert np.array_equal(mp.sort_records(rec), want)
    assert np.array_equal(rec, mp.table_order(want, suf))
    assert info["pairs"] == want.shape[0]
    assert info["max_len"] == (want[:, 2].max() if want.size else 0)
    assert info["walk_steps"] <= 2 * info["pairs"] + 2 * info["run_suffixes"]
    assert info["runs"] <= info["segments"] <= info["run_suffixes"]
    assert (info["pairs"] == 0) == (info["max_pairs_of_one_suffix"] == 0)


def _agree(finder, name, min_len, width=np.uint64):
    _, suf = _set(finder, name, width)
    info = finder.prepare(min_len)
    _check(finder, info, finder.all_pairs(), mp.expected(name, min_len), suf)
    return info


@pytest.mark.parametrize("name", ["homopolymer:4096", "tandem:1400"])
def test_repeats_of_one_unit(finder, name):
    """one run of about k suffixes, about k pairs: a walk over all j > i would
    exceed the bound a thousandfold"""
    info = _agree(finder, name, 16)
    k = mp.subject(name)[0].size
    # (the suffixes of (ACG)^k start with three different letters: three runs)
    assert info["runs"] == (1 if name.startswith("homopolymer") else 3) and k - 48 <= info["run_suffixes"] <= k
    assert info["walk_steps"] <= 2 * info["pairs"] + 2 * info["run_suffixes"] < k * k // 1000


@pytest.mark.parametrize("min_len", [8, 255, 256, 300, 600, 601])
def test_long_copies(finder, min_len):
    """the .llv look-up in the flag (L > 255) and in the values"""
    _, _, lcp, llv = _engine_tables("copies:600")
    assert llv.size >= 2 and (lcp == 255).sum() == llv.size // 2
    info = _agree(finder, "copies:600", min_len)
    if min_len > 8:
        # suffixes k letters into the two copies share 600 - k letters: a run of two for
        # every k up to 600 - L, one pair (k = 0: the others have the same letter in front)
        runs = 601 - min_len
        want = (1, 1, 600, 2 * runs, runs) if min_len <= 600 else (0, 0, 0, 0, 0)
        assert tuple(info[k] for k in ("pairs", "max_pairs_of_one_suffix", "max_len", "run_suffixes", "runs")) == want


def test_specials_on_the_left(finder):
    """copies of one 40-mer at position 0, behind N, behind a separator and behind
    letters: every pair with a unique side is reported"""
    for min_len in (8, 40):
        _agree(finder, "leftspecials", min_len)
    enc = mp.subject("leftspecials")[0]
    at = [p for p in range(enc.size - 39) if np.array_equal(enc[p:p + 40], enc[:40])]
    unique = [p for p in at if p == 0 or enc[p - 1] >= 254]
    assert len(at) == 8 and len(unique) == 5
    listed = {(p, q) for p, q, _ in finder.all_pairs().tolist()}
    assert all((min(p, q), max(p, q)) in listed for p in unique for q in at if p != q)


def test_big_runs(finder):
    info = _agree(finder, "bigruns:5000", 6)
    assert info["pairs"] > 50000 and info["max_pairs_of_one_suffix"] > 30 and info["segments"] > 1000


def test_big_runs_across_workgroups(finder):
    """40,000 symbols, about 4 * 10^5 pairs: the brute force takes too long here,
    the walk on the CPU (tests/test_maxpairs_walk.py holds it to the brute force)
    stands in for it, with the oracle's tables"""
    name = "bigruns:40000"
    enc, _, t = mp.tables(name)
    want, fig = mp.walk(mp.load_shim(), enc, t["suf"], t["lcpfull"], 10)
    _, suf = _set(finder, name)
    assert np.array_equal(suf, t["suf"])
    info = finder.prepare(10)
    rec = finder.all_pairs(capacity=100000)          # (several chunks)
    assert np.array_equal(rec.astype(np.int64), want)
    got = [info[k] for k in ("pairs", "max_pairs_of_one_suffix", "max_len", "walk_steps", "run_suffixes", "segments")]
    assert got == fig and info["pairs"] > 300000 and info["run_suffixes"] > 2048


def _device_copy(a, skew):
    import torch
    t = torch.empty(a.nbytes + 64, dtype=torch.uint8, device="cuda:0")
    t[skew:skew + a.nbytes] = torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to("cuda:0")
    torch.cuda.synchronize()
    return t, t.data_ptr() + skew


@pytest.mark.parametrize("how", ["host64", "host32", "device64", "device32", "engine"])
def test_table_width_and_index_source(finder, how):
    name, min_len = "fixture:Atinsert.fna", 8
    enc, suf, lcp, llv = _engine_tables(name)
    want = mp.expected(name, min_len)
    assert want.shape[0] == 452
    keep = []
    if how.startswith("host"):
        finder.set_index(enc, suf.astype(np.uint32 if how == "host32" else np.uint64), lcp, llv)
    elif how.startswith("device"):
        width = np.uint32 if how == "device32" else np.uint64
        keep = [_device_copy(enc, 3), _device_copy(suf.astype(width), 8), _device_copy(lcp, 5)]
        finder.set_index_device(keep[0][1], enc.size, keep[1][1], np.dtype(width).itemsize, keep[2][1])
    else:
        eng = esa.EsaEngine(enc.size, 4)
        eng.set_sequence(enc)
        eng.run(esa.WANT_SUF | esa.WANT_LCP)
        keep = [eng, _device_copy(enc, 0)]
        finder.set_index_engine(eng, keep[1][1], enc.size)
    try:
        info = finder.prepare(min_len)
        _check(finder, info, finder.all_pairs(), want, suf)
    finally:
        if how == "engine":
            keep[0].close()


def test_engine_context_with_large_values(finder):
    """.llv taken from the engine's context"""
    enc, suf, _, _ = _engine_tables("copies:600")
    with esa.EsaEngine(enc.size, 4) as eng:
        eng.set_sequence(enc)
        eng.run(esa.WANT_SUF | esa.WANT_LCP)
        dev = _device_copy(enc, 0)
        finder.set_index_engine(eng, dev[1], enc.size)
        for min_len in (300, 20):
            info = finder.prepare(min_len)
            _check(finder, info, finder.all_pairs(), mp.expected("copies:600", min_len), suf)
        eng.run(esa.WANT_SUF)
        with pytest.raises(_lib.EsaError, match="did not produce"):
            finder.set_index_engine(eng, dev[1], enc.size)


@pytest.mark.parametrize("min_len", [6, 10])
def test_protein_fixture(finder, min_len):
    _agree(finder, "fixture:sw100K1.fsa:protein", min_len)


def test_protein_with_specials(finder):
    info = _agree(finder, "protein:3000", 4)
    assert info["max_len"] == 50


def test_every_dna_fixture(finder):
    for name in ("Duplicate.fna", "Random.fna", "RandomN.fna", "Random159.fna", "Random160.fna",
                 "Random-Small.fna", "TTT-small.fna", "trna_glutamine.fna", "Repfind-example.fna"):
        _agree(finder, "fixture:" + name, 8)
    assert _agree(finder, "fixture:Duplicate.fna", 8, np.uint32)["pairs"] == 29


def test_streaming(finder):
    """chunks of whole suffixes; the smallest capacity is that of the busiest suffix"""
    name, min_len = "bigruns:5000", 6
    _set(finder, name)
    info = finder.prepare(min_len)
    whole = finder.all_pairs()
    most, z = info["max_pairs_of_one_suffix"], info["pairs"]
    for capacity in (most, z // 7 + most):
        chunks = list(finder.pairs(capacity))
        assert all(0 < c.shape[0] <= capacity for c in chunks) and len(chunks) >= (7 if capacity == most else 2)
        assert np.array_equal(np.concatenate(chunks), whole)
    with pytest.raises(_lib.EsaError, match="at least %d" % most):
        list(finder.pairs(most - 1))
    assert np.array_equal(finder.all_pairs(), whole)          # (the refusal has left the object usable)


def test_chunks_in_device_memory(finder):
    import torch
    name, min_len = "bigruns:5000", 6
    _, suf = _set(finder, name)
    info = finder.prepare(min_len)
    chunks = [c.cpu().numpy().copy() for c in finder.pairs(info["pairs"] // 3 + info["max_pairs_of_one_suffix"],
                                                           device=True)]
    torch.cuda.synchronize()
    assert len(chunks) >= 3
    _check(finder, info, np.concatenate(chunks).astype(np.uint64), mp.expected(name, min_len), suf)


def test_no_pairs_and_all_pairs(finder):
    info = _agree(finder, "copies:600", 100)
    above = finder.prepare(info["max_len"] + 1)
    assert above["pairs"] == 0 and above["run_suffixes"] == 0 and finder.all_pairs().shape == (0, 3)
    every = _agree(finder, "small:64", 1)
    assert every["pairs"] == mp.expected("small:64", 1).shape[0] > 300
    for n in (1, 2, 3):
        _agree(finder, "homopolymer:%d" % n, 1)


def test_refusals(gpu):
    with maxpairs.MaxPairs() as f:
        with pytest.raises(_lib.EsaError, match="no index is set"):
            f.prepare(8)
        with pytest.raises(_lib.EsaError, match="nothing is prepared"):
            f.all_pairs()
        _set(f, "small:64")
        with pytest.raises(_lib.EsaError, match="minimum length of 0"):
            f.prepare(0)
        with pytest.raises(_lib.EsaError, match="nothing is prepared"):
            f.all_pairs()
        enc, suf, lcp, llv = _engine_tables("small:64")
        with pytest.raises(_lib.EsaError, match="4 or 8"):
            _lib.check(gpu.gtamd_maxpairs_set_index_host(f._p, enc.ctypes.data, enc.size, suf.ctypes.data, 2,
                                                         lcp.ctypes.data, None, 0))
        assert f.prepare(2)["pairs"] == mp.expected("small:64", 2).shape[0]      # (the index before is kept)


def test_two_calls_give_the_same_bytes(finder):
    _set(finder, "bigruns:5000")
    info = finder.prepare(6)
    first = finder.all_pairs().tobytes()
    again = finder.prepare(6)
    assert all(again[k] == info[k] for k in info if k not in ("device_ms", "device_bytes"))
    assert finder.all_pairs().tobytes() == first
    with maxpairs.MaxPairs() as other:
        _set(other, "bigruns:5000")
        other.prepare(6)
        assert other.all_pairs(capacity=info["max_pairs_of_one_suffix"] + 1000).tobytes() == first
