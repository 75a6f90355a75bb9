"""The walk of one suffix over the segments of its run
(genometools_amd/csrc/esa_maxpairs_walk.h) -- the code every lane of the
maximal-pairs kernels runs -- compiled with g++ and run on the CPU over every
entry, against the brute force of tests/maxpairs_reference.py.  The segments
are made with numpy from the oracle's tables.  No GPU: what is left for
tests/test_maxpairs_gpu.py is the kernels around the walk (flags, compaction,
scans), the memory they are given and the C ABI."""
import numpy as np
import pytest

import maxpairs_reference as mp

DNA = ["Atinsert.fna", "Duplicate.fna", "Random-Small.fna", "Random.fna", "Random159.fna",
       "Random160.fna", "RandomN.fna", "TTT-small.fna", "trna_glutamine.fna"]


@pytest.fixture(scope="module")
def shim():
    return mp.load_shim()


def _agree(lib, name, min_len, width=np.uint64):
    enc, _, t = mp.tables(name)
    rec, fig = mp.walk(lib, enc, t["suf"].astype(width), t["lcpfull"], min_len)
    want = mp.expected(name, min_len)
    assert np.array_equal(mp.sort_records(rec), want)
    assert np.array_equal(rec, mp.table_order(want, t["suf"]))           # table order, as emitted
    assert fig[0] == want.shape[0]
    assert fig[2] == (want[:, 2].max() if want.size else 0)
    assert fig[3] <= 2 * fig[0] + 2 * fig[4]
    return fig


@pytest.mark.parametrize("min_len", [8, 14, 20])
@pytest.mark.parametrize("name", DNA)
def test_dna_fixtures(shim, name, min_len):
    _agree(shim, "fixture:" + name, min_len)


@pytest.mark.parametrize("min_len", [6, 10])
def test_protein_fixture(shim, min_len):
    _agree(shim, "fixture:sw100K1.fsa:protein", min_len)


def test_repfind_example(shim):
    for min_len in (1, 2, 5):
        _agree(shim, "fixture:Repfind-example.fna", min_len, np.uint32)


@pytest.mark.parametrize("name", ["homopolymer:4096", "tandem:1400"])
def test_work_bound_on_repeats_of_one_unit(shim, name):
    """one run of about k suffixes and about k pairs: a walk over all j > i would
    take k * k / 2 steps"""
    pairs, _, _, steps, M, _ = _agree(shim, name, 16)
    k = mp.subject(name)[0].size
    assert k - 40 <= M <= k and k // 3 - 40 <= pairs <= k      # (pairs start at position 0 only)
    assert steps <= 2 * pairs + 2 * M < k * k // 1000


@pytest.mark.parametrize("min_len", [8, 255, 256, 300, 600, 601])
def test_long_copies(shim, min_len):
    fig = _agree(shim, "copies:600", min_len)
    assert (fig[0] > 0) == (min_len <= 600)
    if min_len > 8:
        assert fig[:3] == ([1, 1, 600] if min_len <= 600 else [0, 0, 0])


def test_specials_on_the_left(shim):
    _agree(shim, "leftspecials", 8)
    enc, _, _ = mp.tables("leftspecials")
    want = mp.expected("leftspecials", 40)
    mer = enc[:40]
    at = [p for p in range(enc.size - 39) if np.array_equal(enc[p:p + 40], mer)]
    unique = [p for p in at if p == 0 or enc[p - 1] >= 254]
    assert len(at) == 8 and len(unique) == 5
    listed = {(p, q) for p, q, _ in want.tolist()}
    assert all((p, q) in listed for p in unique for q in at if p < q)
    assert all((p, q) in listed for q in unique for p in at if p < q)
    _agree(shim, "leftspecials", 40)


def test_big_runs(shim):
    pairs, most, _, _, M, nseg = _agree(shim, "bigruns:5000", 6)
    assert pairs > 50000 and most > 30 and nseg > 1000


def test_other_shapes(shim):
    _agree(shim, "protein:3000", 4)
    _agree(shim, "small:64", 1)
    fig = _agree(shim, "small:64", 30)
    assert fig[0] == 0 and fig[4] == 0
    for n in (1, 2, 3):
        _agree(shim, "homopolymer:%d" % n, 1)
