"""The index checker (include/gtamd_check.h, genometools_amd/check.py) on the
device.  The expected tables come from the CPU oracle, never from the engine:
the checker is tested apart from what it will check.  The tables of a sequence
are unique, so every oracle table must be accepted and every change of one
entry rejected -- with the table, and the index the criterion defines.

Sizes: T = table entries of one workgroup, L = length of a range of symbols
from which a position goes to the work list (check.geometry())."""
import functools

import numpy as np
import pytest

import device_check as dc
import oracle_util as ou
from check_criteria import first_suf_failure
from genometools_amd import check, esa, synth

pytestmark = pytest.mark.gpu

T, L = check.geometry()
WILDCARD, SEPARATOR = 254, 255


@pytest.fixture(scope="module")
def checker(gpu):
    with check.EsaChecker() as c:
        assert (c.TILE, c.LONG_CLAIM) == (T, L)
        yield c


# ---- sequences (by name: the oracle runs once for each) ----------------------

def _random(n, sigma, seed):
    return np.random.default_rng(seed).integers(0, sigma, n, dtype=np.uint8)


def _two_copies(blk, seed=5):
    b = _random(blk, 4, seed + blk)
    return np.concatenate([b, [WILDCARD], b]).astype(np.uint8)


def _with_specials(n, seed):
    """DNA with wildcard runs and separators; a special first and last"""
    enc = _random(n, 4, seed)
    rng = np.random.default_rng(seed + 1)
    for at in rng.integers(0, n, max(1, n // 200)):
        enc[at:at + int(rng.integers(1, 9))] = WILDCARD
    enc[rng.integers(0, n, max(1, n // 300))] = SEPARATOR
    enc[0], enc[-1] = SEPARATOR, WILDCARD
    return enc


def _sequence(name):
    kind, _, arg = name.partition(":")
    v = int(arg) if arg else 0
    if kind == "dna":
        return _random(v, 4, 100 + v), 4
    if kind == "specials":
        return _with_specials(v, 7), 4
    if kind == "allspecial":
        return np.array([WILDCARD, SEPARATOR] * (v // 2) + [WILDCARD], dtype=np.uint8), 4
    if kind == "protein":
        enc = _random(v, 20, 11)
        enc[v // 3] = SEPARATOR
        enc[v // 2:v // 2 + 3] = WILDCARD
        return enc, 20
    if kind == "copies":
        return _two_copies(v), 4
    if kind == "run":
        return np.zeros(v, dtype=np.uint8), 4
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _oracle(name):
    """(enc, tables of the oracle); shared, never written to"""
    enc, sigma = _sequence(name)
    ora = ou.esa(enc, sigma)
    for a in (enc, ora["suf"], ora["lcp"], ora["llv"], ora["bwt"]):
        a.setflags(write=False)
    return enc, ora


def _tables(name):
    """copies a test may damage: enc, suf, lcp, llv, bwt"""
    enc, ora = _oracle(name)
    return enc, ora["suf"].copy(), ora["lcp"].copy(), ora["llv"].copy(), ora["bwt"].copy()


def _accepted(res, ora):
    assert res.ok and res.table == 0 and res.criterion == check.CRIT_NONE and res.message == "", res
    assert res.checked == check.SUF | check.LCP | check.LLV | check.BWT
    st = ora["stats"]
    assert (res.longest, res.largelcpvalues, res.maxbranchdepth) == \
        (st["longest"], st["largelcpvalues"], st["maxbranchdepth"]), (res, st)


# ---- accepted -----------------------------------------------------------------

SIZES = [0, 1, 2, T - 2, T - 1, T, T + 1, 3 * T + 5]
ACCEPT = ["dna:%d" % n for n in SIZES] + ["specials:%d" % (3 * T + 5), "specials:300", "allspecial:1",
                                          "allspecial:301", "protein:%d" % (2 * T + 77)]


@pytest.mark.parametrize("name", ACCEPT)
@pytest.mark.parametrize("width", [np.uint64, np.uint32])
def test_oracle_tables_are_accepted(checker, name, width):
    enc, ora = _oracle(name)
    _accepted(checker.check(enc, ora["suf"].astype(width), ora["lcp"], ora["llv"], ora["bwt"]), ora)


def test_suffix_table_alone_and_with_one_other_table(checker):
    enc, ora = _oracle("specials:%d" % (3 * T + 5))
    res = checker.check(enc, ora["suf"])
    assert res.ok and res.checked == check.SUF and res.longest == ora["stats"]["longest"]
    res = checker.check(enc, ora["suf"], bwt=ora["bwt"])
    assert res.ok and res.checked == check.SUF | check.BWT
    res = checker.check(enc, ora["suf"], ora["lcp"], ora["llv"])
    assert res.ok and res.checked == check.SUF | check.LCP | check.LLV
    assert res.maxbranchdepth == ora["stats"]["maxbranchdepth"]


@pytest.mark.parametrize("width", [np.uint64, np.uint32])
def test_device_entry_point(checker, width):
    """tables already on the device, at addresses that are not multiples of 16"""
    import torch
    enc, ora = _oracle("copies:%d" % (4 * L + 3))
    n = enc.size

    def dev(a, skew):
        t = torch.empty(a.nbytes + 64, dtype=torch.uint8, device="cuda:0")
        t[skew:skew + a.nbytes] = torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to("cuda:0")
        return t, t.data_ptr() + skew
    keep = [dev(enc, 3), dev(ora["suf"].astype(width), 16), dev(ora["lcp"], 1),
            dev(np.ascontiguousarray(ora["llv"]), 8), dev(ora["bwt"], 5)]
    torch.cuda.synchronize()
    ptr = [p for _, p in keep]
    res = checker.check_device(ptr[0], n, ptr[1], np.dtype(width).itemsize, ptr[2], ptr[3],
                               len(ora["llv"]), ptr[4])
    _accepted(res, ora)
    assert res.long_claims >= 1


# ---- .llv boundary ----------------------------------------------------------------

@pytest.mark.parametrize("blk", [254, 255, 256, 255 + 300])
def test_llv_boundary_and_many_entries(checker, blk):
    enc, ora = _oracle("copies:%d" % blk)
    assert len(ora["llv"]) == max(0, blk - 254)      # none, one, two, many
    _accepted(checker.check(enc, ora["suf"], ora["lcp"], ora["llv"], ora["bwt"]), ora)


# ---- long claims --------------------------------------------------------------------

LONG = ["copies:%d" % b for b in (L - 1, L, L + 1, 4 * L + 3, 9 * L)] + ["run:%d" % (2 * L)]


def _largest_claim(ora):
    r = int(np.argmax(ora["lcpfull"]))
    assert np.count_nonzero(ora["lcpfull"] == ora["lcpfull"][r]) == 1
    return r, int(ora["lcpfull"][r])


@pytest.mark.parametrize("name", LONG)
def test_long_claims_are_accepted(checker, name):
    enc, ora = _oracle(name)
    res = checker.check(enc, ora["suf"], ora["lcp"], ora["llv"], ora["bwt"])
    _accepted(res, ora)
    r, v = _largest_claim(ora)
    # two copies: the second one starts behind a wildcard, its range is the whole
    # block; the run: position 1 inherits nothing from position 0 (row 0)
    assert res.long_claims == (1 if v > L else 0)


@pytest.mark.parametrize("name", LONG)
@pytest.mark.parametrize("delta", [1, -1])
def test_long_claim_off_by_one_is_rejected(checker, name, delta):
    enc, suf, lcp, llv, bwt = _tables(name)
    r, v = _largest_claim(_oracle(name)[1])
    j = int(np.flatnonzero(llv[:, 0] == r)[0])         # (L - 1 >= 255: the value is in .llv)
    llv[j, 1] = v + delta
    res = checker.check(enc, suf, lcp, llv, bwt)
    assert not res.ok and res.table == check.LLV and res.index == r and res.llv_entry == j, res
    assert res.criterion == (check.CRIT_LCP_LARGE if delta > 0 else check.CRIT_LCP_SMALL)
    assert (res.claimed, res.found) == (v + delta, v)
    assert (res.pos_a, res.pos_b) == (suf[r - 1], suf[r])
    assert ("too large" if delta > 0 else "too small") in res.message and "index %d " % r in res.message


# ---- rejections: LCP, LLV, BWT ---------------------------------------------------------

PLAIN = "dna:%d" % (3 * T + 5)
MANY = "copies:%d" % (255 + 300)


def _rows(N, lcp):
    """first, a middle and the last table index with a byte that can go both ways
    (the byte of the last rows of a table is 0: the nearest one that is not)"""
    ok = np.flatnonzero((lcp >= 1) & (lcp <= 253))
    return sorted({int(ok[np.argmin(np.abs(ok - want))]) for want in (1, T, N // 2, N - 1)})


@pytest.mark.parametrize("delta", [1, -1])
def test_lcp_byte_off_by_one_is_rejected(checker, delta):
    enc, suf, lcp0, llv, bwt = _tables(PLAIN)
    rows = _rows(suf.size, lcp0)
    assert len(rows) >= 3
    for r in rows + ([suf.size - 1] if delta > 0 else []):
        lcp = lcp0.copy()
        lcp[r] = int(lcp0[r]) + delta
        res = checker.check(enc, suf, lcp, llv, bwt)
        assert not res.ok and res.table == check.LCP and res.index == r, (r, res)
        assert res.criterion == (check.CRIT_LCP_LARGE if delta > 0 else check.CRIT_LCP_SMALL)
        assert (res.claimed, res.found) == (int(lcp0[r]) + delta, int(lcp0[r]))


def test_lcp_first_byte_is_rejected(checker):
    enc, suf, lcp, llv, bwt = _tables(PLAIN)
    lcp[0] = 1
    res = checker.check(enc, suf, lcp, llv, bwt)
    assert not res.ok and (res.table, res.criterion, res.index) == (check.LCP, check.CRIT_LCP0, 0), res


def test_llv_structure_is_rejected(checker):
    enc, suf, lcp0, llv0, bwt = _tables(MANY)
    n, m = enc.size, len(llv0)
    assert m == 301
    j = m // 2
    # a byte 255 without an entry
    r = int(np.flatnonzero(lcp0 < 255)[T // 3])
    lcp = lcp0.copy()
    lcp[r] = 255
    res = checker.check(enc, suf, lcp, llv0, bwt)
    assert not res.ok and (res.table, res.criterion, res.index) == (check.LLV, check.CRIT_LLV_MISSING, r), res
    assert res.llv_entry == np.searchsorted(llv0[:, 0], r) and (res.claimed, res.found) == (m, m + 1)
    # an entry removed
    res = checker.check(enc, suf, lcp0, np.delete(llv0, j, axis=0), bwt)
    assert not res.ok and (res.table, res.criterion) == (check.LLV, check.CRIT_LLV_MISSING), res
    assert (res.index, res.llv_entry) == (llv0[j, 0], j)
    # indices that do not ascend
    llv = llv0.copy()
    llv[[j, j + 1]] = llv0[[j + 1, j]]
    res = checker.check(enc, suf, lcp0, llv, bwt)
    assert not res.ok and (res.table, res.criterion) == (check.LLV, check.CRIT_LLV_ENTRY), res
    assert (res.llv_entry, res.index) == (j + 1, llv0[j, 0])
    # values outside [255, n], an index outside the table
    for col, value in ((1, 254), (1, n + 1), (0, n + 1), (0, 0)):
        for k in (0, j, m - 1):
            llv = llv0.copy()
            llv[k, col] = value
            res = checker.check(enc, suf, lcp0, llv, bwt)
            assert not res.ok and (res.table, res.criterion) == (check.LLV, check.CRIT_LLV_ENTRY), res
            assert (res.llv_entry, res.index, res.claimed) == (k, llv[k, 0], llv[k, 1]), (col, value, k, res)
    # an entry, in ascending order, that names a byte which is not 255
    nxt = np.append(llv0[1:, 0], n + 1)
    k = int(np.flatnonzero(nxt > llv0[:, 0] + 1)[0])
    llv = llv0.copy()
    llv[k, 0] += 1
    assert lcp0[llv[k, 0]] != 255
    res = checker.check(enc, suf, lcp0, llv, bwt)
    assert not res.ok and (res.table, res.criterion) == (check.LLV, check.CRIT_LLV_ENTRY), res
    assert (res.llv_entry, res.index) == (k, llv[k, 0])


def test_bwt_byte_is_rejected(checker):
    enc, suf, lcp, llv, bwt0 = _tables("specials:%d" % (3 * T + 5))
    N = suf.size
    for r in (0, T - 1, T, N // 2, N - 1, int(np.flatnonzero(suf == 0)[0])):
        bwt = bwt0.copy()
        bwt[r] = 0 if bwt0[r] >= 254 else (bwt0[r] + 1) % 4
        res = checker.check(enc, suf, lcp, llv, bwt)
        assert not res.ok and (res.table, res.criterion, res.index) == (check.BWT, check.CRIT_BWT, r), res
        assert (res.claimed, res.found, res.pos_b) == (bwt[r], bwt0[r], suf[r])


# ---- rejections: SUF ----------------------------------------------------------------------

def _torch_rejects(enc, suf):
    import torch
    sa = torch.from_numpy(suf.astype(np.uint64).view(np.int64).copy())
    ok, _ = dc.check_suffix_array_exact(sa, torch.from_numpy(enc.copy()))
    return not ok


def _suf_damages(width):
    enc, suf0, _, _, _ = _tables(PLAIN)
    n, N = enc.size, suf0.size
    suf0 = suf0.astype(width)
    big = (1 << 32) - 1 if width == np.uint32 else 1 << 40
    for what, rows, values in (
            ("n + 1", [T + 3], [n + 1]), ("beyond 32 bits", [2 * T], [big]), ("first", [0], [n + 1]),
            ("duplicate", [T], [suf0[5]]),
            ("swap at a tile border", [T - 1, T], [suf0[T], suf0[T - 1]]),
            ("swap of the last two", [N - 2, N - 1], [suf0[N - 1], suf0[N - 2]])):
        suf = suf0.copy()
        suf[rows] = values
        yield what, enc, suf


@pytest.mark.parametrize("width", [np.uint64, np.uint32])
def test_suffix_table_damage_is_rejected(checker, width):
    seen = set()
    for what, enc, suf in _suf_damages(width):
        crit, index = first_suf_failure(enc, suf)
        assert crit != check.CRIT_NONE, what
        seen.add(crit)
        res = checker.check(enc, suf)
        assert not res.ok and res.table == check.SUF, (what, res)
        assert (res.criterion, res.index) == (crit, index), (what, res)
        assert res.message.startswith("suf: ")
        assert _torch_rejects(enc, suf), what
    assert seen == {check.CRIT_RANGE, check.CRIT_PERM, check.CRIT_ORDER}


def test_damaged_suffix_table_ends_the_check_before_the_other_tables(checker):
    """phases 2 to 5 use the table as an index: they do not run on a damaged one"""
    enc, suf, lcp, llv, bwt = _tables(PLAIN)
    suf[T] = 1 << 40
    lcp[7] ^= 1
    bwt[9] ^= 1
    res = checker.check(enc, suf, lcp, llv, bwt)
    assert not res.ok and (res.table, res.criterion, res.index) == (check.SUF, check.CRIT_RANGE, T)
    assert res.phase_ms[0] > 0 and res.phase_ms[1:] == (0, 0, 0, 0)


# ---- the engine's resident tables ---------------------------------------------------------------

@pytest.mark.parametrize("readmode", [0, 3])
def test_engine_tables_are_accepted(checker, readmode):
    import torch
    enc = synth.generate(synth.MODEL_HUMANLIKE_DNA, 43, 300000)
    want = esa.WANT_SUF | esa.WANT_LCP | esa.WANT_BWT
    read = ou.apply_readmode(enc, ("fwd", "rev", "cpl", "rcl")[readmode])
    d_enc = torch.from_numpy(read).to("cuda:0")
    torch.cuda.synchronize()
    with esa.EsaEngine(enc.size, 4) as eng:
        eng.set_readmode(readmode)
        eng.set_sequence(enc)
        eng.run(want)
        res = checker.check_engine(eng, d_enc.data_ptr(), enc.size, want)
        st = eng.stats()
        assert res.ok, res
        assert (res.longest, res.largelcpvalues, res.maxbranchdepth) == \
            (st["longest"], st["largelcpvalues"], st["maxbranchdepth"])
        assert res.check_ms > 0 and all(t > 0 for t in res.phase_ms)
        # the tables of the other strand are not those of this sequence
        if readmode:
            d_fwd = torch.from_numpy(enc).to("cuda:0")
            torch.cuda.synchronize()
            assert not checker.check_engine(eng, d_fwd.data_ptr(), enc.size, want).ok
        with pytest.raises(esa.EsaError, match="through the .suf table"):
            checker.check_engine(eng, d_enc.data_ptr(), enc.size, esa.WANT_LCP)
        with pytest.raises(esa.EsaError, match="not the whole table"):
            checker.check_engine(eng, d_enc.data_ptr(), enc.size - 1, want)
