"""Phase 5 of the index checker (esa_check.hip) asked to FIND a mismatch: inside
a claimed prefix, in the middle of a range, under the word branch of first_bad16
and on the work list, with specials and at the borders of the sequence; and
phase 2 asked about every pair of neighbours of a small table.

The damaged tables and the model of which branch meets each mismatch are
tests/check_damage_cases.py; the expected report is check_criteria's judge
(first_lcp_failure, first_suf_failure), held to the oracle and to
device_check.check_lcp_exact by tests/test_check_damage_reference.py.  Every
expected table is the CPU oracle's, never the engine's."""
import collections

import numpy as np
import pytest

import check_damage_cases as cd
from check_criteria import first_lcp_failure, first_suf_failure
from genometools_amd import check

pytestmark = pytest.mark.gpu

WIDTHS = [np.uint64, np.uint32]
OVERFLOW_WINDOWS = 24
TALLY = collections.Counter()
FIELDS = ("table", "criterion", "index", "llv_entry", "claimed", "found", "pos_a", "pos_b")


@pytest.fixture(scope="module")
def checker(gpu):
    with check.EsaChecker() as c:
        assert (c.TILE, c.LONG_CLAIM) == (cd.TILE, cd.LONG)
        yield c


def _report(res):
    return tuple(getattr(res, f) for f in FIELDS)


def _rejected(res, want, what):
    assert want is not None, what
    assert not res.ok and _report(res) == tuple(int(v) for v in want), (what, want, res)
    assert "index %d " % want[2] in res.message, (what, res.message)
    assert ("too small" if want[1] == check.CRIT_LCP_SMALL else "too large") in res.message
    assert res.message.startswith("llv: " if want[0] == check.LLV else "lcp: ")


_expected = {}


def _judge(c):
    """the judge's report of a case; the same for both widths of .suf"""
    if (c.text, c.r, c.claim) not in _expected:
        t = cd.text(c.text)
        lcp, llv = cd.damaged(c)
        _expected[c.text, c.r, c.claim] = first_lcp_failure(t.enc, t.ora["suf"], lcp, llv)
    return _expected[c.text, c.r, c.claim]


# ---- one damaged value ---------------------------------------------------------------------

@pytest.mark.parametrize("name", cd.CASE_TEXTS)
@pytest.mark.parametrize("width", WIDTHS)
def test_every_single_damage_is_rejected(checker, name, width):
    t = cd.text(name)
    suf = t.ora["suf"].astype(width)
    res = checker.check(t.enc, suf, t.ora["lcp"], t.ora["llv"], t.ora["bwt"])
    assert res.ok and res.long_claims == cd.listed_positions(t, t.ora["lcp"], t.ora["llv"]), res
    for c in cd.cases(name):
        lcp, llv = cd.damaged(c)
        want = _judge(c)
        assert want[2:6] == (c.r, want[3], c.claim, c.true), (c, want)
        _rejected(checker.check(t.enc, suf, lcp, llv, t.ora["bwt"]), want, c)
        TALLY["single", np.dtype(width).itemsize] += 1


class _Resident:
    """tables in device memory, enc at an address of a chosen residue mod 4"""

    def __init__(self, skew, enc, suf, lcp, llv):
        import torch
        self.torch, self.keep, self.ptr = torch, [], []
        for a, k in ((enc, skew), (suf, 0), (lcp, 0), (np.ascontiguousarray(llv), 0)):
            b = torch.zeros(a.nbytes + 16, dtype=torch.uint8, device="cuda:0")
            assert b.data_ptr() % 16 == 0
            b[k:k + a.nbytes] = torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to("cuda:0")
            self.keep.append(b)
            self.ptr.append(b.data_ptr() + k)
        self.n, self.suf_bytes, self.pairs = enc.size, suf.dtype.itemsize, len(llv)
        self.lcp = self.keep[2]
        self.llv = self.keep[3][:16 * len(llv)].view(torch.int64)
        torch.cuda.synchronize()

    def check(self, checker):
        self.torch.cuda.synchronize()
        return checker.check_device(self.ptr[0], self.n, self.ptr[1], self.suf_bytes, self.ptr[2],
                                    self.ptr[3] if self.pairs else None, self.pairs)


def _skew_cases():
    """one case of the word branch for every pair of alignments and either path"""
    pick = {}
    for c in cd.all_cases():
        if c.branch == "word":
            pick.setdefault((c.path, c.ma, c.mb), c)
    assert len(pick) == 32
    return list(pick.values())


@pytest.mark.parametrize("skew", [0, 1, 2, 3])
def test_damage_is_rejected_at_every_address_skew(checker, skew):
    """check_device with enc at an address that is `skew` mod 4: the alignment of
    the words the kernel loads is that of the address, not of the position"""
    resident = {}
    for c in _skew_cases():
        t = cd.text(c.text)
        if c.text not in resident:
            resident[c.text] = _Resident(skew, t.enc, t.ora["suf"], t.ora["lcp"], t.ora["llv"])
        dev = resident[c.text]
        assert dev.check(checker).ok
        lcp, llv = cd.damaged(c)
        if c.in_llv:
            j = int(np.searchsorted(llv[:, 0], c.r))
            dev.llv[2 * j + 1] = c.claim
        else:
            dev.lcp[c.r] = c.claim
        res = dev.check(checker)
        if c.in_llv:
            dev.llv[2 * j + 1] = c.true
        else:
            dev.lcp[c.r] = c.true
        _rejected(res, _judge(c), (skew, c))
        TALLY["skew", skew] += 1


# ---- more than one damaged value -----------------------------------------------------------

@pytest.mark.parametrize("width", WIDTHS)
def test_two_damages_in_one_table(checker, width):
    t = cd.text("A")
    suf = t.ora["suf"].astype(width)
    for what, damages in cd.double_damages():
        lcp, llv = cd.write_claims(t, damages)
        want = first_lcp_failure(t.enc, t.ora["suf"], lcp, llv)
        assert want[2] in [r for r, _ in damages]
        _rejected(checker.check(t.enc, suf, lcp, llv, t.ora["bwt"]), want, (what, damages))
        TALLY["double"] += 1


@pytest.mark.parametrize("width", WIDTHS)
def test_more_long_claims_than_the_list_holds(checker, width):
    """the positions that find the work list full are compared by their lanes"""
    t = cd.text("A")
    cap = cd.list_cap(t)
    suf = t.ora["suf"].astype(width)
    rows = cd.overflow_rows(cap + 5)
    lcp, llv = cd.list_overflow(rows)
    want = first_lcp_failure(t.enc, t.ora["suf"], lcp, llv)
    assert want[2] == min(rows)
    res = checker.check(t.enc, suf, lcp, llv, t.ora["bwt"])
    _rejected(res, want, "list overflow")
    assert res.long_claims == len(rows) == cap + 5
    # which positions find the list full is the order of an atomic.  Twice as many
    # claims as the list holds, the window moved row by row: every window's
    # smallest row is reported, whether its position went to the list or not
    rows = cd.overflow_rows(2 * cap + OVERFLOW_WINDOWS)
    assert rows == sorted(rows)
    for k in range(OVERFLOW_WINDOWS):
        lcp, llv = cd.list_overflow(rows[k:k + 2 * cap])
        res = checker.check(t.enc, suf, lcp, llv, t.ora["bwt"])
        assert not res.ok and res.long_claims == 2 * cap, (k, res)
        assert (res.index, res.claimed, res.found) == (rows[k], t.true[rows[k]] + 600, t.true[rows[k]]), (k, res)
        TALLY["overflow"] += 1


# ---- text D: more listed positions than the work list's kernel has workgroups ---------------

@pytest.fixture(scope="module")
def text_d(checker):
    t = cd.text("D")
    rows, entry = cd.d_rows()
    dev = _Resident(0, t.enc, t.ora["suf"].astype(np.uint32), t.ora["lcp"], t.ora["llv"])
    yield t, rows, entry, dev


def test_text_d_is_accepted(checker, text_d):
    t, rows, entry, dev = text_d
    for width in WIDTHS:
        res = checker.check(t.enc, t.ora["suf"].astype(width), t.ora["lcp"], t.ora["llv"], t.ora["bwt"])
        assert res.ok and res.long_claims == rows.size == 2099 > 2048, res
        assert res.maxbranchdepth == t.ora["stats"]["maxbranchdepth"]
    res = dev.check(checker)
    assert res.ok and res.long_claims == 2099, res


def test_text_d_every_listed_row_damaged_in_turn(checker, text_d):
    """which slot of the list a position gets is the order of an atomic: only
    damaging every listed position makes the result independent of that order
    (2099 checks of 1 M entries in device memory: 2 s)"""
    t, rows, entry, dev = text_d
    for k in range(rows.size):
        r, j = int(rows[k]), int(entry[k])
        dev.llv[2 * j + 1] = cd.D_CLAIM
        res = dev.check(checker)
        dev.llv[2 * j + 1] = cd.D_BLOCK
        assert not res.ok and res.long_claims == rows.size, (k, res)
        assert _report(res) == (check.LLV, check.CRIT_LCP_LARGE, r, j, cd.D_CLAIM, cd.D_BLOCK,
                                t.suf[r - 1], t.suf[r]), (k, res)
        TALLY["D"] += 1


# ---- order damage ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["specials:300", "protein:300"])
@pytest.mark.parametrize("width", WIDTHS)
def test_every_swap_of_rows_is_rejected(checker, name, width):
    enc, suf0, swaps = cd.order_swaps(name)
    assert checker.check(enc, suf0.astype(width)).ok
    for i, j in swaps:
        suf = suf0.astype(width)
        suf[[i, j]] = suf0[[j, i]]
        crit, at = first_suf_failure(enc, suf)
        assert crit == check.CRIT_ORDER
        res = checker.check(enc, suf)
        assert not res.ok and (res.table, res.criterion, res.index) == (check.SUF, crit, at), (i, j, res)
        assert (res.pos_a, res.pos_b) == (suf[at - 1], suf[at]), (i, j, res)
        assert "index %d " % at in res.message
        TALLY["swap", name] += 1


# ---------------------------------------------------------------------------
def test_every_case_ran():
    """judges the run of the whole module: the cases run are the cases generated"""
    want = collections.Counter()
    for width in WIDTHS:
        want["single", np.dtype(width).itemsize] = len(cd.all_cases())
    for skew in range(4):
        want["skew", skew] = 32
    want["double"] = len(WIDTHS) * len(cd.double_damages())
    want["overflow"] = len(WIDTHS) * OVERFLOW_WINDOWS
    want["D"] = 2099
    for name in ("specials:300", "protein:300"):
        want["swap", name] = len(WIDTHS) * (300 + 100)
    assert len(cd.all_cases()) > 1400 and len(cd.double_damages()) >= 12
    assert TALLY == want, (TALLY - want, want - TALLY)
