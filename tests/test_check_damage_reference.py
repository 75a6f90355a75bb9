"""The judge of tests/test_check_damage_gpu.py held to two other statements of
criterion 5 (include/gtamd_check.h), with no GPU: check_criteria.first_lcp_failure
finds no failure in the CPU oracle's tables, and it rejects every damaged table
of tests/check_damage_cases.py that tests/device_check.py::check_lcp_exact (torch,
here on the CPU) rejects -- which is all of them.  The coverage the cases claim
is asserted here too."""
import numpy as np
import pytest
import torch

import check_damage_cases as cd
import device_check as dc
from check_criteria import first_lcp_failure
from genometools_amd import check


def _torch_rejects(t, lcp, llv):
    sa = torch.from_numpy(t.suf.copy())
    idx = torch.from_numpy(llv[:, 0].astype(np.int64))
    val = torch.from_numpy(llv[:, 1].astype(np.int64))
    ok, _ = dc.check_lcp_exact(sa, torch.from_numpy(t.enc.copy()), torch.from_numpy(lcp.copy()), idx, val,
                               rank=torch.from_numpy(t.rank.copy()))
    return not ok


@pytest.mark.parametrize("name", cd.CASE_TEXTS + ["D", "specials:300", "protein:300"])
def test_oracle_tables_pass_the_judge(name):
    if name in cd.CASE_TEXTS + ["D"]:
        t = cd.text(name)
        enc, suf, lcp, llv = t.enc, t.ora["suf"], t.ora["lcp"], t.ora["llv"]
    else:
        import oracle_util as ou
        enc, _ = cd.order_text(name)
        ora = ou.esa(enc, 20 if name.startswith("protein") else 4)
        suf, lcp, llv = ora["suf"], ora["lcp"], ora["llv"]
    assert first_lcp_failure(enc, suf, lcp, llv) is None
    assert first_lcp_failure(enc, suf.astype(np.uint32), lcp, llv) is None


def test_cases_cover_every_class():
    seen = cd.assert_coverage()
    assert len(cd.all_cases()) == sum(v for k, v in seen.items() if k[0] == "table")


@pytest.mark.parametrize("name", cd.CASE_TEXTS)
def test_single_damage_is_rejected_by_judge_and_torch(name):
    t = cd.text(name)
    assert cd.cases(name)
    for c in cd.cases(name):
        lcp, llv = cd.damaged(c)
        got = first_lcp_failure(t.enc, t.ora["suf"], lcp, llv)
        # one damaged row: it is the one that fails, with its claim and the true value
        want = (check.LLV if c.in_llv else check.LCP,
                check.CRIT_LCP_SMALL if c.below else check.CRIT_LCP_LARGE, c.r,
                int(np.searchsorted(t.ora["llv"][:, 0], c.r)) if c.in_llv else check.NONE,
                c.claim, c.true, c.q, c.p)
        assert got == want, c
        assert _torch_rejects(t, lcp, llv), c


def test_double_damage_is_rejected_by_judge_and_torch():
    t = cd.text("A")
    first, second = 0, 0
    for what, damages in cd.double_damages():
        lcp, llv = cd.write_claims(t, damages)
        got = first_lcp_failure(t.enc, t.ora["suf"], lcp, llv)
        assert got is not None and got[2] in [r for r, _ in damages], (what, damages, got)
        assert got[4] == dict(damages)[got[2]] and got[5] == t.true[got[2]]
        first += got[2] == damages[0][0]
        second += got[2] == damages[1][0]
        assert _torch_rejects(t, lcp, llv), what
    assert first and second        # either row is the reported one in some table


def test_list_overflow_is_rejected_by_judge_and_torch():
    t = cd.text("A")
    rows = cd.overflow_rows(cd.list_cap(t) + 5)
    lcp, llv = cd.list_overflow(rows)
    got = first_lcp_failure(t.enc, t.ora["suf"], lcp, llv)
    assert got[:3] == (check.LLV, check.CRIT_LCP_LARGE, min(rows)) and got[4] == got[5] + 600
    assert _torch_rejects(t, lcp, llv)


def test_text_d_fills_the_work_list_past_its_workgroups():
    t = cd.text("D")
    rows, entry = cd.d_rows()
    assert t.enc.size == 1079400 and rows.size == 2099
    # three of the rows, damaged as the GPU test damages all of them
    for k in (0, 1000, 2098):
        llv = t.ora["llv"].copy()
        llv[entry[k], 1] = cd.D_CLAIM
        got = first_lcp_failure(t.enc, t.ora["suf"], t.ora["lcp"], llv)
        assert got == (check.LLV, check.CRIT_LCP_LARGE, rows[k], entry[k], cd.D_CLAIM, cd.D_BLOCK,
                       t.suf[rows[k] - 1], t.suf[rows[k]])
        assert cd.listed_positions(t, t.ora["lcp"], llv) == rows.size


def test_order_swaps_cover_what_decides_an_order():
    seen = cd.order_classes()
    assert {"two specials", "decided at a + 1 = n", "a letter against a special",
            "decided by the ranks", "two letters"} <= seen
