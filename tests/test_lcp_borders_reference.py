"""The border cases of the tie paths (tests/lcp_border_cases.py) held to the CPU
oracle: what every probe implies by construction is in the oracle's tables, the model
sends every text down the path it is meant to take, and the cases reach every class
of alignment, window, decision and border they were made for.  No GPU: this file
fails when an edit of the cases loses a class."""
import numpy as np
import pytest

import lcp_border_cases as cases
import oracle_util as ou


@pytest.mark.parametrize("name", cases.NAMES)
def test_probes_are_in_the_oracle_tables(name):
    """every (a, b, LCP, order) of every probe; the copies stand together"""
    t = cases.text(name)
    assert t.enc.size <= 70_000
    assert cases.check_by_construction(t, t.ora["suf"], t.ora["lcpfull"]) > 0


@pytest.mark.parametrize("name", cases.NAMES)
def test_direct_lcp_equals_kasai(name):
    t = cases.text(name)
    direct = ou.esa(t.enc, t.sigma, kasai=False)
    assert np.array_equal(direct["lcpfull"], t.ora["lcpfull"])
    assert np.array_equal(direct["suf"], t.ora["suf"])


def test_overflow_bytes_at_every_place_of_a_group_of_16():
    """the entries of 255 over all texts occupy every i & 15 (llv_mask takes 16 entries
    at a time), and text `last_group` has one in the last, partial group of its table"""
    seen = set()
    for name in cases.NAMES:
        seen |= set(int(i) & 15 for i in np.flatnonzero(cases.text(name).ora["lcp"] == 255))
    assert seen == set(range(16))
    lcp = cases.text("last_group").ora["lcp"]
    assert lcp.size % 16 != 0
    assert (lcp[lcp.size - lcp.size % 16:] == 255).any()
    assert not (cases.text("last_group").enc >= cases.WILD).any()


def test_backgrounds_hold_no_known_mer_twice():
    for name in cases.NAMES:
        t = cases.text(name)
        assert not cases.has_repeated_kmer(t.bg, cases.KNOWN[t.sigma], t.sigma), name
        assert (40_000 if t.sigma == 4 else 20_000) <= t.bg.size <= (70_000 if t.sigma == 4 else 30_000)
    # (the check itself: a planted repeat is seen)
    bg = cases.text("direct").bg.copy()
    bg[30_000:30_020] = bg[100:120]
    assert cases.has_repeated_kmer(bg, 20, 4)
    assert not cases.has_repeated_kmer(cases.text("direct").bg, 20, 4)


@pytest.mark.parametrize("name", cases.NAMES)
def test_model_sends_the_text_down_its_path(name):
    t = cases.text(name)
    pred = cases.predict(t.enc, t.sigma, t.ora)
    assert cases.path_of(pred) == cases.EXPECTED_PATH[name]


def test_direct_limit_texts_differ_by_one_member():
    a, b = cases.text("direct_count_4096"), cases.text("direct_count_4097")
    pa, pb = cases.predict(a.enc, 4, a.ora), cases.predict(b.enc, 4, b.ora)
    assert pa["members"] == cases.DIRECT_LIMIT and pb["members"] == cases.DIRECT_LIMIT + 1
    for t in (a, b):            # all shallow: only the count can turn the direct path away
        assert t.ora["lcpfull"].max() < cases.DIRECT_MAX_LCP


def test_border_values_are_where_they_are_meant_to_be():
    d = cases.text("direct")
    assert d.ora["lcpfull"].max() == cases.DIRECT_MAX_LCP - 1
    deep = cases.text("deep_250")
    lf = deep.ora["lcpfull"]
    assert lf.max() == cases.DIRECT_MAX_LCP and np.count_nonzero(lf == cases.DIRECT_MAX_LCP) == 1
    pred = cases.predict(deep.enc, 4, deep.ora)
    left = pred["sizes"][pred["is_left"]]
    assert left.min() >= 5 and left.max() <= cases.DIRECT_MAX_GROUP
    g17 = cases.text("group_17")
    p17 = cases.predict(g17.enc, 4, g17.ora)
    assert p17["sizes"].max() == 17 and g17.ora["lcpfull"].max() < cases.DIRECT_MAX_LCP
    s = cases.text("small")
    ps = cases.predict(s.enc, 4, s.ora)
    assert ps["ties"]["small_groups"] > 1000 and ps["ties"]["left"] == 0
    # small groups whose pairwise LCPs differ, with 254 and 255 among them
    lf = s.ora["lcpfull"]
    mixed = [lf[h + 1:h + g] for h, g in zip(ps["heads"][ps["is_small"]], ps["sizes"][ps["is_small"]])
             if lf[h + 1:h + g].min() != lf[h + 1:h + g].max()]
    assert any(254 in m for m in mixed) and any(255 in m for m in mixed) and any(20 in m for m in mixed)
    for name in ("pairs", "rounds", "protein"):
        lf = cases.text(name).ora["lcpfull"]
        for v in (249, 250, 254, 255, 256):
            assert (lf == v).any(), (name, v)


def test_small_groups_come_in_every_order():
    """the members of a group of three / four, taken in position order, stand in the
    sorted table in all 6 / 24 orders"""
    s = cases.text("small")
    ps = cases.predict(s.enc, 4, s.ora)
    suf = s.ora["suf"].astype(np.int64)
    orders = {3: set(), 4: set()}
    for h, g in zip(ps["heads"][ps["is_small"]], ps["sizes"][ps["is_small"]]):
        orders[int(g)].add(tuple(np.argsort(suf[h:h + g])))
    assert len(orders[3]) == 6 and len(orders[4]) == 24


@pytest.mark.parametrize("pair_chunk", [0, 16, 64])
def test_coverage_is_complete(pair_chunk):
    cov = cases.coverage(pair_chunk)
    reached = set().union(*cov.values())
    assert not (cases.REQUIRED - reached), sorted(cases.REQUIRED - reached)
    # a class no text can reach is named with its reason, and is really not reached
    for name, reason in cases.UNREACHABLE.items():
        assert name not in reached and len(reason) > 40
    assert reached <= cases.REQUIRED | set(cases.UNREACHABLE)


def test_different_records_are_fresh_under_each_chunk():
    t = cases.text("pairs")
    fresh = {}
    for chunk in (16, 64):
        pred = cases.predict(t.enc, 4, t.ora, pair_chunk=chunk)
        assert pred["pair_resolve"]["chunk"] == chunk
        fresh[chunk] = cases.resolve_model(t.enc, 4, t.ora, pred)["fresh"]
    assert fresh[16].sum() > fresh[64].sum() > 0
    assert (fresh[16] | ~fresh[64]).all()        # (a chunk start of 64 is one of 16)


def test_protein_tie_rule_of_the_msd_sort_differs():
    """eight symbols and the class of the ninth tie more suffixes than ten symbols"""
    t = cases.text("protein")
    lsd = cases.predict(t.enc, 20, t.ora)
    msd = cases.predict(t.enc, 20, t.ora, msd=True)
    assert msd["tied"] > lsd["tied"] > 0
