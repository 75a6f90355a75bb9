"""The tie paths of the engine at the borders of their arithmetic
(tests/lcp_border_cases.py: 250, 255, 16 members, 4096 tied suffixes, the window steps of
the comparisons, the chunk starts).  Every build is compared entry by entry with the
CPU oracle and with what the probes imply by construction, and what GTAMD_DEBUG says
of the path -- the direct calls, the figures of the pair path, its records and chunk,
the rounds -- is compared with the model's prediction, which is made from the
oracle's tables alone."""
import re

import numpy as np
import pytest

import engine_paths
import lcp_border_cases as cases
from genometools_amd import esa
from thread_comm import build_in_parts

pytestmark = pytest.mark.gpu

BASE = {"narrow": {}, "wide": {"GTAMD_FORCE_WIDE": "1"}, "msd": {"GTAMD_MSD": "1"}}
_SLICE = re.compile(r"slice (\d+) entries at (\d+)")


def _assert_same_as_oracle(t, suf, lcp, llv, bwt, stats):
    """(as test_esa_gpu._assert_same_as_oracle, for assembled tables as well)"""
    ora = t.ora
    assert np.array_equal(suf, ora["suf"]), "suf"
    assert np.array_equal(bwt, ora["bwt"]), "bwt"
    assert np.array_equal(lcp, ora["lcp"]), "lcp"
    assert np.array_equal(llv, ora["llv"]), "llv"
    st = ora["stats"]
    assert stats["longest"] == st["longest"]
    assert stats["largelcpvalues"] == st["largelcpvalues"]
    assert stats["maxbranchdepth"] == st["maxbranchdepth"]
    assert stats["lcptabsum"] == int(st["lcptabsum"])
    assert stats["prefixlength"] == st["prefixlength"]
    # the second, independent statement: what the probes are made of
    assert cases.check_by_construction(t, suf, cases.lcpfull_of(lcp, llv)) > 0


def _build(t, monkeypatch, capfd, env):
    """one whole-table build under `env`: tables against the oracle, the path against
    the model; returns (what the engine reported, the prediction)"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("GTAMD_DEBUG", "1")
    capfd.readouterr()
    res = esa.suffixerator_tables(t.enc, t.sigma)
    p = engine_paths.single(capfd.readouterr().err)
    _assert_same_as_oracle(t, res.suf, res.lcp, res.llv, res.bwt, res.stats)
    wide = env.get("GTAMD_FORCE_WIDE") == "1"
    msd = env.get("GTAMD_MSD") == "1" and not wide       # (64-bit positions: the sort of the parts)
    assert p["run"]["positions"] == (64 if wide else 32)
    assert p["run"]["first_sort"] == ("msd" if msd or (wide and t.sigma == 4) else "lsd")
    pred = cases.predict(t.enc, t.sigma, t.ora, msd=msd, dist=wide,
                         no_pairs=env.get("GTAMD_NO_PAIRS") == "1",
                         no_small=env.get("GTAMD_NO_SMALL_GROUPS") == "1",
                         pair_chunk=int(env.get("GTAMD_PAIR_CHUNK", 0)))
    assert p["direct"] == pred["direct"]
    assert p["ties"] == pred["ties"]
    if pred["pair_resolve"] is None:
        assert p["pair_resolve"] is None
    else:
        assert p["pair_resolve"] is not None
        assert {k: p["pair_resolve"][k] for k in ("records", "chunk")} == pred["pair_resolve"]
    assert (p["rounds"] > 0) == pred["rounds"] and (res.stats["refine_rounds"] > 0) == pred["rounds"]
    return p, pred


@pytest.mark.parametrize("base", sorted(BASE))
@pytest.mark.parametrize("name", cases.NAMES)
def test_every_text_on_its_path(gpu, monkeypatch, capfd, name, base):
    """32-bit and 64-bit positions, the tie bitmap of k_tiebits and of level D"""
    t = cases.text(name)
    _, pred = _build(t, monkeypatch, capfd, BASE[base])
    if base == "narrow":
        assert cases.path_of(pred) == cases.EXPECTED_PATH[name]


@pytest.mark.parametrize("chunk", ["16", "64"])
@pytest.mark.parametrize("name", ["pairs", "small"])
def test_pair_chunks(gpu, monkeypatch, capfd, name, chunk):
    """other records are fresh comparisons under each chunk"""
    p, pred = _build(cases.text(name), monkeypatch, capfd, {"GTAMD_PAIR_CHUNK": chunk})
    assert p["switches"]["pair_chunk"] == int(chunk) and pred["pair_resolve"]["chunk"] == int(chunk)


@pytest.mark.parametrize("switch", ["GTAMD_NO_PAIRS", "GTAMD_NO_SMALL_GROUPS"])
@pytest.mark.parametrize("name", ["pairs", "small", "deep_250"])
def test_without_the_pair_path_or_the_small_groups(gpu, monkeypatch, capfd, name, switch):
    """everything, or the groups of three and four, through the rounds and k_lcp_chunks"""
    p, pred = _build(cases.text(name), monkeypatch, capfd, {switch: "1"})
    assert p["switches"][switch[6:].lower()] == 1
    assert pred["ties"]["small_groups"] == 0
    if switch == "GTAMD_NO_PAIRS":
        assert pred["ties"]["pairs"] == 0 and pred["pair_resolve"] is None and pred["rounds"]


@pytest.mark.parametrize("apply_early", ["0", "1", "2"])
def test_pairs_with_every_placement_of_their_entries(gpu, monkeypatch, capfd, apply_early):
    """the LCP values beyond the byte in a buffer of their own, or where the rank table was"""
    p, _ = _build(cases.text("pairs"), monkeypatch, capfd, {"GTAMD_APPLY_EARLY": apply_early})
    assert [a["placement"] for a in p["apply"]] == [int(apply_early)]


@pytest.mark.parametrize("parts", [2, 3])
@pytest.mark.parametrize("name", ["pairs", "small", "rounds", "deep_250"])
def test_in_parts(gpu, monkeypatch, capfd, name, parts):
    """a part sees every R-th position of a repeat (p - prevp > 1 in k_lcp_chunks), the
    parts agree on the direct path, nothing is settled behind the pair path"""
    t = cases.text(name)
    monkeypatch.setenv("GTAMD_DEBUG", "1")
    capfd.readouterr()
    tabs, stats, _ = build_in_parts(t.enc, t.sigma, parts)
    per_part = engine_paths.parse(capfd.readouterr().err)
    assert sorted(per_part) == list(range(parts))
    _assert_same_as_oracle(t, tabs["suf"], tabs["lcp"], tabs["llv"], tabs["bwt"], stats)
    slices = []
    for r in range(parts):
        m = _SLICE.search(per_part[r]["tile"])
        slices.append((int(m.group(2)), int(m.group(1))))
    pred = cases.predict(t.enc, t.sigma, t.ora, slices=slices)
    assert pred["ties"] is not None
    for k in ("tied", "pairs", "small_groups", "settled", "left"):
        assert sum(p["ties"][k] for p in per_part.values()) == pred["ties"][k], k
    calls = [c for p in per_part.values() for c in p["direct"]]
    assert all(c["call"] == "first" for c in calls)          # (settle_few_left is skipped)
    if calls:                                                 # (all parts try, or none)
        assert len(calls) == parts and sum(c["tied"] for c in calls) == pred["members"]
        assert any(c["gaveup"] for c in calls)
    assert (max(p["rounds"] for p in per_part.values()) > 0) == pred["rounds"]
    if name in ("rounds", "deep_250"):
        assert pred["rounds"]
        seen = cases.chunks_model(t.enc, t.sigma, t.ora, pred, slices=slices)["classes"]
        assert "chunks:p - prevp > 1" in seen


def test_a_run_that_gave_up_leaves_nothing_to_the_next(gpu, monkeypatch, capfd):
    """one context: the direct path settles a text, gives up on the next (too deep, too
    big a group) or is not asked at all, and settles the first text again -- dfallback,
    dsum and dmax of a run must not reach the next one"""
    names = ["direct", "rounds", "direct", "group_17", "direct", "deep_250", "direct"]
    monkeypatch.setenv("GTAMD_DEBUG", "1")
    with esa.EsaEngine(max(cases.text(n).enc.size for n in names), 4) as eng:
        for name in names:
            t = cases.text(name)
            capfd.readouterr()
            eng.set_sequence(t.enc)
            eng.run()
            res = eng.result()
            p = engine_paths.single(capfd.readouterr().err)
            _assert_same_as_oracle(t, res.suf, res.lcp, res.llv, res.bwt, res.stats)
            assert p["direct"] == cases.predict(t.enc, 4, t.ora)["direct"], name
