"""Pairs in the wrong order never change places in the engine's suffix array;
their .suf/.bwt entries are swapped when they are written (k_pair_apply, beside
the doubling rounds or behind them).  Every walk that ranks the table's entries
by their index takes the resolved order from the bitmaps of k_pair_swapbits:
the rank table of the selected windows (k_win_filter), the whole table
(k_heads, the partition pass that makes the heads on the fly) and the first ranks
of a part build.  (Windows added between rounds need windows of 2^2 positions:
test_parts_gpu.test_deep_groups_reach_new_rank_windows.)  These inputs make the
order of a deep tie group depend on the ranks of pair members, at every place
of the flow."""
import numpy as np
import pytest

import engine_paths
import oracle_util as ou
from genometools_amd import esa
from thread_comm import build_in_parts

pytestmark = pytest.mark.gpu


def _same_as_oracle(enc, sigma, suf, lcp, llv, bwt, stats):
    ora = ou.esa(enc, sigma)
    assert np.array_equal(suf, ora["suf"]), "suf"
    assert np.array_equal(bwt, ora["bwt"]), "bwt"
    assert np.array_equal(lcp, ora["lcp"]), "lcp"
    assert np.array_equal(llv, ora["llv"]), "llv"
    st = ora["stats"]
    assert stats["longest"] == st["longest"]
    assert stats["largelcpvalues"] == st["largelcpvalues"]
    assert stats["maxbranchdepth"] == st["maxbranchdepth"]
    assert stats["lcptabsum"] == int(st["lcptabsum"])


def _single(enc, sigma, capfd=None):
    """the build against the oracle; with `capfd` (and GTAMD_DEBUG set): also what
    it reports (engine_paths)"""
    if capfd is not None:
        capfd.readouterr()
    res = esa.suffixerator_tables(enc, sigma)
    p = engine_paths.single(capfd.readouterr().err) if capfd is not None else None
    _same_as_oracle(enc, sigma, res.suf, res.lcp, res.llv, res.bwt, res.stats)
    return (res.stats, p) if capfd is not None else res.stats


def _parts(monkeypatch, capfd, enc, parts):
    monkeypatch.setenv("GTAMD_DEBUG", "1")
    capfd.readouterr()
    tabs, stats, _ = build_in_parts(enc, 4, parts)
    per_part = engine_paths.parse(capfd.readouterr().err)
    assert sorted(per_part) == list(range(parts))
    _same_as_oracle(enc, 4, tabs["suf"], tabs["lcp"], tabs["llv"], tabs["bwt"], stats)
    return per_part


def _targets_text(seed, copies=6, alen=2500, tail=60_000):
    """A block A in `copies` copies (a tie group of more than four: the rounds
    take it), each copy followed by one of two copies of a block B_k and a
    random stretch: the suffixes inside the B_k are pairs, swapped or not as
    the stretches behind them decide, and they are the look-up targets p + h of
    the rounds that order the copies of A"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 4, alen, dtype=np.uint8)
    parts = [rng.integers(0, 4, 3000, dtype=np.uint8)]
    bs = [rng.integers(0, 4, 900, dtype=np.uint8) for _ in range((copies + 1) // 2)]
    for k in range(copies):
        parts += [a, bs[k // 2], rng.integers(0, 4, 700, dtype=np.uint8)]
    parts.append(rng.integers(0, 4, tail, dtype=np.uint8))
    return np.concatenate(parts).astype(np.uint8)


@pytest.mark.parametrize("apply_early", ["0", "1", "2"])
@pytest.mark.parametrize("wbits,all_windows", [(None, "0"), (6, "0"), (6, "1"), (9, "0")])
def test_swapped_pairs_as_lookup_targets(gpu, monkeypatch, capfd, apply_early, wbits, all_windows):
    """the whole table with the heads as an array (default window) or made in the
    partition pass (small windows, whole table), the selected windows (small
    windows), with the pairs' entries behind the rounds or beside them"""
    monkeypatch.setenv("GTAMD_APPLY_EARLY", apply_early)
    monkeypatch.setenv("GTAMD_RANK_ALL_WINDOWS", all_windows)
    if wbits is not None:
        monkeypatch.setenv("GTAMD_RANK_WINDOW_BITS", str(wbits))
    monkeypatch.setenv("GTAMD_DEBUG", "1")
    enc = _targets_text(7 + (wbits or 0))
    st, p = _single(enc, 4, capfd)
    sw = p["switches"]
    assert sw["apply_early"] == int(apply_early) and sw["rank_all_windows"] == int(all_windows)
    assert sw["rank_window_bits"] == (wbits or 15)
    assert [a["placement"] for a in p["apply"]] == [int(apply_early)] and p["apply"][0]["pair_grid"] > 0
    if all_windows == "1":
        assert p["rank_whole"] and not p["rank_windows"]
    elif wbits is not None:
        assert p["rank_windows"] and not p["rank_windows"][0]["whole"]
    assert st["refine_rounds"] > 0
    assert st["pair_suffixes"] > 1000


@pytest.mark.parametrize("lds", ["1", "0"])
def test_swapped_pairs_with_the_window_bitmap_in_global_memory(gpu, monkeypatch, capfd, lds):
    monkeypatch.setenv("GTAMD_RANK_WINDOW_BITS", "8")
    monkeypatch.setenv("GTAMD_WIN_FILTER_LDS", lds)
    monkeypatch.setenv("GTAMD_DEBUG", "1")
    enc = _targets_text(21, copies=8)
    st, p = _single(enc, 4, capfd)
    assert p["switches"]["win_filter_global"] == int(lds == "0") and p["win_filter"]
    assert all(w["bitmap"] == ("global" if lds == "0" else "lds") for w in p["win_filter"])
    assert st["refine_rounds"] > 0


def test_swapped_pairs_with_wide_positions(gpu, monkeypatch, capfd):
    monkeypatch.setenv("GTAMD_FORCE_WIDE", "1")
    monkeypatch.setenv("GTAMD_DEBUG", "1")
    enc = _targets_text(5)
    _, p = _single(enc, 4, capfd)
    assert p["switches"]["force_wide"] == 1 and p["run"]["positions"] == 64


def test_pair_next_to_a_round_group(gpu):
    """a copy of A with one change a few symbols in: its suffixes there are pairs
    whose keys follow those of A's group in the table -- the LCP between a pair's
    entry and the group beside it"""
    rng = np.random.default_rng(3)
    a = rng.integers(0, 4, 3000, dtype=np.uint8)
    a2 = a.copy()
    a2[40] = (a2[40] + 1) & 3
    parts = [rng.integers(0, 4, 2000, dtype=np.uint8)]
    for blk in (a, a, a, a, a, a2, a2):
        parts += [blk, rng.integers(0, 4, 500, dtype=np.uint8)]
    parts.append(rng.integers(0, 4, 40_000, dtype=np.uint8))
    enc = np.concatenate(parts).astype(np.uint8)
    st = _single(enc, 4)
    assert st["refine_rounds"] > 0


@pytest.mark.parametrize("n", [70_337, 70_337 + 31, 70_400])
@pytest.mark.parametrize("all_windows", ["0", "1"])
def test_pairs_in_the_last_word_of_the_table(gpu, monkeypatch, capfd, n, all_windows):
    """the largest suffixes are pairs -- two copies of a block over {G, T} in a
    text over {A, C, G} -- so that they fill the last bitmap word of the table;
    a deep group of A copies makes the rounds (and the rank table) run"""
    monkeypatch.setenv("GTAMD_RANK_WINDOW_BITS", "6")
    monkeypatch.setenv("GTAMD_RANK_ALL_WINDOWS", all_windows)
    rng = np.random.default_rng(n)
    enc = rng.integers(0, 3, n, dtype=np.uint8)
    blk = rng.integers(2, 4, 400, dtype=np.uint8)
    blk[::3] = 3
    enc[n // 3:n // 3 + 400] = blk
    enc[n - 400:] = blk                                 # (the second copy ends the text)
    a = enc[1000:3000].copy()
    for at in (n // 2, n // 2 + 2500, n // 2 + 5000, n // 2 + 7500, n // 2 + 10000):
        enc[at:at + 2000] = a
    monkeypatch.setenv("GTAMD_DEBUG", "1")
    st, p = _single(enc, 4, capfd)
    assert p["switches"]["rank_window_bits"] == 6
    assert p["switches"]["rank_all_windows"] == int(all_windows)
    if all_windows == "1":
        assert p["rank_whole"] and not p["rank_windows"]
    assert st["refine_rounds"] > 0


@pytest.mark.parametrize("parts", [2, 3])
@pytest.mark.parametrize("wbits", [None, 6])
def test_swapped_pairs_in_parts(gpu, monkeypatch, capfd, parts, wbits):
    """part builds: the first ranks that travel, listed by the filter"""
    if wbits is not None:
        monkeypatch.setenv("GTAMD_RANK_WINDOW_BITS", str(wbits))
    enc = _targets_text(11, copies=6, tail=150_000)
    per_part = _parts(monkeypatch, capfd, enc, parts)
    for p in per_part.values():
        assert p["switches"]["rank_window_bits"] == (wbits or 15) and p["run"]["parts"] == parts
        assert not p["rank_exchange_all"]
    assert any(p["win_filter"] for p in per_part.values())
    assert any(t["fresh"] > 0 for p in per_part.values() for t in p["ranks_travel"])


@pytest.mark.parametrize("parts", [1, 3])
def test_swapped_pairs_all_windows_in_parts(gpu, monkeypatch, capfd, parts):
    """part builds that send the first ranks of the whole slice, chunk by chunk"""
    monkeypatch.setenv("GTAMD_RANK_ALL_WINDOWS", "1")
    enc = _targets_text(13, copies=5)
    per_part = _parts(monkeypatch, capfd, enc, parts)
    for p in per_part.values():
        assert p["switches"]["rank_all_windows"] == 1
        assert not p["ranks_travel"] and not p["win_filter"]
    # (one part: a whole-table build, which builds the whole rank table)
    assert any(p["rank_exchange_all"] or p["rank_whole"] for p in per_part.values())
