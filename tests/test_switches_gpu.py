"""The engine's switches (read_switches(), genometools_amd/csrc/esa_engine.hip):
how each one is parsed, the four that only the fuzzer used to set, at their
edges against the oracle, and the fuzzer's combinations replayed with fixed
seeds.  Every build here also asserts, from the GTAMD_DEBUG lines, that the
path it forces ran (engine_paths.py)."""
import numpy as np
import pytest

import engine_paths
import oracle_util as ou
from fuzz_cases import msd_switches, parts_switches, prefix_length, random_sequence
from genometools_amd import esa, synth
from test_esa_gpu import _assert_same_as_oracle
from thread_comm import build_in_parts

pytestmark = pytest.mark.gpu


@pytest.fixture
def debug(monkeypatch, capfd):
    monkeypatch.setenv("GTAMD_DEBUG", "1")
    capfd.readouterr()
    return monkeypatch


def _run(capfd, enc, sigma=4):
    capfd.readouterr()
    res = esa.suffixerator_tables(enc, sigma)
    return res, engine_paths.single(capfd.readouterr().err)


# ---------------------------------------------------------------------------
# parse rules: a value inside the range, both ends, one value just outside each
# end (the default, or the documented fall-back)
# ---------------------------------------------------------------------------
_DEF = {"msd": -1, "msd_part_off": 0, "msd_cbits": -1, "msd_big_max": 524288, "msd_radix": 0,
        "msd_pack": 1, "msd_pack_cap": 4096, "msd_bin_limit": 128, "fused_pass0": 1, "force_wide": 0,
        "no_pairs": 0, "no_small_groups": 0, "apply_early": 2, "apply_wgs": 0, "apply_wgs_given": 0,
        "rank_window_bits": 15, "rank_all_windows": 0, "win_filter_global": 0, "pair_chunk": 0,
        "round_stride": 1536}

PARSE = [
    # (variable, value, {field: effective value})
    ("GTAMD_MSD", "1", {"msd": 1, "msd_part_off": 0}),
    ("GTAMD_MSD", "0", {"msd": 0, "msd_part_off": 1}),
    ("GTAMD_MSD", "2", {"msd": 0, "msd_part_off": 0}),          # (any other value: the LSD sort)
    ("GTAMD_MSD_CBITS", "4", {"msd_cbits": 4}),
    ("GTAMD_MSD_CBITS", "0", {"msd_cbits": 0}),
    ("GTAMD_MSD_CBITS", "8", {"msd_cbits": 8}),
    ("GTAMD_MSD_CBITS", "-1", {"msd_cbits": -1}),
    ("GTAMD_MSD_CBITS", "9", {"msd_cbits": -1}),
    ("GTAMD_MSD_BIG_MAX", "8192", {"msd_big_max": 8192}),
    ("GTAMD_MSD_BIG_MAX", "4096", {"msd_big_max": 4096}),
    ("GTAMD_MSD_BIG_MAX", "524288", {"msd_big_max": 524288}),
    ("GTAMD_MSD_BIG_MAX", "4095", {"msd_big_max": 524288}),
    ("GTAMD_MSD_BIG_MAX", "524289", {"msd_big_max": 524288}),
    ("GTAMD_MSD_RADIX", "1", {"msd_radix": 1}),
    ("GTAMD_MSD_RADIX", "0", {"msd_radix": 0}),
    ("GTAMD_MSD_RADIX", "2", {"msd_radix": 0}),
    ("GTAMD_MSD_PACK", "0", {"msd_pack": 0}),
    ("GTAMD_MSD_PACK", "1", {"msd_pack": 1}),
    ("GTAMD_MSD_PACK", "7", {"msd_pack": 1}),
    ("GTAMD_MSD_PACK_CAP", "3000", {"msd_pack_cap": 3000}),
    ("GTAMD_MSD_PACK_CAP", "1024", {"msd_pack_cap": 1024}),
    ("GTAMD_MSD_PACK_CAP", "4096", {"msd_pack_cap": 4096}),
    ("GTAMD_MSD_PACK_CAP", "1023", {"msd_pack_cap": 4096}),
    ("GTAMD_MSD_PACK_CAP", "4097", {"msd_pack_cap": 4096}),
    ("GTAMD_MSD_BIN_LIMIT", "16", {"msd_bin_limit": 16}),
    ("GTAMD_MSD_BIN_LIMIT", "2", {"msd_bin_limit": 2}),
    ("GTAMD_MSD_BIN_LIMIT", "4096", {"msd_bin_limit": 4096}),
    ("GTAMD_MSD_BIN_LIMIT", "1", {"msd_bin_limit": 128}),
    ("GTAMD_MSD_BIN_LIMIT", "4097", {"msd_bin_limit": 128}),
    ("GTAMD_FUSED_PASS0", "0", {"fused_pass0": 0}),
    ("GTAMD_FUSED_PASS0", "1", {"fused_pass0": 1}),
    ("GTAMD_FUSED_PASS0", "x", {"fused_pass0": 1}),
    ("GTAMD_FORCE_WIDE", "1", {"force_wide": 1}),
    ("GTAMD_FORCE_WIDE", "0", {"force_wide": 0}),
    ("GTAMD_FORCE_WIDE", "2", {"force_wide": 0}),
    ("GTAMD_NO_PAIRS", "1", {"no_pairs": 1}),
    ("GTAMD_NO_PAIRS", "0", {"no_pairs": 0}),
    ("GTAMD_NO_PAIRS", "2", {"no_pairs": 0}),
    ("GTAMD_NO_SMALL_GROUPS", "1", {"no_small_groups": 1}),
    ("GTAMD_NO_SMALL_GROUPS", "0", {"no_small_groups": 0}),
    ("GTAMD_NO_SMALL_GROUPS", "2", {"no_small_groups": 0}),
    ("GTAMD_APPLY_EARLY", "1", {"apply_early": 1}),
    ("GTAMD_APPLY_EARLY", "0", {"apply_early": 0}),
    ("GTAMD_APPLY_EARLY", "2", {"apply_early": 2}),
    ("GTAMD_APPLY_EARLY", "-1", {"apply_early": 0}),              # (out of range: 0, not the default)
    ("GTAMD_APPLY_EARLY", "3", {"apply_early": 0}),
    ("GTAMD_APPLY_WGS", "1000", {"apply_wgs": 1000, "apply_wgs_given": 1}),
    ("GTAMD_APPLY_WGS", "64", {"apply_wgs": 64, "apply_wgs_given": 1}),
    ("GTAMD_APPLY_WGS", "4194304", {"apply_wgs": 4194304, "apply_wgs_given": 1}),
    ("GTAMD_APPLY_WGS", "63", {"apply_wgs": 0, "apply_wgs_given": 1}),     # (given, out of range:
    ("GTAMD_APPLY_WGS", "4194305", {"apply_wgs": 0, "apply_wgs_given": 1}),  # the grid uncapped)
    ("GTAMD_RANK_WINDOW_BITS", "9", {"rank_window_bits": 9}),
    ("GTAMD_RANK_WINDOW_BITS", "2", {"rank_window_bits": 2}),
    ("GTAMD_RANK_WINDOW_BITS", "15", {"rank_window_bits": 15}),
    ("GTAMD_RANK_WINDOW_BITS", "1", {"rank_window_bits": 15}),
    ("GTAMD_RANK_WINDOW_BITS", "16", {"rank_window_bits": 15}),
    ("GTAMD_RANK_ALL_WINDOWS", "1", {"rank_all_windows": 1}),
    ("GTAMD_RANK_ALL_WINDOWS", "0", {"rank_all_windows": 0}),
    ("GTAMD_RANK_ALL_WINDOWS", "2", {"rank_all_windows": 0}),
    ("GTAMD_WIN_FILTER_LDS", "0", {"win_filter_global": 1}),
    ("GTAMD_WIN_FILTER_LDS", "1", {"win_filter_global": 0}),
    ("GTAMD_WIN_FILTER_LDS", "x", {"win_filter_global": 0}),
    ("GTAMD_PAIR_CHUNK", "32", {"pair_chunk": 32}),
    ("GTAMD_PAIR_CHUNK", "4", {"pair_chunk": 4}),
    ("GTAMD_PAIR_CHUNK", "1024", {"pair_chunk": 1024}),
    ("GTAMD_PAIR_CHUNK", "3", {"pair_chunk": 0}),
    ("GTAMD_PAIR_CHUNK", "1025", {"pair_chunk": 0}),
    ("GTAMD_ROUND_STRIDE", "1000", {"round_stride": 1000}),
    ("GTAMD_ROUND_STRIDE", "512", {"round_stride": 512}),
    ("GTAMD_ROUND_STRIDE", "2048", {"round_stride": 2048}),
    ("GTAMD_ROUND_STRIDE", "511", {"round_stride": 1536}),
    ("GTAMD_ROUND_STRIDE", "2049", {"round_stride": 1536}),
]


def test_switches_line_without_switches(gpu, debug, capfd):
    enc = synth.generate(synth.MODEL_UNIFORM_DNA, 3, 3000)
    _, p = _run(capfd, enc)
    assert p["switches"] == dict(_DEF, debug=1)


@pytest.mark.parametrize("var,value,want", PARSE, ids=["%s=%s" % (c[0], c[1]) for c in PARSE])
def test_parse_rules(gpu, debug, capfd, var, value, want):
    debug.setenv(var, value)
    enc = synth.generate(synth.MODEL_HUMANLIKE_DNA, 4, 3000)
    capfd.readouterr()
    esa.suffixerator_tables(enc, 4)
    parts = engine_paths.parse(capfd.readouterr().err)
    assert sorted(parts) == [0]
    assert parts[0]["switches"] == dict(_DEF, debug=1, **want)


# ---------------------------------------------------------------------------
# GTAMD_MSD_BIN_LIMIT: the crowded-bin limit of k_msd_local
# ---------------------------------------------------------------------------
def _bin_inputs():
    rng = np.random.default_rng(41)
    r = rng.integers(0, 4, 30000, dtype=np.uint8)
    yield "one_12mer_over_and_over", np.concatenate(
        [np.concatenate([r[:12], rng.integers(0, 4, 9, dtype=np.uint8)]) for _ in range(3000)])
    blk = rng.integers(0, 4, 3000, dtype=np.uint8)      # (bins of 40 equal suffixes)
    yield "forty_copies", np.concatenate([np.concatenate([blk, rng.integers(0, 4, 500, dtype=np.uint8)])
                                          for _ in range(40)])
    yield "humanlike", synth.generate(synth.MODEL_HUMANLIKE_DNA, 43, 300000)


@pytest.mark.parametrize("name,enc", list(_bin_inputs()), ids=[c[0] for c in _bin_inputs()])
@pytest.mark.parametrize("limit", [2, 16, 4096])
def test_msd_bin_limit(gpu, debug, capfd, limit, name, enc):
    debug.setenv("GTAMD_MSD", "1")
    debug.setenv("GTAMD_MSD_BIN_LIMIT", str(limit))
    res, p = _run(capfd, enc)
    _assert_same_as_oracle(enc, 4, res)
    assert p["switches"]["msd_bin_limit"] == limit
    assert p["msd_local"]["bin_limit"] == limit and p["msd_local"]["force_radix"] == 0
    if limit <= 16:
        assert p["msd_local"]["radix_runs"] > 0
        assert res.stats["msd_crowded_entries"] > 0
    else:                       # (no bin of a run of at most 4096 entries holds more)
        assert p["msd_local"]["radix_runs"] == 0
        assert res.stats["msd_crowded_entries"] == 0


# ---------------------------------------------------------------------------
# GTAMD_MSD_PACK_CAP: the size limit of a packed level-D tile
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("pack", ["1", "0"])
def test_msd_pack_cap(gpu, debug, capfd, pack):
    debug.setenv("GTAMD_MSD", "1")
    debug.setenv("GTAMD_MSD_PACK", pack)
    debug.setenv("GTAMD_MSD_CBITS", "8")
    rng = np.random.default_rng(45)
    # (two letters: 256 parents of some 7800 entries, cut into tiles by the cap)
    enc = rng.integers(0, 2, 2_000_000, dtype=np.uint8) * 3
    enc[rng.integers(0, enc.size, 40)] = 254
    ora = ou.esa(enc, 4)
    tiles = {}
    for cap in (1024, 2048, 3000, 4096):
        debug.setenv("GTAMD_MSD_PACK_CAP", str(cap))
        res, p = _run(capfd, enc)
        _assert_same_as_oracle(enc, 4, res, ora)
        assert p["switches"]["msd_pack_cap"] == cap
        d = p["level_d"]
        assert d["packed"] == int(pack) and d["pack_cap"] == cap and d["tiles"] > 0
        tiles[cap] = d["tiles"]
        if pack == "1":
            # a tile above the cap is one range alone, and no range is above the LDS tile here
            assert p["msd"]["big"] == 0 and p["msd"]["giant"] == 0
            assert d["largest"] <= 4096
    if pack == "1":     # (a smaller cap: more tiles)
        assert tiles[1024] > tiles[2048] > tiles[3000] > tiles[4096]
    else:               # (the stride rule does not look at the cap)
        assert len(set(tiles.values())) == 1


# ---------------------------------------------------------------------------
# GTAMD_PAIR_CHUNK: pairs per thread of k_pair_resolve, with record counts just
# below, at and just above a multiple of chunk x 256 (the last thread's partial
# chunk, the grid edge)
# ---------------------------------------------------------------------------
def _pair_text(copy_len, extra, seed=47):
    """random DNA with one block copied: every suffix in the block and its copy
    is a pair; `extra` more symbols copied in front of the block add as many
    pairs and change nothing behind it (mostly: a chance tie in front can add
    two or three at once)"""
    rng = np.random.default_rng(seed)
    n = 2 * copy_len + 60000
    enc = rng.integers(0, 4, n, dtype=np.uint8)
    src, dst = 20000, copy_len + 40000
    enc[dst - extra:dst + copy_len] = enc[src - extra:src + copy_len]
    return enc


def _pairs_run(capfd, enc):
    res, p = _run(capfd, enc)
    return res, p, p["pair_resolve"]["records"]


def _pairs_exactly(capfd, base, target):
    """the text of _pair_text with exactly `target` pair records (a few more
    symbols in front of the block, until the count is right)"""
    seen = []
    for seed in range(47, 55):
        _, _, r0 = _pairs_run(capfd, _pair_text(base, 0, seed))
        e0 = target - r0
        for d in (0, -1, 1, -2, 2, -3, 3):
            enc = _pair_text(base, e0 + d, seed)
            res, p, nrec = _pairs_run(capfd, enc)
            if nrec == target:
                return enc, res, p
            seen.append(nrec)
    raise AssertionError("no text with %d pair records: %s" % (target, seen))


@pytest.mark.parametrize("chunk,want", [("17", 32), ("32", 32), ("128", 128), ("1024", 1024)])
def test_pair_chunk_at_the_grid_edge(gpu, debug, capfd, chunk, want):
    debug.setenv("GTAMD_PAIR_CHUNK", chunk)
    per_wg = want * 256
    for target in (per_wg - 1, per_wg, per_wg + 1):
        enc, res, p = _pairs_exactly(capfd, per_wg - 200, target)
        nrec = p["pair_resolve"]["records"]
        assert p["switches"]["pair_chunk"] == int(chunk)
        pr = p["pair_resolve"]
        assert pr["chunk"] == want
        assert pr["grid"] == -(-(-(-nrec // want)) // 256)
        assert res.stats["pair_suffixes"] > 0
        _assert_same_as_oracle(enc, 4, res)


# ---------------------------------------------------------------------------
# GTAMD_ROUND_STRIDE: the distance of the round tiles' starts
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("stride", [512, 1000, 2048])
def test_round_stride(gpu, debug, capfd, stride):
    debug.setenv("GTAMD_ROUND_STRIDE", str(stride))
    rng = np.random.default_rng(53)
    unit = rng.integers(0, 4, 23, dtype=np.uint8)
    enc = np.concatenate([rng.integers(0, 4, 9000, dtype=np.uint8), np.tile(unit, 2500),
                          rng.integers(0, 4, 20000, dtype=np.uint8),
                          synth.generate(synth.MODEL_REPEAT_HEAVY, 5, 100000)]).astype(np.uint8)
    res, p = _run(capfd, enc)
    _assert_same_as_oracle(enc, 4, res)
    assert p["switches"]["round_stride"] == stride
    assert p["rounds"] > 0 and p["across"]
    assert all(a["stride"] == stride for a in p["across"])
    assert engine_paths.across_entries(p) > 0


# ---------------------------------------------------------------------------
# the fuzzer's combinations (tests/fuzz_cases.py), replayed with fixed seeds
# ---------------------------------------------------------------------------
REPLAY_CASES = 400
REPLAY_SEED = 20261016


def _seen(paths, p, stats=None):
    sw, run = p["switches"], p["run"]
    if run["first_sort"] == "msd" and run["parts"] == 1:
        paths.add("msd whole table")
        paths.add("level C depth %d" % p["msd"]["cbits"])
        if p["msd"]["giant"]:
            paths.add("giant runs")
        if p["msd"]["big"]:
            paths.add("big runs")
        paths.add("level D packed=%d" % p["level_d"]["packed"])
        if p["msd_local"]["radix_runs"] and p["msd_local"]["force_radix"]:
            paths.add("radix runs, forced")
        if p["msd_local"]["radix_runs"] and not p["msd_local"]["force_radix"]:
            paths.add("radix runs, crowded bins")
    if run["parts"] > 1:
        paths.add("%d parts, %s first sort" % (run["parts"], run["first_sort"]))
        if run["positions"] == 64:
            paths.add("parts with 64-bit positions")
    if p["pair_resolve"] and p["pair_resolve"]["chunk"] != 16:
        paths.add("pair chunk %d" % p["pair_resolve"]["chunk"])
    for a in p["apply"]:
        if a["pair_grid"]:
            paths.add("apply placement %d" % a["placement"])
    for w in p["win_filter"]:
        paths.add("window bitmap in %s" % w["bitmap"])
    if p["rank_whole"]:
        paths.add("whole rank table")
    if any(not w["whole"] for w in p["rank_windows"]):
        paths.add("rank table of selected windows")
    if engine_paths.across_entries(p) and sw["round_stride"] != 1536:
        paths.add("groups across round tiles, stride %d" % sw["round_stride"])


# (runs above the LDS tile need larger ranges than the fuzzer's texts have:
# test_msd_gpu.test_skewed_ranges forces them)
REPLAY_PATHS = (["msd whole table", "level D packed=0", "level D packed=1",
                 "radix runs, forced", "radix runs, crowded bins", "whole rank table",
                 "rank table of selected windows", "window bitmap in lds",
                 "window bitmap in global"] +
                ["level C depth %d" % c for c in range(9)] +
                ["pair chunk %d" % c for c in (32, 128, 1024)] +
                ["apply placement %d" % a for a in range(3)] +
                ["%d parts, msd first sort" % r for r in range(2, 6)] +
                ["%d parts, lsd first sort" % r for r in range(2, 6)] +
                ["parts with 64-bit positions"] +
                ["groups across round tiles, stride %d" % s for s in (512, 2048)])


def test_fuzz_replay(gpu, debug, capfd):
    """whole-table builds through the MSD first sort with the switch draws of the
    fuzzer, and one case in three in 2 to 5 parts, each against the oracle; over
    the whole replay every path the engine reports runs at least once.  The draws
    and the cases of 64-bit positions are the fuzzer's (fuzz_cases.py)."""
    paths = set()
    for case in range(REPLAY_CASES):
        seed = REPLAY_SEED * 1000003 + case
        rng = np.random.default_rng(seed)
        sigma = 20 if rng.integers(0, 4) == 0 else 4
        enc = random_sequence(rng, sigma)
        prefix_length(rng, sigma)       # (the fuzzer's first build: drawn, not built here)
        wide = case % 7 == 3            # (the fuzzer: 64-bit positions, no MSD build)
        ora = ou.esa(enc, sigma)
        if enc.size >= 64 and not wide:
            env = msd_switches(rng)
            with debug.context() as mp:
                for k, v in env.items():
                    mp.setenv(k, v)
                res, p = _run(capfd, enc, sigma)
                try:
                    _assert_same_as_oracle(enc, sigma, res, ora)
                except AssertionError as e:
                    raise AssertionError("seed %d %s: %s" % (seed, env, e)) from e
            assert p["run"]["first_sort"] == "msd", (seed, env)
            _seen(paths, p)
        if case % 3 == 0:
            parts, env = parts_switches(rng)
            if wide:
                env["GTAMD_FORCE_WIDE"] = "1"
            with debug.context() as mp:
                for k, v in env.items():
                    mp.setenv(k, v)
                capfd.readouterr()
                tabs = build_in_parts(enc, sigma, parts)[0]
                per_part = engine_paths.parse(capfd.readouterr().err)
            for name in ("suf", "lcp", "llv", "bwt"):
                assert np.array_equal(tabs[name], ora[name]), "seed %d parts %d %s %s" % (
                    seed, parts, env, name)
            assert sorted(per_part) == list(range(parts)), (seed, sorted(per_part))
            for q in per_part.values():
                _seen(paths, q)
    missing = [x for x in REPLAY_PATHS if x not in paths]
    assert not missing, "never ran: %s (ran: %s)" % (missing, sorted(paths))
