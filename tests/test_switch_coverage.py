"""CPU checks of the engine's switches: every variable read_switches() reads
(genometools_amd/csrc/esa_engine.hip) is set by some test under tests/ -- a
switch that only a tool sets is a path the suite never forces -- and the parser
of the GTAMD_DEBUG lines (engine_paths.py) reads every line the engine writes."""
import os
import re

import pytest

import engine_paths

TESTS = os.path.dirname(os.path.abspath(__file__))
ENGINE = os.path.join(os.path.dirname(TESTS), "genometools_amd", "csrc", "esa_engine.hip")
NOT_A_PATH = {"GTAMD_DEBUG"}       # (it only reports)


def _read_switches_body():
    src = open(ENGINE).read()
    start = src.index("static Switches read_switches() {")
    end = src.index("\n}\n", start)
    return src[start:end]


def _switch_names():
    return sorted(set(re.findall(r'"(GTAMD_[A-Z0-9_]+)"', _read_switches_body())))


def _set_somewhere(name):
    """test modules (tests/test_*.py) that set `name`: monkeypatch.setenv,
    os.environ[...] = or a key of a dict of switches.  Helper modules do not
    count: fuzz_cases.py names most switches for the fuzzer, and a switch that
    only its draws set is fuzz-only again."""
    pat = re.compile(r'(setenv\(\s*["\']%s["\']|environ\[\s*["\']%s["\']\s*\]\s*=|["\']%s["\']\s*:)'
                     % ((re.escape(name),) * 3))
    hits = []
    for dirpath, _, files in os.walk(TESTS):
        for f in files:
            if f.startswith("test_") and f.endswith(".py") and f != os.path.basename(__file__):
                path = os.path.join(dirpath, f)
                if pat.search(open(path, encoding="utf-8", errors="replace").read()):
                    hits.append(os.path.relpath(path, TESTS))
    return hits


def test_read_switches_reads_the_switches():
    names = _switch_names()
    assert "GTAMD_MSD" in names and "GTAMD_DEBUG" in names and len(names) >= 19, names
    assert "getenv(" in _read_switches_body()


@pytest.mark.parametrize("name", [n for n in _switch_names() if n not in NOT_A_PATH])
def test_every_switch_is_set_by_a_test(name):
    assert _set_somewhere(name), "%s is read by read_switches() but no tests/test_*.py sets it" % name


def test_every_switch_is_in_the_comment_above_the_struct():
    src = open(ENGINE).read()
    comment = src[src.index("// Switches of a build run"):src.index("struct Switches {")]
    for name in _switch_names():
        assert re.search(r"//\s+%s\s" % name, comment), name


def test_every_debug_line_has_a_parser():
    """the format strings of the engine's GTAMD_DEBUG lines, filled with numbers,
    are all recognised (none lands in "other")"""
    src = open(ENGINE).read()
    fmts = re.findall(r'fprintf\(stderr,\s*((?:"(?:[^"\\]|\\.)*"\s*)+)', src)
    assert len(fmts) >= 14
    for f in fmts:
        text = "".join(re.findall(r'"((?:[^"\\]|\\.)*)"', f)).replace("\\n", "")
        assert text.startswith("gtamd: "), text
        sample = re.sub(r"%(ll)?[ud]", "3", text.replace("%smsd", "msd")).replace("%s", "")
        p = next(iter(engine_paths.parse(sample).values()))
        assert not p["other"], (text, sample, p["other"])


SAMPLE = """\
gtamd: part 0: switches: msd=1 msd_part_off=0 msd_cbits=8 msd_big_max=4096 msd_radix=1 msd_pack=1 \
msd_pack_cap=4096 msd_bin_limit=128 fused_pass0=1 force_wide=0 no_pairs=0 no_small_groups=0 \
apply_early=2 apply_wgs=0 apply_wgs_given=0 rank_window_bits=15 rank_all_windows=0 \
win_filter_global=1 pair_chunk=17 round_stride=512 debug=1
gtamd: part 0: run: parts=1 positions=32 first_sort=msd pass0=none
gtamd: msd sort: 8 bits at level C, 120 runs, 0 big (largest 0, 0 entries in all), 2 giant
gtamd: msd level D: packed=1 pack_cap=4096 tiles=120 largest=3999
gtamd: msd local: radix_runs=118 force_radix=1 bin_limit=128
gtamd: part 0: pair resolve: records=8193 chunk=32 grid=2
gtamd: part 0: 7 tied with a neighbour, 5 pairs, 1 small groups (3 entries settled), 900 left
gtamd: rank table: 3 of 10 windows of 2^12 positions
gtamd: part 0: win filter: bitmap=global windows=3
gtamd: part 0: apply: placement=2 pair_grid=17 small_grid=1
gtamd: part 0 round 1 h=32 tied=900
gtamd: part 0 round 1: 44 entries in groups across tile borders (2 tiles, stride 512)
gtamd: part 0 round 2 h=64 tied=100
gtamd: part 0 round 2: 6 entries in groups across tile borders (1 tiles, stride 512)
"""


def test_parser_on_a_whole_table_build():
    p = engine_paths.single(SAMPLE)
    assert p["switches"]["msd_big_max"] == 4096 and p["switches"]["pair_chunk"] == 17
    assert p["run"] == {"parts": 1, "positions": 32, "first_sort": "msd", "pass0": "none"}
    assert p["msd"] == {"cbits": 8, "runs": 120, "big": 0, "largest_big": 0, "big_entries": 0, "giant": 2}
    assert p["level_d"]["largest"] == 3999 and p["msd_local"]["radix_runs"] == 118
    assert p["pair_resolve"] == {"records": 8193, "chunk": 32, "grid": 2}
    assert p["ties"]["pairs"] == 5 and p["ties"]["left"] == 900
    assert p["rank_windows"] == [{"selected": 3, "windows": 10, "bits": 12, "whole": False}]
    assert p["win_filter"] == [{"bitmap": "global", "windows": 3}]
    assert p["apply"] == [{"placement": 2, "pair_grid": 17, "small_grid": 1}]
    assert p["rounds"] == 2 and engine_paths.across_entries(p) == 50
    assert p["other"] == []


def test_parser_keeps_parts_apart():
    err = ("gtamd: part 1: switches: pair_chunk=0\n"
           "gtamd: part 0: switches: pair_chunk=0\n"
           "gtamd: part 1/2: tile 5 positions, slice 6 entries at 7\n"
           "gtamd: part 1: msd sort: 2 bits at level C, 3 runs, 1 big (largest 5000, 5000 entries in all), 0 giant\n"
           "gtamd: part 1: rank exchange: all windows\n"
           "gtamd: part 0: ranks of 2 more windows of 2^16 positions travel (2 of 9 so far)\n"
           "gtamd: part 0: rank table: whole table of 77 entries\n")
    parts = engine_paths.parse(err)
    assert sorted(parts) == [0, 1]
    assert parts[1]["msd"]["big"] == 1 and parts[0]["msd"] is None
    assert parts[1]["rank_exchange_all"] and not parts[0]["rank_exchange_all"]
    assert parts[0]["ranks_travel"] == [{"fresh": 2, "bits": 16, "built": 2, "windows": 9}]
    assert parts[0]["rank_whole"] == [77]
    with pytest.raises(AssertionError):
        engine_paths.single(err)
    with pytest.raises(ValueError):
        engine_paths.parse(err + "gtamd: part 0: switches: pair_chunk=0\n")
