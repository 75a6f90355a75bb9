"""What a build chose, read back from the engine's GTAMD_DEBUG lines on stderr
(genometools_amd/csrc/esa_engine.hip).  Forced-path tests capture stderr with
`capfd` and assert that the path they force really ran: a switch value out of
range falls back to the default without a word, and the tables still match.

    paths = engine_paths.parse(capfd.readouterr().err)
    p = paths[0]                  # part 0: a whole-table build
    p["switches"]["msd_big_max"], p["msd"]["giant"], p["win_filter"][0]["bitmap"]

One dict per part.  Lines without a part number come from part 0 (a whole-table
build).  A capture must hold one build: a second `switches` line for a part is an
error.  Helper module, not a conftest."""
import re

_KV = re.compile(r"(\w+)=(\S+)")

_MSD = re.compile(r"(\d+) bits at level C, (\d+) runs, (\d+) big \(largest (\d+), (\d+) entries in all\), "
                  r"(\d+) giant$")
_RANK_SEL = re.compile(r"(\d+) of (\d+) windows of 2\^(\d+) positions( -> whole table)?$")
_RANK_WHOLE = re.compile(r"whole table of (\d+) entries$")
_TRAVEL = re.compile(r"ranks of (\d+) more windows of 2\^(\d+) positions travel \((\d+) of (\d+) so far\)$")
_TIES = re.compile(r"(\d+) tied with a neighbour, (\d+) pairs, (\d+) small groups \((\d+) entries settled\), "
                   r"(\d+) left$")
_ROUND = re.compile(r"round (\d+) h=(\d+) tied=(\d+)$")
_ACROSS = re.compile(r"round (\d+): (\d+) entries in groups across tile borders \((\d+) tiles, stride (\d+)\)$")
_LINE = re.compile(r"gtamd: (?:part (\d+)(?:/\d+)?(?::\s*|\s+(?=round)))?(.*)$")


def _value(v):
    try:
        return int(v)
    except ValueError:
        return v


def _kv(text):
    return {k: _value(v) for k, v in _KV.findall(text)}


def _part():
    return {"switches": None, "run": None, "msd": None, "level_d": None, "msd_local": None,
            "pair_resolve": None, "apply": [], "win_filter": [], "rank_windows": [],
            "rank_whole": [], "rank_exchange_all": False, "ranks_travel": [], "ties": None,
            "rounds": 0, "across": [], "tile": None, "direct": [], "other": []}


def parse(err):
    """{part: dict} from captured stderr"""
    parts = {}
    for raw in err.splitlines():
        m = _LINE.match(raw.strip())
        if m is None:
            continue
        part = int(m.group(1)) if m.group(1) is not None else 0
        body = m.group(2)
        p = parts.setdefault(part, _part())
        topic, _, rest = body.partition(": ")
        if topic == "switches":
            if p["switches"] is not None:
                raise ValueError("two builds of part %d in one capture" % part)
            p["switches"] = _kv(rest)
        elif topic.startswith("tile "):
            p["tile"] = body
        elif topic == "run":
            p["run"] = _kv(rest)
        elif topic == "msd sort" and _MSD.match(rest):
            g = [int(x) for x in _MSD.match(rest).groups()]
            p["msd"] = dict(zip(("cbits", "runs", "big", "largest_big", "big_entries", "giant"), g))
        elif topic == "msd level D":
            p["level_d"] = _kv(rest)
        elif topic == "msd local":
            p["msd_local"] = _kv(rest)
        elif topic == "pair resolve":
            p["pair_resolve"] = _kv(rest)
        elif topic == "apply":
            p["apply"].append(_kv(rest))
        elif topic == "direct ties":          # call=first|left tied=M0 gaveup=0|1, one per call
            p["direct"].append(_kv(rest))
        elif topic == "win filter":
            p["win_filter"].append(_kv(rest))
        elif topic == "rank table" and _RANK_SEL.match(rest):
            sel, total, bits, whole = _RANK_SEL.match(rest).groups()
            p["rank_windows"].append({"selected": int(sel), "windows": int(total), "bits": int(bits),
                                      "whole": whole is not None})
        elif topic == "rank table" and _RANK_WHOLE.match(rest):
            p["rank_whole"].append(int(_RANK_WHOLE.match(rest).group(1)))
        elif topic == "rank exchange" and rest == "all windows":
            p["rank_exchange_all"] = True
        elif _TRAVEL.match(body):
            fresh, bits, sofar, total = (int(x) for x in _TRAVEL.match(body).groups())
            p["ranks_travel"].append({"fresh": fresh, "bits": bits, "built": sofar, "windows": total})
        elif _TIES.match(body):
            g = [int(x) for x in _TIES.match(body).groups()]
            p["ties"] = dict(zip(("tied", "pairs", "small_groups", "settled", "left"), g))
        elif _ACROSS.match(body):
            rnd, entries, tiles, stride = (int(x) for x in _ACROSS.match(body).groups())
            p["across"].append({"round": rnd, "entries": entries, "tiles": tiles, "stride": stride})
        elif _ROUND.match(body):
            p["rounds"] = max(p["rounds"], int(_ROUND.match(body).group(1)))
        else:
            p["other"].append(body)
    return parts


def single(err):
    """the one part of a whole-table build (part 0), which must have reported its switches"""
    parts = parse(err)
    assert list(parts) == [0], "expected one whole-table build, got parts %s" % sorted(parts)
    p = parts[0]
    assert p["switches"] is not None, "no switches line: GTAMD_DEBUG not set?\n" + err
    return p


def across_entries(p):
    """entries in groups across round-tile borders, summed over the rounds"""
    return sum(a["entries"] for a in p["across"])
