"""The golden calls of tests/golden/golden_assembly.json (made by
tests/golden/make_golden_assembly.py) for the tests of the assembly step: the
reads the list numbers, the list, the options of a call and what the reference
gave.  Also the shapes and the search the mutation checks share."""
import json
import os

import numpy as np

import oracle_util as ou
import prefilter_reference as pr
import strgraph_reference as sg

DIR = os.path.join(ou.GOLDEN_DIR, "assembly")
with open(os.path.join(ou.GOLDEN_DIR, "golden_assembly.json")) as _f:
    GOLDEN = json.load(_f)
CALLS = [(n, w, k) for n in sorted(GOLDEN) for w in ("calls", "shuffled") for k in sorted(GOLDEN[n][w])]
E2E_SETS = sorted(GOLDEN)           # the sets of the end-to-end comparison: none had to be left out
_cache = {}


def reads_of(name):
    if name not in _cache:
        path = os.path.join(DIR, name + ".p.fas")
        _cache[name] = pr.parse_reads(path) if os.path.getsize(path) else []
    return _cache[name]


def list_path(name, which="calls"):
    return os.path.join(DIR, name + (".0.spm" if which == "calls" else ".shuffled.0.spm"))


def records_of(name, which="calls"):
    """the list in its order, as an array of (suffix_read, prefix_read, len, flags)"""
    with open(list_path(name, which), "rb") as f:
        raw = f.read()
    assert raw[0] == 2 and (len(raw) - 1) % 12 == 0
    w = np.frombuffer(raw[1:], dtype="<u4").reshape(-1, 3).astype(np.uint64)
    return np.stack([w[:, 0], w[:, 1], w[:, 2] >> np.uint64(2), w[:, 2] & np.uint64(3)], axis=1)


def options(name, key):
    """(min_len, depthcutoff, lengthcutoff) of a call"""
    if key == "default":
        return 0, sg.DEPTHCUTOFF, sg.LENGTHCUTOFF
    return (GOLDEN[name]["l"] if key == "l" else 0), 1, 1


def cli_options(name, key):
    out = [] if key == "default" else ["-depthcutoff", "1", "-lengthcutoff", "1"]
    return out + (["-l", str(GOLDEN[name]["l"])] if key == "l" else [])


def call(name, which, key):
    return reads_of(name), records_of(name, which), GOLDEN[name][which][key]


def generated():
    """name -> (reads, records, min_len, depthcutoff, lengthcutoff): the shapes
    the device tests run, each at the smallest size that reaches its case"""
    out = {}
    for count in (2, 3, 64, 65, 130):
        out["chain%d" % count] = sg.chain(count) + (0, 1, 1)
    out["circle"] = sg.circle(9) + (0, 1, 1)
    out["two_circles"] = sg.join(sg.circle(7, seed=22), sg.chain(4), sg.circle(5, seed=23)) + (0, 1, 1)
    out["hairpin"] = sg.hairpin() + (0, 1, 1)
    out["junction3"] = sg.junction(3) + (0, 1, 1)
    out["junction3_default_depth"] = sg.junction(3) + (0, 3, 1)
    reads, records = sg.chain(6)
    own = np.array([[2, 2, 5, 3], [4, 4, 6, 2]], dtype=np.uint64)
    out["self_match"] = (reads, np.concatenate([records[:2], own, records[2:]]), 0, 1, 1)
    out["min_len"] = _shorter(9, at=4) + (13, 1, 1)
    reads, records = sg.chain(5, length=20, step=7)                 # depth 5, 48 letters
    for d in (5, 6):
        out["depth_cutoff_%d" % d] = (reads, records, 0, d, 1)
    for c in (48, 49):
        out["length_cutoff_%d" % c] = (reads, records, 0, 1, c)
    for letters, (count, step) in {59: (4, 13), 60: (6, 8), 61: (2, 20), 120: (11, 10)}.items():
        length = letters - step * (count - 1)
        out["letters%d" % letters] = sg.chain(count, length=length, step=step, seed=letters) + (0, 1, 1)
    out["empty_list"] = (sg.chain(3)[0], np.zeros((0, 4), dtype=np.uint64), 0, 1, 1)
    out["lone_reads"] = (sg.chain(3)[0], sg.chain(3)[1][:1], 0, 1, 1)
    return out


def _shorter(count, at):
    """a chain in which the overlap of reads at, at + 1 is 12 letters and the
    others 13: -l 13 removes it and turns two internal vertices into ends"""
    rng = np.random.default_rng(77)
    steps = [7] * (count - 1)
    steps[at] = 8
    starts = np.concatenate([[0], np.cumsum(steps)])
    text = rng.integers(0, 4, int(starts[-1]) + 20, dtype=np.uint8)
    reads = [text[a:a + 20].copy() for a in starts.tolist()]
    records = [sg.match(a, True, a + 1, True, 20 - steps[a]) for a in range(count - 1)]
    return reads, np.array(records, dtype=np.uint64)


def results(broken=()):
    """every golden call (as bytes of X.contigs.fas) and every generated shape
    through the restatement, lazily, by name"""
    for name, which, key in CALLS:
        reads, records, _ = call(name, which, key)
        yield (name, which, key), sg.fasta(sg.contigs(reads, records, *options(name, key), broken=broken))
    for name, (reads, records, min_len, depth, length) in generated().items():
        yield name, sg.fasta(sg.contigs(reads, records, min_len, depth, length, broken=broken))


_intact = {}


def first_miss(rule):
    """the first golden call or generated shape a restatement with `rule` broken
    gets wrong, or None"""
    if not _intact:
        _intact.update(results())
    for name, raw in results(broken=(rule,)):
        if raw != _intact[name]:
            return name
    return None
