"""`gt-suffixerator-amd matstat` and `uniquesub` on indexes the tool itself
built: the stdout of every call recorded from the reference in
tests/golden/golden_mstat.json (md5 and line count; three outputs byte for
byte), and what the reference's suite does not call: -suftabuint, -dir rev,
several query files, descriptions that are empty."""
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import mstat_reference as mr
import oracle_util as ou
from genometools_amd import _lib

pytestmark = pytest.mark.gpu

CLI = os.path.join(_lib.HERE, "gt-suffixerator-amd")
CHARACTERS = {"dna": "acgt", "protein": "LVIFKREDAGSTNQYWPHMC"}

with open(os.path.join(ou.GOLDEN_DIR, "golden_mstat.json")) as _f:
    GOLDEN = json.load(_f)


@pytest.fixture(scope="module")
def cli(gpu):
    subprocess.run(["make", "-C", os.path.join(_lib.HERE, "csrc", "host")], check=True,
                   stdout=subprocess.DEVNULL)
    return CLI


def _build(cli, name, idx, flag="-dna", extra=()):
    src = ou.fixture_path(name)
    subprocess.run([cli, flag, "-tis", "-suf", "-ssp", "-indexname", idx, "-db", os.path.basename(src)] +
                   list(extra), check=True, cwd=os.path.dirname(src), stdout=subprocess.DEVNULL)


def _run(cli, tool, idx, queries, args):
    p = subprocess.run([cli, tool] + list(args) + ["-esa", idx, "-query"] + list(queries),
                       capture_output=True)
    assert p.returncode == 0 and p.stderr == b"", (tool, args, p.stderr)
    return p.stdout


def _tool_of(call):
    return call.split("_")[0]


def _per_query_file(out, queries):
    """the stdout of one call over several query files, cut into what a call for
    each file alone prints: its units, numbered from 0 (one process per index and
    call instead of one per pair)"""
    counts = [len(mr.read_descriptions(q)) for q in queries]
    firsts = np.concatenate([[0], np.cumsum(counts)])
    parts = [[] for _ in queries]
    k = -1
    for line in out.splitlines(keepends=True):
        if line.startswith(b"unit "):
            unit = int(line.split()[1])
            k = int(np.searchsorted(firsts, unit, side="right")) - 1
            line = b"unit %d" % (unit - firsts[k]) + line[len(b"unit %d" % unit):]
        parts[k].append(line)
    assert k == len(queries) - 1
    return [b"".join(p) for p in parts]


SUBJECTS = sorted({pair.split("|")[0] for pair in GOLDEN["dna"]})


@pytest.mark.parametrize("subject", SUBJECTS)
def test_every_recorded_call(cli, subject, tmp_path):
    idx = str(tmp_path / "sfx")
    _build(cli, subject, idx)
    pairs = [p for p in sorted(GOLDEN["dna"]) if p.split("|")[0] == subject]
    assert len(pairs) == 8
    queries = [ou.fixture_path(p.split("|")[1]) for p in pairs]
    for call in sorted(GOLDEN["calls"]):
        outs = _per_query_file(_run(cli, _tool_of(call), idx, queries, GOLDEN["calls"][call]), queries)
        for pair, out in zip(pairs, outs):
            want = GOLDEN["dna"][pair][call]
            assert (hashlib.md5(out).hexdigest(), out.count(b"\n")) == (want["md5"], want["lines"]), (pair, call)


def test_the_protein_pair(cli, tmp_path):
    (pair, entry), = GOLDEN["protein"].items()
    subject, query = pair.split("|")
    idx = str(tmp_path / "sfx")
    _build(cli, subject, idx, "-protein")
    for call, want in sorted(entry.items()):
        out = _run(cli, _tool_of(call), idx, [ou.fixture_path(query)], GOLDEN["calls"][call])
        assert (hashlib.md5(out).hexdigest(), out.count(b"\n")) == (want["md5"], want["lines"]), call


@pytest.mark.parametrize("name", sorted(GOLDEN["texts"]))
def test_whole_outputs(cli, name, tmp_path):
    t = GOLDEN["texts"][name]
    idx = str(tmp_path / "sfx")
    _build(cli, t["subject"], idx, "-" + t["alphabet"])
    out = _run(cli, _tool_of(t["call"]), idx, [ou.fixture_path(t["query"])], GOLDEN["calls"][t["call"]])
    assert out == open(os.path.join(ou.GOLDEN_DIR, "mstat", name), "rb").read()
    # -verify changes nothing with -esa
    if t["call"].startswith("matstat"):
        assert _run(cli, "matstat", idx, [ou.fixture_path(t["query"])],
                    GOLDEN["calls"][t["call"]] + ["-verify"]) == out


FULL = {"matstat": (["-output", "querypos", "subjectpos", "sequence", "-min", "1"],
                    {"querypos", "subjectpos", "sequence"}),
        "uniquesub": (["-output", "querypos", "sequence", "-min", "1"], {"querypos", "sequence"})}


def _expected_text(tool, enc, queries, show, minlen=1, maxlen=None):
    """the brute force over the query files, units numbered across them"""
    suf = ou.esa(enc, 4)["suf"]
    out, unit = "", 0
    for q in queries:
        query = ou.encode_fasta(q)
        ms, w, mu = mr.brute_force(enc, suf, query)
        desc = mr.read_descriptions(q)
        out += mr.tool_output(query, desc, ms if tool == "matstat" else mu, w, CHARACTERS["dna"], show,
                              minlen=minlen, maxlen=maxlen, first_unit=unit)
        unit += len(desc)
    return out.encode("latin-1")


def test_suftabuint_gives_the_same_output(cli, tmp_path):
    a, b = str(tmp_path / "wide"), str(tmp_path / "narrow")
    _build(cli, "Atinsert.fna", a)
    _build(cli, "Atinsert.fna", b, extra=["-suftabuint"])
    assert os.path.getsize(a + ".suf") == 2 * os.path.getsize(b + ".suf")
    query = [ou.fixture_path("Duplicate.fna")]
    for tool, (args, _) in FULL.items():
        out = _run(cli, tool, b, query, args)
        assert out == _run(cli, tool, a, query, args) and out.count(b"\n") > 100


def test_reversed_index_against_the_brute_force(cli, tmp_path):
    idx = str(tmp_path / "rev")
    _build(cli, "Atinsert.fna", idx, extra=["-dir", "rev"])
    enc = ou.apply_readmode(ou.encode_fasta(ou.fixture_path("Atinsert.fna")), "rev")
    query = [ou.fixture_path("Duplicate.fna")]
    for tool, (args, show) in FULL.items():
        assert _run(cli, tool, idx, query, args) == _expected_text(tool, enc, query, show)


def test_two_query_files_and_empty_descriptions(cli, tmp_path):
    """units count across the files; `unit U` alone for an empty description"""
    idx = str(tmp_path / "sfx")
    _build(cli, "Atinsert.fna", idx)
    enc = ou.encode_fasta(ou.fixture_path("Atinsert.fna"))
    own = str(tmp_path / "own.fna")
    # the longest stretch of the subject without a special (it has many wildcards)
    cuts = np.flatnonzero(np.concatenate([[True], enc >= 254, [True]]))
    k = int(np.argmax(np.diff(cuts)))
    stretch = enc[cuts[k]:cuts[k + 1] - 1]
    assert stretch.size >= 30 and (stretch < 254).all()
    seq = "".join("acgt"[c] for c in stretch)
    half = len(seq) // 2
    with open(own, "w") as f:
        f.write(">\n%s\n>second one\n%sn%s\n>\nacgtacgtac\n" % (seq[:half], seq[half:], seq[:7]))
    queries = [ou.fixture_path("Random159.fna"), own, ou.fixture_path("trna_glutamine.fna")]
    for tool, (args, show) in FULL.items():
        out = _run(cli, tool, idx, queries, args)
        assert out == _expected_text(tool, enc, queries, show)
        units = [l for l in out.split(b"\n") if l.startswith(b"unit ")]
        first = len(mr.read_descriptions(queries[0]))
        assert units[first:first + 3] == [b"unit %d" % first, b"unit %d (second one)" % (first + 1),
                                          b"unit %d" % (first + 2)]
        assert len(units) == first + 3 + len(mr.read_descriptions(queries[2]))
    # -min and -max together, lengths in [5, 8] only
    args = ["-output", "querypos", "-min", "5", "-max", "8"]
    out = _run(cli, "matstat", idx, queries, args)
    assert out == _expected_text("matstat", enc, queries, {"querypos"}, minlen=5, maxlen=8)
    lengths = [int(l.split()[1]) for l in out.decode().splitlines() if not l.startswith("unit")]
    assert lengths and min(lengths) >= 5 and max(lengths) <= 8
