"""`gt-suffixerator-amd repfind` on indexes the tool itself built: its sorted
output against the two results the reference records (tests/golden/repfind/),
against every call of tests/golden/golden_repfind.json (md5 and line count of
the reference's sorted output), on an index with 4-byte suffix entries, and the
options and indexes it refuses."""
import hashlib
import json
import os
import subprocess

import pytest

import maxpairs_reference as mp
import oracle_util as ou
from genometools_amd import _lib

pytestmark = pytest.mark.gpu

CLI = os.path.join(_lib.HERE, "gt-suffixerator-amd")
REPFIND_DIR = os.path.join(ou.GOLDEN_DIR, "repfind")
with open(os.path.join(ou.GOLDEN_DIR, "golden_repfind.json")) as _f:
    GOLDEN = json.load(_f)
RECORDED = {"Duplicate.fna.result": ("Duplicate.fna", 8, 29), "Atinsert-8-8": ("Atinsert.fna", 8, 452)}
REFUSED = ["-r", "-p", "-q", "-qii", "-spm", "-samples", "-maxfreq", "-seedlength", "-extendxdrop",
           "-extendgreedy", "-xdropbelow", "-minidentity", "-history", "-outfmt", "-evalue"]


@pytest.fixture(scope="module")
def cli(gpu):
    subprocess.run(["make", "-C", os.path.join(_lib.HERE, "csrc", "host")], check=True,
                   stdout=subprocess.DEVNULL)
    return CLI


@pytest.fixture(scope="module")
def indexes(cli, tmp_path_factory):
    """name|alphabet -> index built by the tool, once"""
    root, built = tmp_path_factory.mktemp("repfind"), {}

    def get(name, alphabet="dna", extra=()):
        key = (name, alphabet) + tuple(extra)
        if key not in built:
            idx = str(root / ("idx%d" % len(built)))
            src = ou.fixture_path(name)
            subprocess.run([cli, "-" + alphabet, "-tis", "-suf", "-lcp", "-ssp", "-indexname", idx, "-db",
                            os.path.basename(src)] + list(extra), check=True, cwd=os.path.dirname(src),
                           stdout=subprocess.DEVNULL)
            built[key] = idx
        return built[key]
    return get


def _run(cli, idx, args=()):
    p = subprocess.run([cli, "repfind"] + list(args) + ["-ii", idx], capture_output=True)
    assert p.returncode == 0 and p.stderr == b"", (args, p.stderr)
    return p.stdout


def _fails(cli, args):
    p = subprocess.run([cli, "repfind"] + list(args), capture_output=True)
    assert p.returncode == 1 and p.stdout == b"", (args, p.stdout[:200])
    lines = p.stderr.decode().splitlines()
    assert len(lines) == 1 and lines[0].startswith("gt repfind: error: "), p.stderr
    return lines[0][len("gt repfind: error: "):]


@pytest.mark.parametrize("result", sorted(RECORDED))
def test_recorded_results(cli, indexes, result):
    name, minlen, count = RECORDED[result]
    with open(os.path.join(REPFIND_DIR, result), "rb") as f:
        want = mp.normalised(f.read())
    out = _run(cli, indexes(name), ["-l", str(minlen)])
    assert len(want) == count and mp.normalised(out) == want
    # the tool's own order is table order: the brute force's records, so ordered
    enc = mp.encoded(name)
    suf = mp.tables("fixture:" + name)[2]["suf"]
    assert out.decode().splitlines() == mp.format_lines(mp.table_order(mp.expected("fixture:" + name, minlen), suf), enc)


SUBJECTS = sorted({tuple(call.split("|")[:2]) for call in GOLDEN})


@pytest.mark.parametrize("subject", SUBJECTS, ids=[s[0] for s in SUBJECTS])
def test_every_golden_call(cli, indexes, subject):
    calls = [call for call in sorted(GOLDEN) if tuple(call.split("|")[:2]) == subject]
    assert len(GOLDEN) == 29 and len(SUBJECTS) == 10 and len(calls) in (2, 3)
    for call in calls:
        name, alphabet, minlen = call.split("|")
        lines = mp.normalised(_run(cli, indexes(name, alphabet), ["-l", minlen]))
        text = "".join(l + "\n" for l in lines).encode("latin-1")
        assert (hashlib.md5(text).hexdigest(), len(lines)) == (GOLDEN[call]["md5"], GOLDEN[call]["lines"]), call


def test_default_length_and_accepted_options(cli, indexes):
    idx = indexes("Atinsert.fna")
    want = _run(cli, idx, ["-l", "20"])
    assert want.count(b"\n") == GOLDEN["Atinsert.fna|dna|20"]["lines"] > 0
    assert _run(cli, idx) == want                                     # default -l 20
    assert _run(cli, idx, ["-f", "-scan"]) == want
    verbose = _run(cli, idx, ["-v"])
    assert verbose.startswith(b"# ") and b"".join(l for l in verbose.splitlines(True) if not l.startswith(b"#")) == want


def test_suftabuint_gives_the_same_output(cli, indexes):
    a, b = indexes("Atinsert.fna"), indexes("Atinsert.fna", extra=["-suftabuint"])
    assert os.path.getsize(a + ".suf") == 2 * os.path.getsize(b + ".suf")
    out = _run(cli, b, ["-l", "8"])
    assert out == _run(cli, a, ["-l", "8"]) and out.count(b"\n") == 452


@pytest.mark.parametrize("option", REFUSED)
def test_refused_options(cli, indexes, option):
    msg = _fails(cli, ["-l", "8", "-ii", indexes("Duplicate.fna"), option])
    assert msg == 'option "%s" is not supported by the MI355X engine' % option


def test_other_refusals(cli, indexes, tmp_path):
    idx = indexes("Duplicate.fna")
    assert _fails(cli, ["-l", "8"]) == 'option "-ii" is mandatory'
    assert _fails(cli, ["-ii", idx, "-l"]) == 'missing argument to option "-l"'
    assert _fails(cli, ["-ii", idx, "-l", "0"]) == 'argument to option "-l" must be an integer >= 1'
    assert _fails(cli, ["-ii", idx, "extra"]) == 'superfluous arguments: "extra"'
    assert _fails(cli, ["-ii", idx, "-nosuch"]).startswith("unknown option: -nosuch")
    # a read mode other than forward, a mirrored index
    src = ou.fixture_path("Duplicate.fna")
    for extra, word in ((["-dir", "rev"], "read mode"), (["-mirrored"], "mirrored")):
        other = str(tmp_path / ("x" + extra[0][1:]))
        subprocess.run([cli, "-dna", "-tis", "-suf", "-lcp", "-ssp", "-indexname", other, "-db",
                        os.path.basename(src)] + extra, check=True, cwd=os.path.dirname(src),
                       stdout=subprocess.DEVNULL)
        assert word in _fails(cli, ["-l", "8", "-ii", other])


def test_missing_tables(cli, tmp_path):
    src = ou.fixture_path("Duplicate.fna")
    for missing in (".lcp", ".suf"):
        idx = str(tmp_path / ("no" + missing[1:]))
        subprocess.run([cli, "-dna", "-tis", "-ssp", "-suf", "-lcp", "-indexname", idx, "-db",
                        os.path.basename(src)], check=True, cwd=os.path.dirname(src), stdout=subprocess.DEVNULL)
        os.remove(idx + missing)
        assert _fails(cli, ["-l", "8", "-ii", idx]) == \
            'cannot open file "%s%s": No such file or directory' % (idx, missing)
