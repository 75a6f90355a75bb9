"""`gt-suffixerator-amd encseq2spm` on indexes the tool itself built from the
golden read sets: its output, sorted as text, against every call of
tests/golden/golden_spm.json (md5 and line count of the reference's sorted
output), its count lines byte for byte, the two outputs stored whole; on an index
built with -suftabuint; without -spm; and with -v."""
import hashlib
import json
import os
import subprocess

import pytest

import oracle_util as ou
from genometools_amd import _lib

pytestmark = pytest.mark.gpu

CLI = os.path.join(_lib.HERE, "gt-suffixerator-amd")
with open(os.path.join(ou.GOLDEN_DIR, "golden_spm.json")) as _f:
    GOLDEN = json.load(_f)


@pytest.fixture(scope="module")
def cli(gpu):
    subprocess.run(["make", "-C", os.path.join(_lib.HERE, "csrc", "host")], check=True,
                   stdout=subprocess.DEVNULL)
    return CLI


@pytest.fixture(scope="module")
def indexes(cli, tmp_path_factory):
    """read file -> index built by the tool, once; the sequence is all encseq2spm needs"""
    root, built = tmp_path_factory.mktemp("encseq2spm"), {}

    def get(name, extra=("-tis", "-ssp")):
        key = (name,) + tuple(extra)
        if key not in built:
            idx = str(root / ("idx%d" % len(built)))
            src = os.path.join(ou.GOLDEN_DIR, name)
            subprocess.run([cli, "-dna", "-indexname", idx, "-db", os.path.basename(src)] + list(extra), check=True,
                           cwd=os.path.dirname(src), stdout=subprocess.DEVNULL)
            built[key] = idx
        return built[key]
    return get


def _run(cli, idx, args):
    p = subprocess.run([cli, "encseq2spm"] + list(args) + ["-ii", idx], capture_output=True)
    assert p.returncode == 0 and p.stderr == b"", (args, p.stderr)
    return p.stdout


def _sorted(out):
    return b"".join(sorted(out.splitlines(True)))


FILES = sorted({k.split("|")[0] for k in GOLDEN["calls"]})


@pytest.mark.parametrize("name", FILES)
def test_every_golden_call(cli, indexes, name):
    calls = [k for k in sorted(GOLDEN["calls"]) if k.split("|")[0] == name]
    assert len(GOLDEN["calls"]) == 11 and len(FILES) == 5 and len(calls) in (1, 4)
    for key in calls:
        min_len, want = key.split("|")[1], GOLDEN["calls"][key]
        text = _sorted(_run(cli, indexes(name), ["-l", min_len, "-spm", "show"]))
        assert (hashlib.md5(text).hexdigest(), text.count(b"\n")) == (want["md5"], want["lines"]), key
        assert _run(cli, indexes(name), ["-l", min_len, "-spm", "count"]) == \
            b"number of suffix-prefix matches=%d\n" % want["count"], key


def test_text_fixtures(cli, indexes):
    assert len(GOLDEN["texts"]) == 2
    for name, key in GOLDEN["texts"].items():
        with open(os.path.join(ou.GOLDEN_DIR, "spm", name), "rb") as f:
            assert _sorted(_run(cli, indexes(key.split("|")[0]), ["-spm", "show", "-l", key.split("|")[1]])) == f.read()


def test_the_tables_of_the_index_do_not_matter(cli, indexes):
    """the tool builds its own tables of the mirrored reads: an index with 4-byte
    suffix entries, one with 8-byte entries and one without tables give the same bytes"""
    name = "spm/mixed.fna"
    plain = _run(cli, indexes(name), ["-l", "20", "-spm", "show"])
    assert plain.count(b"\n") == 1724
    small = indexes(name, ("-tis", "-ssp", "-suf", "-lcp", "-suftabuint"))
    wide = indexes(name, ("-tis", "-ssp", "-suf", "-lcp"))
    assert os.path.getsize(wide + ".suf") == 2 * os.path.getsize(small + ".suf")
    assert _run(cli, small, ["-l", "20", "-spm", "show"]) == plain
    assert _run(cli, wide, ["-l", "20", "-spm", "show"]) == plain
    assert _run(cli, small, ["-l", "20", "-spm", "count"]) == b"number of suffix-prefix matches=1724\n"


def test_without_spm_and_verbose(cli, indexes):
    idx = indexes("spm/equal.fna")
    assert _run(cli, idx, ["-l", "20"]) == b""
    assert _run(cli, idx, ["-l", "20", "-v"]) == b""
    want = _run(cli, idx, ["-l", "20", "-spm", "show"])
    verbose = _run(cli, idx, ["-v", "-spm", "show", "-l", "20"])
    marks = [l for l in verbose.splitlines() if l.startswith(b"#")]
    assert len(marks) == 2 and b" table entries built in " in marks[0] and marks[1].startswith(b"# 1500 matches, ")
    assert b"".join(l for l in verbose.splitlines(True) if not l.startswith(b"#")) == want
    counted = _run(cli, idx, ["-v", "-spm", "count", "-l", "20"]).splitlines()
    assert len(counted) == 3 and counted[2] == b"number of suffix-prefix matches=1500"


def test_a_mirrored_project_is_refused(cli, indexes, tmp_path):
    src = os.path.join(ou.GOLDEN_DIR, "spm", "equal.fna")
    for extra, k in ((["-mirrored"], 0), (["-dir", "rcl"], 1)):
        idx = str(tmp_path / ("x%d" % k))
        subprocess.run([cli, "-dna", "-tis", "-ssp", "-suf", "-indexname", idx, "-db", os.path.basename(src)] + extra,
                       check=True, cwd=os.path.dirname(src), stdout=subprocess.DEVNULL)
        p = subprocess.run([cli, "encseq2spm", "-l", "20", "-spm", "count", "-ii", idx], capture_output=True, text=True)
        assert p.returncode == 1 and p.stdout == "" and p.stderr.startswith("gt encseq2spm: error: ") and \
            "mirrors the reads itself" in p.stderr
