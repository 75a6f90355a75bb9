"""`gt-suffixerator-amd tagerator` on the device against what `gt tagerator`
printed: every call of tests/golden/golden_tagmatch.json, from index files
written by this project's own tool into a temporary directory.  As recorded, the
`# indexname` and `# queryfile` lines (they hold paths) are set aside and the
match lines of every tag's block sorted: their order there is the reference's
stack order, here the table's.  The lines set aside are checked by themselves."""
import hashlib
import os
import subprocess

import pytest

import oracle_util as ou
import tagmatch_reference as tr
from genometools_amd import _lib
from test_tagmatch_host import GOLDEN, TAGDIR, parse_call

pytestmark = pytest.mark.gpu

CLI = os.path.join(_lib.HERE, "gt-suffixerator-amd")
SUBJECTS = sorted({k.split("|")[0] for k in GOLDEN["calls"]})


@pytest.fixture(scope="module")
def indexes(gpu, tmp_path_factory):
    """INDEX.prj, .esq, .ssp and .suf of every subject, 4-byte entries for one"""
    subprocess.run(["make", "-C", os.path.join(_lib.HERE, "csrc", "host")], check=True, stdout=subprocess.DEVNULL)
    root = tmp_path_factory.mktemp("tagerator")
    out = {}
    for name in SUBJECTS:
        out[name] = str(root / name)
        subprocess.run([CLI, "-protein" if name.endswith(".fsa") else "-dna", "-tis", "-suf", "-ssp", "-db",
                        ou.fixture_path(name), "-indexname", out[name]] +
                       (["-suftabuint"] if name == "Duplicate.fna" else []), check=True)
    return out


def _run(index, key):
    args, tagfiles = key.split("|")[2].split(), parse_call(key)[5]
    paths = [os.path.join(TAGDIR, t + ".tags.fna") for t in tagfiles]
    p = subprocess.run([CLI, "tagerator"] + args + ["-esa", index, "-q"] + paths, capture_output=True)
    lines = p.stdout.decode("latin-1").splitlines()
    aside = [l for l in lines if l.startswith("# indexname") or l.startswith("# queryfile")]
    assert aside == ["# indexname(esa)=%s" % index] + ["# queryfile=%s" % q for q in paths] == lines[1:1 + len(aside)]
    kept = tr.block_sorted([l for l in lines if l not in aside])
    return p, "".join(l + "\n" for l in kept).encode("latin-1")


@pytest.mark.parametrize("subject", SUBJECTS)
def test_every_recorded_call(indexes, subject):
    calls = [k for k in sorted(GOLDEN["calls"]) if k.split("|")[0] == subject]
    assert calls
    for key in calls:
        want = GOLDEN["calls"][key]
        p, text = _run(indexes[subject], key)
        assert (hashlib.md5(text).hexdigest(), text.count(b"\n")) == (want["md5"], want["lines"]), key
        # the error after the blocks of the tags in front of the failing one
        assert p.returncode == want["exit"], (key, p.stderr)
        assert p.stderr.decode() == ("gt tagerator: error: %s\n" % want["error"] if want["exit"] else ""), key


def test_whole_outputs_line_for_line(indexes):
    for name, key in GOLDEN["texts"].items():
        with open(os.path.join(TAGDIR, name), "rb") as f:
            want = f.read()
        assert _run(indexes[key.split("|")[0]], key)[1].splitlines() == want.splitlines() and want.count(b"\n") > 30


def test_two_tag_files_are_numbered_through(indexes):
    key = "Duplicate.fna|dna|-e 0|trna_glutamine.fna,Duplicate.fna"
    _, text = _run(indexes["Duplicate.fna"], key)
    numbers = [int(l.split(b"\t")[1]) for l in text.splitlines() if l.startswith(b"#\t")]
    first = len(tr.read_tags([os.path.join(TAGDIR, "trna_glutamine.fna.tags.fna")]))
    assert numbers == list(range(len(numbers))) and len(numbers) > first > 0


def test_replaced_wildcards_and_verbose(indexes, tmp_path):
    """-rw: the wildcard of a tag becomes the first letter, as the tag line shows"""
    tags = str(tmp_path / "rw.fna")
    enc, suf = tr.fixture("Duplicate.fna")
    text = "".join(tr.DNA[c] for c in enc[100:120])
    with open(tags, "w") as f:
        f.write(">\n%sn%s\n" % (text[:10], text[11:]))
    p = subprocess.run([CLI, "tagerator", "-e", "1", "-esa", indexes["Duplicate.fna"], "-q", tags],
                       capture_output=True, text=True)
    assert (p.returncode, p.stderr) == (1, "gt tagerator: error: wildcard in tag number 0\n")
    p = subprocess.run([CLI, "tagerator", "-e", "1", "-rw", "-v", "-esa", indexes["Duplicate.fna"], "-q", tags],
                       capture_output=True, text=True)
    assert p.returncode == 0 and p.stderr == ""
    lines = p.stdout.splitlines()
    shown = text[:10] + "a" + text[11:]
    assert lines[4] == "#\t0\t" + shown
    want = tr.tool_lines(enc, suf, tr.DNA, [shown], 1, tr.FORWARD | tr.REVCOMP)
    assert tr.block_sorted(lines[4:-1]) == tr.block_sorted(want) and len(want) > 1
    assert lines[-1].startswith("# 2 jobs, %d matches" % (len(want) - 1))


def test_the_error_after_partial_output(indexes, tmp_path):
    tags = str(tmp_path / "partial.fna")
    enc, suf = tr.fixture("Duplicate.fna")
    good = "".join(tr.DNA[c] for c in enc[300:314])
    with open(tags, "w") as f:
        f.write(">\n%s\n>\n%s\n>\nac.gt\n>\n%s\n" % (good, good[:13], good))
    p = subprocess.run([CLI, "tagerator", "-e", "1", "-nop", "-esa", indexes["Duplicate.fna"], "-q", tags],
                       capture_output=True, text=True)
    assert (p.returncode, p.stderr) == (1, "gt tagerator: error: undefined character '.' in tag number 2\n")
    want = tr.tool_lines(enc, suf, tr.DNA, [good, good[:13]], 1, tr.FORWARD)
    assert tr.block_sorted(p.stdout.splitlines()[4:]) == tr.block_sorted(want) and len(want) > 3
