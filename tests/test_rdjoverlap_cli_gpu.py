"""`gt-suffixerator-amd readjoiner overlap` on readsets the tool itself encoded
from the golden read sets: its stdout against every call of
tests/golden/golden_rdjoverlap.json byte for byte, the match lines sorted (md5
and line count of the reference's sorted lines, its `#` lines verbatim and in
their places); -q; -elimtrans no; X.0.spm parsed and compared as a set of records
with the reference's; -v; and a readset with contained reads, which is refused."""
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import oracle_util as ou
import spmred_reference as rr
from genometools_amd import _lib

pytestmark = pytest.mark.gpu

CLI = os.path.join(_lib.HERE, "gt-suffixerator-amd")
with open(os.path.join(ou.GOLDEN_DIR, "golden_rdjoverlap.json")) as _f:
    GOLDEN = json.load(_f)
FILES = sorted({k.split("|")[0] for k in GOLDEN["calls"]})


@pytest.fixture(scope="module")
def cli(gpu):
    subprocess.run(["make", "-C", os.path.join(_lib.HERE, "csrc", "host")], check=True,
                   stdout=subprocess.DEVNULL)
    return CLI


@pytest.fixture(scope="module")
def readsets(cli, tmp_path_factory):
    """read file -> readset encoded by the tool, once: X.esq and X.ssp are all the tool reads"""
    root, built = tmp_path_factory.mktemp("rdjoverlap"), {}

    def get(path):
        if path not in built:
            idx = str(root / ("reads%d" % len(built)))
            subprocess.run([cli, "-dna", "-indexname", idx, "-db", os.path.basename(path), "-tis", "-ssp"], check=True,
                           cwd=os.path.dirname(path), stdout=subprocess.DEVNULL)
            built[path] = idx
        return built[path]
    return get


def _run(cli, idx, args):
    p = subprocess.run([cli, "readjoiner", "overlap", "-readset", idx] + list(args), capture_output=True)
    assert p.returncode == 0 and p.stderr == b"", (args, p.stderr)
    return p.stdout.decode().splitlines()


def _golden_path(name):
    return os.path.join(ou.GOLDEN_DIR, "rdj", name)


def _text(lines):
    return "".join(l + "\n" for l in lines).encode()


@pytest.mark.parametrize("name", FILES)
def test_every_golden_call(cli, readsets, name):
    calls = [k for k in sorted(GOLDEN["calls"]) if k.split("|")[0] == name]
    assert len(GOLDEN["calls"]) == 12 and len(FILES) == 3 and len(calls) == 4
    idx = readsets(_golden_path(name))
    for key in calls:
        _, min_len, elim = key.split("|")
        want = GOLDEN["calls"][key]
        args = ["-l", min_len] + ([] if elim == "yes" else ["-elimtrans", "no"])
        lines = _run(cli, idx, args + ["-showspm"])
        closing = 3 if elim == "yes" else 2
        # the two opening lines, the matches, the closing lines: the reference's, in their places
        assert lines[:2] + lines[-closing:] == want["hash_lines"], key
        matches = lines[2:-closing]
        assert not any(l.startswith("#") for l in matches)
        text = _text(sorted(matches))
        assert (hashlib.md5(text).hexdigest(), len(matches)) == (want["md5"], want["lines"]), key
        # -q: the matches alone, the same bytes
        assert _run(cli, idx, args + ["-showspm", "-q"]) == matches
        # without -showspm: the `#` lines alone, and the list file
        if os.path.exists(idx + ".0.spm"):
            os.remove(idx + ".0.spm")
        assert _run(cli, idx, args) == want["hash_lines"], key
        records = rr.parse_bin32(open(idx + ".0.spm", "rb").read())
        assert len(records) == len(set(records)) == want["lines"]
        assert hashlib.md5(rr.sorted_text(np.array(records).reshape(-1, 4))).hexdigest() == want["spm_md5"], key
        assert _text(sorted(rr.lines(np.array(records).reshape(-1, 4)))) == text


def test_text_fixtures(cli, readsets):
    assert len(GOLDEN["texts"]) == 2
    for name, key in GOLDEN["texts"].items():
        path, min_len, _ = key.split("|")
        with open(_golden_path(name), "rb") as f:
            assert _text(sorted(_run(cli, readsets(_golden_path(path)), ["-l", min_len, "-showspm", "-q"]))) == f.read()


def test_quiet_writes_the_list_and_nothing_else(cli, readsets):
    idx = readsets(_golden_path("equal.fna"))
    assert _run(cli, idx, ["-l", "20", "-q"]) == []
    assert len(rr.parse_bin32(open(idx + ".0.spm", "rb").read())) == 190
    before = os.path.getmtime(idx + ".0.spm"), open(idx + ".0.spm", "rb").read()
    assert len(_run(cli, idx, ["-l", "12", "-elimtrans", "no", "-showspm", "-q"])) == 933
    assert open(idx + ".0.spm", "rb").read() == before[1]          # -showspm writes no list


def test_verbose_adds_lines_of_its_own(cli, readsets):
    idx = readsets(_golden_path("mixed.fna"))
    plain = _run(cli, idx, ["-l", "20", "-showspm"])
    verbose = _run(cli, idx, ["-l", "20", "-showspm", "-v"])
    assert [l for l in verbose if not l.startswith("#")] == [l for l in plain if not l.startswith("#")]
    marks = [l for l in verbose if l.startswith("#")]
    assert marks[:3] == ["# gt readjoiner overlap (version 1.2)", "# verbose output activated",
                         "# number of reads in filtered readset = 93"]
    assert len(marks) == 9 and " table entries built in " in marks[3]
    assert " suffix-prefix matches decided, 94 kept, " in marks[4] and " candidates examined, " in marks[5]
    assert marks[-3:] == [l for l in plain if l.startswith("#")][-3:]


def test_a_readset_with_contained_reads_is_refused(cli, readsets, tmp_path):
    """tests/golden/spm/mixed.fna: duplicates, contained reads, a palindrome -- counted and named"""
    idx = readsets(os.path.join(ou.GOLDEN_DIR, "spm", "mixed.fna"))
    p = subprocess.run([cli, "readjoiner", "overlap", "-readset", idx, "-l", "20", "-q"], capture_output=True, text=True)
    assert p.returncode == 1 and p.stdout == "" and not os.path.exists(idx + ".0.spm")
    assert p.stderr.startswith("gt readjoiner overlap: error: readset '%s' holds " % idx)
    assert "sequences, counted on both strands, that occur whole at another place of the set" in p.stderr and \
        p.stderr.rstrip().endswith("remove them with gt readjoiner prefilter")
    count = int(p.stderr.split(" holds ")[1].split()[0])
    assert count >= 14 and count % 2 == 0
