"""`gt-suffixerator-amd readjoiner prefilter` on the device, from reads in to X.esq
out: on every set of reads of one length of tests/golden/golden_prefilter.json the
stdout (default, -v, -q, -encodeonly) and X.esq, X.p.fas and X.cnt are the
reference's byte for byte; on sets of reads of several lengths, where the
reference departs from its definition (include/gtamd_contained.h), they are the
brute force's of tests/prefilter_reference.py; and what -strict leaves goes
through `readjoiner overlap`.  Every case starts the tool: that is what is
tested."""
import hashlib
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import oracle_util as ou
import prefilter_reference as pr
import spm_reference as sr
from genometools_amd import _lib
from test_prefilter_host import _read_esq

pytestmark = pytest.mark.gpu

CLI = os.path.join(_lib.HERE, "gt-suffixerator-amd")
DATA = os.path.join(ou.GOLDEN_DIR, "prefilter")

with open(os.path.join(ou.GOLDEN_DIR, "golden_prefilter.json")) as _f:
    GOLDEN = json.load(_f)


def _tool(cwd, files, readset, *options, tool="prefilter"):
    args = ["-db"] + list(files) + ["-readset", readset] if tool == "prefilter" else ["-readset", readset]
    p = subprocess.run([CLI, "readjoiner", tool] + args + list(options), cwd=cwd, capture_output=True, timeout=120)
    return p.returncode, p.stdout, p.stderr.decode()


def _digest(path):
    raw = open(path, "rb").read()
    return {"md5": hashlib.md5(raw).hexdigest(), "size": len(raw)}


def _written(cwd, readset, files=()):
    """the endings of the files of a readset, the input files apart"""
    return sorted(f[len(readset) + 1:] for f in os.listdir(cwd) if f.startswith(readset + ".") and f not in files)


@pytest.mark.parametrize("name", sorted(GOLDEN["equal"]))
def test_reads_of_one_length_are_the_reference_s(gpu, name, tmp_path):
    golden = GOLDEN["equal"][name]
    cwd = str(tmp_path)
    for f in golden["files"]:
        shutil.copy(os.path.join(DATA, f), cwd)
    assert _tool(cwd, golden["files"], name) == (0, golden["stdout"].encode(), "")
    assert _written(cwd, name, golden["files"]) == ["esq"] and _digest(os.path.join(cwd, name + ".esq")) == golden["esq"]
    assert _tool(cwd, golden["files"], name, "-v", "-fasta", "-cnt") == (0, golden["stdout_v"].encode(), "")
    assert _written(cwd, name, golden["files"]) == ["cnt", "esq", "p.fas"]
    for ext in ("esq", "p.fas", "cnt"):
        assert _digest(os.path.join(cwd, "%s.%s" % (name, ext))) == golden[ext], ext
    os.remove(os.path.join(cwd, name + ".esq"))
    assert _tool(cwd, golden["files"], name, "-q") == (0, b"", "")
    assert _digest(os.path.join(cwd, name + ".esq")) == golden["esq"]
    assert _tool(cwd, golden["files"], name, "-v", "-encodeonly") == (0, golden["stdout_encodeonly"].encode(), "")
    assert _digest(os.path.join(cwd, name + ".esq")) == golden["esq_encodeonly"]


def _variable_sets(tmp):
    """name -> files: the two sets of the golden file and one of two files, FASTQ and FASTA over several lines,
    with a read that holds a wildcard"""
    sets = {name: e["files"] for name, e in GOLDEN["variable"].items()}
    for files in sets.values():
        for f in files:
            shutil.copy(os.path.join(DATA, f), tmp)
    a, b = pr.seeded_reads(221, (20, 60)), pr.seeded_reads(222, (20, 60))
    wild = a[7].copy()
    wild[3] = 254
    pr.write_fastq(os.path.join(tmp, "mixed_a.fq"), a[:40] + [wild] + [b[5]])
    pr.write_fasta(os.path.join(tmp, "mixed_b.fna"), b[:50] + [a[2][:15]], width=25)
    sets["mixed"] = ["mixed_a.fq", "mixed_b.fna"]
    return sets


@pytest.mark.parametrize("strict", [False, True])
def test_reads_of_several_lengths_are_the_definition_s(gpu, strict, tmp_path):
    cwd = str(tmp_path)
    for name, files in sorted(_variable_sets(cwd).items()):
        _, valid = pr.file_figures([os.path.join(cwd, f) for f in files])
        reads = [r for r, _ in valid]
        v = pr.verdicts(reads)
        kept = pr.kept_reads(reads, v, strict)
        options = ["-strict"] if strict else []
        cur = os.getcwd()
        os.chdir(cwd)
        try:
            want = [pr.expected_stdout(name, files, mode, strict, fasta=True, cnt=True) for mode in ("default", "verbose")]
        finally:
            os.chdir(cur)
        assert _tool(cwd, files, name, "-fasta", "-cnt", *options) == (0, want[0], "")
        assert _tool(cwd, files, name, "-v", "-fasta", "-cnt", *options) == (0, want[1], "")
        assert open(os.path.join(cwd, name + ".p.fas"), "rb").read() == pr.p_fas(kept)
        assert np.array_equal(_read_esq(os.path.join(cwd, name)), sr.joined(kept))
        mask = pr.STRICT_MASK if strict else pr.DEFAULT_MASK
        assert open(os.path.join(cwd, name + ".cnt"), "rb").read() == pr.cntlist(mask >> v & 1)
        assert "rlt" not in _written(cwd, name, files)
        # the next step of the assembler takes what -strict leaves, and refuses what the default leaves of these
        rc, out, err = _tool(cwd, files, name, "-l", "12", tool="overlap")
        if strict:
            assert (rc, err) == (0, "") and b"# number of reads in filtered readset = %d\n" % len(kept) in out
        else:
            assert pr.tallies(v)["internal"] + pr.tallies(v)["self_complementary"] > 0
            assert rc == 1 and err.rstrip().endswith("remove them with gt readjoiner prefilter")


def test_nothing_is_left(gpu, tmp_path):
    cwd = str(tmp_path)
    wild = np.array([0, 1, 254, 2, 3, 0, 1], dtype=np.uint8)
    pr.write_fasta(os.path.join(cwd, "none.fna"), [wild, wild[::-1], wild])
    lines = b"".join(b"# %s\n" % l for l in (
        b"gt readjoiner prefilter (version 1.2)", b"number of reads in complete readset = 3", b"low-quality reads = 3",
        b"contained reads = 0", b"number of reads in filtered readset = 0",
        b"no readset saved as no sequence passed the filters"))
    assert _tool(cwd, ["none.fna"], "none", "-fasta", "-cnt") == (0, lines, "")
    assert _written(cwd, "none", ["none.fna"]) == ["cnt", "p.fas"]
    assert open(os.path.join(cwd, "none.p.fas"), "rb").read() == b""
    assert open(os.path.join(cwd, "none.cnt"), "rb").read() == pr.cntlist([])


def test_the_default_readset_name_and_the_errors_of_the_input(gpu, tmp_path):
    cwd = str(tmp_path)
    shutil.copy(os.path.join(DATA, "dups.fna"), cwd)
    rc, out, err = _tool(cwd, ["dups.fna"], "unused")
    assert rc == 0
    p = subprocess.run([CLI, "readjoiner", "prefilter", "-db", "dups.fna", "-v"], cwd=cwd, capture_output=True)
    assert p.returncode == 0 and b"# readset name = dups.fna\n" in p.stdout
    assert b"# suffix-prefix-free readset saved: dups.fna.esq\n" in p.stdout
    assert _digest(os.path.join(cwd, "dups.fna.esq")) == _digest(os.path.join(cwd, "unused.esq"))
    rc, out, err = _tool(cwd, ["missing.fna"], "X")
    assert rc == 1 and err.startswith("gt readjoiner prefilter: error: cannot open file 'missing.fna'")
    open(os.path.join(cwd, "bad.fna"), "w").write(">r\nacgt!acgt\n")
    rc, out, err = _tool(cwd, ["bad.fna"], "X", "-q")
    assert (rc, out) == (1, b"") and "illegal character '!'" in err
