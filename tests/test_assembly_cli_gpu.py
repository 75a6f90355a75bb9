"""`gt-suffixerator-amd assembly` on the device: for every call recorded from `gt
readjoiner assembly` in tests/golden/golden_assembly.json -- the reference's
list and its shuffled order, default options, cutoffs of 1, a raised -l --
X.contigs.fas has the recorded md5 and the stdout is the reference's byte for
byte; -q; no X.paths; and from reads to contigs with this project's tools alone:
`readjoiner prefilter -strict`, `readjoiner overlap`, `assembly`, whose contigs
are the reference's as a multiset of min(sequence, reverse complement) (the
list stands in table order here, tests/test_assembly_reference.py holds that
this multiset does not depend on it).  Every case starts the tool: that is what
is tested."""
import hashlib
import os
import shutil
import subprocess

import numpy as np
import pytest

import assembly_golden as ag
import strgraph_reference as sg
from genometools_amd import _lib

pytestmark = pytest.mark.gpu

CLI = os.path.join(_lib.HERE, "gt-suffixerator-amd")


@pytest.fixture(scope="module")
def readsets(gpu, tmp_path_factory):
    """name -> readset the tool itself encoded from the reads the list numbers, once"""
    subprocess.run(["make", "-C", os.path.join(_lib.HERE, "csrc", "host")], check=True, stdout=subprocess.DEVNULL)
    root, built = tmp_path_factory.mktemp("assembly"), {}

    def get(name):
        if name not in built:
            idx = str(root / name)
            subprocess.run([CLI, "-dna", "-tis", "-ssp", "-db", os.path.join(ag.DIR, name + ".p.fas"), "-indexname", idx],
                           check=True, stdout=subprocess.DEVNULL)
            built[name] = idx
        return built[name]
    return get


def _run(*args, cwd=None):
    p = subprocess.run([CLI] + list(args), capture_output=True, cwd=cwd, timeout=120)
    assert p.returncode == 0 and p.stderr == b"", (args, p.stderr)
    return p.stdout


def _digest(path):
    with open(path, "rb") as f:
        raw = f.read()
    return hashlib.md5(raw).hexdigest(), len(raw)


@pytest.mark.parametrize("name", sorted(ag.GOLDEN))
def test_every_golden_call(readsets, name):
    idx = readsets(name)
    calls = [(w, k) for n, w, k in ag.CALLS if n == name]
    assert len(calls) == (5 if ag.GOLDEN[name]["matches"] else 4)
    for which, key in calls:
        want = ag.GOLDEN[name][which][key]
        shutil.copy(ag.list_path(name, which), idx + ".0.spm")
        fas = idx + ".contigs.fas"
        if os.path.exists(fas):
            os.remove(fas)
        assert _run("assembly", "-readset", idx, *ag.cli_options(name, key)).decode() == want["stdout"], (which, key)
        assert _digest(fas) == (want["md5"], want["size"]), (which, key)
        assert not os.path.exists(idx + ".paths")
    # -q: the same file, no line
    os.remove(fas)
    assert _run("assembly", "-readset", idx, "-q", *ag.cli_options(name, key)) == b""
    assert _digest(fas) == (want["md5"], want["size"])
    # -spmfiles 1 is the default
    assert _run("assembly", "-readset", idx, "-spmfiles", "1", *ag.cli_options(name, key)).decode() == want["stdout"]


def test_fasta_lines_at_their_borders(gpu, tmp_path):
    """contigs of 59, 60, 61 and 120 letters: a line short of one letter, a full
    line, a line and a letter, two full lines"""
    import prefilter_reference as pr
    import spmred_reference as rr
    shapes = ag.generated()
    reads, records = sg.join(*[shapes["letters%d" % k][:2] for k in (59, 60, 61, 120)])
    cwd = str(tmp_path)
    pr.write_fasta(os.path.join(cwd, "reads.fna"), reads)
    _run("-dna", "-tis", "-ssp", "-db", "reads.fna", "-indexname", "x", cwd=cwd)
    with open(os.path.join(cwd, "x.0.spm"), "wb") as f:
        f.write(rr.bin32(records))
    want = sg.contigs(reads, records, 0, 1, 1)
    assert [c[0].size for c in want] == [59, 60, 61, 120]
    out = _run("assembly", "-readset", "x", "-depthcutoff", "1", "-lengthcutoff", "1", cwd=cwd)
    assert out == sg.stdout(reads, want)
    with open(os.path.join(cwd, "x.contigs.fas"), "rb") as f:
        assert f.read() == sg.fasta(want)


def _contigs_of(path):
    out = []
    with open(path) as f:
        for line in f:
            if line.startswith(">"):
                out.append("")
            else:
                out[-1] += line.strip()
    return [np.array(["acgt".index(c) for c in t], dtype=np.uint8) for t in out]


@pytest.mark.parametrize("name", ag.E2E_SETS)
def test_reads_to_contigs_with_this_project_s_tools(gpu, name, tmp_path):
    cwd = str(tmp_path)
    shutil.copy(os.path.join(ag.DIR, name + ".fna"), cwd)
    _run("readjoiner", "prefilter", "-db", name + ".fna", "-readset", name, "-strict", cwd=cwd)
    _run("readjoiner", "overlap", "-readset", name, "-l", str(ag.GOLDEN[name]["min_len"]), cwd=cwd)
    out = _run("assembly", "-readset", name, cwd=cwd).decode()
    reads, records, want = ag.call(name, "calls", "default")
    found = sg.contigs(reads, records)
    got = _contigs_of(os.path.join(cwd, name + ".contigs.fas"))
    assert sorted(min(c.tobytes(), sg.revcomp(c).tobytes()) for c in got) == sg.canonical(found)
    # the lines that do not depend on the order of the contigs are the reference's
    assert out.splitlines()[:2] == want["stdout"].splitlines()[:2]
    assert sorted(out.splitlines()[7:]) == sorted(want["stdout"].splitlines()[7:])
