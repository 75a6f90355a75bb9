"""`gt-suffixerator-amd readjoiner correct` against what the reference did
(tests/golden/golden_correct.json, made by tests/golden/make_golden_correct.py):
every golden call through the tool, INDEX.esq byte for byte the reference's
before and after, nothing on stdout, the exit codes, the refusal of reads of two
lengths with the reference's sentence; the tool run twice against the
restatement applied twice (a second call of the reference walks the tables of
the reads as they were: it is not recorded); and kcorrect.correct() on the same
reads."""
import hashlib
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import kcorrect_reference as kr
import oracle_util as ou
from genometools_amd import _lib, kcorrect

pytestmark = pytest.mark.gpu

CLI = os.path.join(_lib.HERE, "gt-suffixerator-amd")
DATA = os.path.join(ou.GOLDEN_DIR, "correct")

with open(os.path.join(ou.GOLDEN_DIR, "golden_correct.json")) as _f:
    GOLDEN = json.load(_f)


def digest(path):
    with open(path, "rb") as f:
        raw = f.read()
    return {"md5": hashlib.md5(raw).hexdigest(), "size": len(raw)}


def encode(tmp_path, fasta):
    """INDEX.prj, .esq and .ssp of the FASTA file, written with bare names as the golden calls were"""
    shutil.copy(os.path.join(DATA, fasta), tmp_path)
    p = subprocess.run([CLI, "-dna", "-tis", "-ssp", "-mirrored", "-indexname", "reads", "-db", fasta], cwd=tmp_path,
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr


def correct(tmp_path, k, c):
    return subprocess.run([CLI, "readjoiner", "correct", "-k", str(k), "-c", str(c), "-ii", "reads"], cwd=tmp_path,
                          capture_output=True, text=True)


def decoded(tmp_path):
    """the symbols of reads.esq, through the library's reader"""
    import ctypes
    host = ctypes.CDLL(os.path.join(_lib.HERE, "libgtamd_host.so"))
    enc, n, protein = ctypes.c_void_p(), ctypes.c_uint64(), ctypes.c_int()
    err = ctypes.create_string_buffer(2048)
    host.gtamd_read_esq.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_uint64),
                                    ctypes.POINTER(ctypes.c_int), ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t]
    ss = ctypes.create_string_buffer(512)
    rc = host.gtamd_read_esq(os.path.join(str(tmp_path), "reads").encode(), ctypes.byref(enc), ctypes.byref(n),
                             ctypes.byref(protein), ss, err, 2048)
    assert rc == 0, err.value
    out = np.ctypeslib.as_array(ctypes.cast(enc, ctypes.POINTER(ctypes.c_uint8)), shape=(n.value,)).copy()
    ctypes.CDLL(None).free(enc)
    return out


@pytest.mark.parametrize("name", sorted(GOLDEN["sets"]))
def test_golden_call(gpu, tmp_path, name):
    e = GOLDEN["sets"][name]
    encode(tmp_path, e["file"])
    esq = str(tmp_path / "reads.esq")
    assert digest(esq) == e["esq_before"]
    p = correct(tmp_path, e["k"], e["c"])
    assert (p.returncode, p.stdout, p.stderr) == (e["first"]["exit"], e["first"]["stdout"], "")
    assert digest(esq) == e["first"]["esq"]
    reads = [np.array(["acgt".index(ch) for ch in s], dtype=np.uint8) for s in e["first"]["reads"]]
    assert np.array_equal(decoded(tmp_path), kr.joined(reads))


def test_reads_of_two_lengths_are_refused_as_by_the_reference(gpu, tmp_path):
    e = GOLDEN["refusals"]["two_lengths"]
    encode(tmp_path, e["file"])
    before = digest(str(tmp_path / "reads.esq"))
    p = correct(tmp_path, e["k"], e["c"])
    assert (p.returncode, p.stdout) == (e["exit"], e["stdout"])
    assert p.stderr == "gt readjoiner correct: error: %s\n" % e["message"]
    assert digest(str(tmp_path / "reads.esq")) == before


@pytest.mark.parametrize("name", ["planted", "chain"])
def test_twice_and_the_library_call(gpu, tmp_path, name):
    e = GOLDEN["sets"][name]
    reads = kr.parse_fasta(os.path.join(DATA, e["file"]))
    once, _, _ = kr.correct_reads(reads, e["k"], e["c"])
    twice, _, _ = kr.correct_reads(once, e["k"], e["c"])
    encode(tmp_path, e["file"])
    for want in (once, twice):
        p = correct(tmp_path, e["k"], e["c"])
        assert (p.returncode, p.stdout, p.stderr) == (0, "", "")
        assert np.array_equal(decoded(tmp_path), kr.joined(want))
    out, _, _ = kcorrect.correct(kr.joined(reads), e["k"], e["c"])
    assert np.array_equal(out, kr.joined(once))
    assert np.array_equal(kcorrect.correct(out, e["k"], e["c"])[0], kr.joined(twice))
