"""What one lane of the k-mer correction kernels does
(genometools_amd/csrc/esa_kcorrect_core.h: the group of a child and the records
it gives, the record a record's letter comes from, a round of the pointer
doubling, the final letter of a position), compiled with g++ and run on the CPU
over every child and record of the oracle's tables, against the restatement
tests/kcorrect_reference.py.  No GPU: what is left for
tests/test_kcorrect_gpu.py is the kernels around it, the ballots, the scans, the
sort and the C ABI."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import kcorrect_reference as kr
import oracle_util as ou

ROOT = ou.ROOT
SHIM_SRC = os.path.join(ROOT, "tests", "kcorrect_core_shim.cpp")
HEADERS = [os.path.join(ROOT, "genometools_amd", "csrc", h) for h in ("esa_kcorrect_core.h", "esa_mstat_search.h")]
SHIM = os.path.join(ROOT, "oracle", "_build", "libkcorrect_core_shim.so")
TILE = 256


class Figures(ctypes.Structure):
    _fields_ = [(name, ctypes.c_uint64) for name in ("groups", "untrusted_groups", "records", "dependent", "rounds",
                                                     "changed")] + [("delta", ctypes.c_int64 * 4)]


@pytest.fixture(scope="module")
def shim():
    ou.build()
    if not os.path.exists(SHIM) or os.path.getmtime(SHIM) < max(os.path.getmtime(f) for f in [SHIM_SRC] + HEADERS):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-shared", "-fPIC", "-o", SHIM, SHIM_SRC], check=True)
    lib = ctypes.CDLL(SHIM)
    P = ctypes.c_void_p
    lib.kc_shim_run.argtypes = [P, ctypes.c_uint64, P, ctypes.c_int, P, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32, P,
                                ctypes.c_uint64, P, ctypes.POINTER(Figures)]
    lib.kc_shim_run.restype = ctypes.c_int64
    return lib


def _run(lib, text, t, width, k, c, mirror):
    text = np.ascontiguousarray(text, dtype=np.uint8)
    suf = np.ascontiguousarray(t["suf"].astype(width))
    lcp = np.ascontiguousarray(t["lcp"])
    triples = np.zeros((text.size + 1, 3), dtype=np.uint64)
    out = np.full(text.size >> 1 if mirror else text.size, 77, dtype=np.uint8)
    fig = Figures()
    R = lib.kc_shim_run(text.ctypes.data, text.size, suf.ctypes.data, suf.dtype.itemsize, lcp.ctypes.data, int(mirror), k, c,
                        triples.ctypes.data, text.size + 1, out.ctypes.data, ctypes.byref(fig))
    assert R >= 0
    return out, triples[:R], fig


def _agree(lib, reads, k, c, mirror=True, widths=(np.uint64, np.uint32)):
    """both table widths against the restatement; its info"""
    text = kr.joined(reads)
    if mirror:
        text = kr.mirrored(text)
    t = ou.esa(text, 4)
    want, triples, info = kr.correct(text, k, c, mirror, suf=t["suf"], lcp=t["lcpfull"])
    for width in widths:
        out, got, fig = _run(lib, text, t, width, k, c, mirror)
        assert np.array_equal(out, want), np.flatnonzero(out != want)[:10]
        assert got.tolist() == [list(x) for x in triples]
        assert (fig.groups, fig.untrusted_groups, fig.records, fig.dependent, fig.rounds, fig.changed) == \
            (info["groups"], info["untrusted_groups"], info["records"], info["dependent"], info["rounds"], info["changed"])
        assert list(fig.delta) == info["delta"]
    return info


def test_golden_sets(shim):
    with open(os.path.join(ou.GOLDEN_DIR, "golden_correct.json")) as f:
        golden = json.load(f)
    for name, e in golden["sets"].items():
        reads = kr.parse_fasta(os.path.join(ou.GOLDEN_DIR, "correct", e["file"]))
        info = _agree(shim, reads, e["k"], e["c"])
        assert info["records"] == e["first"]["records"], name


@pytest.mark.parametrize("seed", range(300, 330))
def test_seeded_sets(shim, seed):
    length, count, k = ((20, 24, 6), (12, 40, 4))[seed % 2]
    info = _agree(shim, kr.coverage_reads(seed, length, count), k, 2)
    assert info["records"] >= 1


@pytest.mark.parametrize("mirror", [True, False])
def test_borders_widths_and_tails(shim, mirror):
    for seed in (79, 0):
        _agree(shim, kr.coverage_reads(seed, 20, 60), 6, 2, mirror)
    assert _agree(shim, *kr.width_reads(), mirror)["records"] >= 2
    assert _agree(shim, *kr.invalid_tail_reads(TILE), mirror, widths=(np.uint64,))["records"] >= 1
    assert _agree(shim, *kr.mixed_reads(), mirror)["records"] >= 5


def test_many_records_and_chains(shim):
    assert _agree(shim, *kr.many_records_reads(), widths=(np.uint32,))["records"] > 4096
    info = _agree(shim, *kr.chain_reads(), widths=(np.uint64,))
    assert info["chain"] >= 3 and info["rounds"] >= 2


@pytest.mark.parametrize("k", [254, 255])
def test_the_lcp_byte_suffices_up_to_255(shim, k):
    reads = kr.long_reads()
    info = _agree(shim, reads, k, 2, widths=(np.uint64,))
    assert info["records"] == 2
    assert (ou.esa(kr.mirrored(kr.joined(reads)), 4)["lcp"] == 255).sum() > 10


def test_no_record(shim):
    clean = kr.coverage_reads(8, 40, 120, errors=0.0, genome=200)
    for reads, k, c in ((clean, 13, 3), (clean, 1, 2), (clean, 41, 2), (clean, 40, 2), (clean, 13, 1000)):
        info = _agree(shim, reads, k, c, widths=(np.uint64,))
        assert info["records"] == info["changed"] == info["untrusted_groups"] == 0
