"""What one lane of the string-graph kernels does
(genometools_amd/csrc/esa_strgraph_core.h: the edges of a match, the kind of a
vertex, a step of the pointer doubling, the choice between the orientations of
a path, the element and the letter of a symbol), compiled with g++ and run on
the CPU in the steps of the kernels, against the brute force of
tests/strgraph_reference.py: every golden call and every generated shape.  No
GPU: what is left for tests/test_strgraph_gpu.py is the kernels around it, the
sort, the scans and the C ABI."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import assembly_golden as ag
import oracle_util as ou
import spm_reference as sr
import strgraph_reference as sg

ROOT = ou.ROOT
SHIM_SRC = os.path.join(ROOT, "tests", "strgraph_core_shim.cpp")
HEADERS = [os.path.join(ROOT, "genometools_amd", "csrc", h) for h in ("esa_strgraph_core.h", "esa_mstat_search.h")]
SHIM = os.path.join(ROOT, "oracle", "_build", "libstrgraph_core_shim.so")
P, U32, U64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64


@pytest.fixture(scope="module")
def shim():
    ou.build()
    if not os.path.exists(SHIM) or os.path.getmtime(SHIM) < max(os.path.getmtime(f) for f in [SHIM_SRC] + HEADERS):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-shared", "-fPIC", "-o", SHIM, SHIM_SRC], check=True)
    lib = ctypes.CDLL(SHIM)
    lib.sg_shim_edge.argtypes = [P, U32, P, P]
    lib.sg_shim_rank_step.argtypes = [P, P, P]
    for name in ("kind", "junction"):
        getattr(lib, "sg_shim_" + name).argtypes = [U32, U32]
    lib.sg_shim_written.argtypes = [U32, U32, U32, U32]
    lib.sg_shim_single_written.argtypes = [U32, U32]
    lib.sg_shim_cycle_written.argtypes = [U32, U32]
    lib.sg_shim_kept.argtypes = [U64, U64, U32, U32]
    lib.sg_shim_element_of.argtypes = [P, U64, U64, U64]
    lib.sg_shim_element_of.restype = U64
    lib.sg_shim_run.argtypes = [P, U64, P, U64, U32, U32, U32, P, U64, P, U64, P]
    lib.sg_shim_run.restype = ctypes.c_int64
    return lib


def run(lib, reads, records, min_len, depthcutoff, lengthcutoff):
    """(contig rows, symbols, figures) of the shim, or its refusal"""
    enc = sr.joined(reads) if len(reads) else np.zeros(0, dtype=np.uint8)
    records = np.ascontiguousarray(records, dtype=np.uint64).reshape(-1, 4)
    most = max(1, 2 * records.shape[0])
    rows = np.zeros((most, 5), dtype=np.uint64)
    symbols = np.full(int(enc.size) * 2 + 1, 9, dtype=np.uint8)
    figures = np.zeros(9, dtype=np.uint64)
    C = lib.sg_shim_run(enc.ctypes.data, enc.size, records.ctypes.data, records.shape[0], min_len, depthcutoff, lengthcutoff,
                        rows.ctypes.data, most, symbols.ctypes.data, symbols.size, figures.ctypes.data)
    if C < 0:
        return C
    return rows[:C], symbols[:int(figures[2])], dict(zip(
        ("contigs", "elements", "symbols", "rounds", "cycle_rounds", "paths", "cycles", "internal", "edges"), figures.tolist()))


def agree(rows, symbols, want):
    """contig records and symbols are those of the brute force's contigs"""
    assert rows.shape[0] == len(want)
    at = 0
    for row, (sym, depth, first, last) in zip(rows.tolist(), want):
        assert row == [sym.size, depth, first, last, at]
        assert np.array_equal(symbols[at:at + sym.size], sym)
        at += sym.size
    assert at == symbols.size


def test_the_edges_of_the_strand_cases(shim):
    """the three cases a list can hold; the fourth of the reference, both reads
    reversed (flags 0), is refused before an edge is made: test_records_outside_the_read_set_are_refused"""
    for flags in (1, 2, 3):
        for sn, pn in ((3, 8), (8, 3), (0, 1)):
            rec = np.array([sn, pn, 12, flags], dtype=np.uint64)
            got = []
            for second in (0, 1):
                a, b = U32(), U32()
                shim.sg_shim_edge(rec.ctypes.data, second, ctypes.byref(a), ctypes.byref(b))
                got.append((a.value, b.value))
            assert tuple(got) == sg.edge_pair(sn, pn, flags)
            assert got[1] == (got[0][1] ^ 1, got[0][0] ^ 1)        # mirror images


def test_classification(shim):
    for outdeg in range(4):
        for indeg in range(4):
            kind = shim.sg_shim_kind(outdeg, indeg)
            assert kind == (2 if outdeg == indeg == 1 else 1 if outdeg else 0)
            assert bool(shim.sg_shim_junction(outdeg, indeg)) == ((outdeg > 1 and indeg > 0) or (outdeg == 1 and indeg > 1))


def test_one_doubling_step(shim):
    a = np.array([7, 2, 30, 5, 6], dtype=np.uint32)
    b = np.array([11, 4, 50, 3, 9], dtype=np.uint32)
    out = np.zeros(5, dtype=np.uint32)
    shim.sg_shim_rank_step(a.ctypes.data, b.ctypes.data, out.ctypes.data)
    assert out.tolist() == [11, 6, 80, 3, 9]
    b[3] = 8
    shim.sg_shim_rank_step(a.ctypes.data, b.ctypes.data, out.ctypes.data)
    assert out.tolist() == [11, 6, 80, 5, 9]


def test_orientation_choice(shim):
    # the start of the mirror image is other(t): 9 ^ 1 = 8
    assert shim.sg_shim_written(4, 0, 9, 0) and not shim.sg_shim_written(8, 0, 5, 0)
    assert shim.sg_shim_written(4, 2, 9, 0) and not shim.sg_shim_written(10, 0, 9, 5)
    # a hairpin: t = other(i), both start at i and the smaller edge number decides
    assert shim.sg_shim_written(6, 0, 7, 1) and not shim.sg_shim_written(6, 1, 7, 0)
    assert shim.sg_shim_written(7, 2, 6, 3) and not shim.sg_shim_written(7, 3, 6, 2)
    # a single edge: the marks, not the mirror image
    assert shim.sg_shim_single_written(3, 4) and not shim.sg_shim_single_written(4, 3)
    assert shim.sg_shim_cycle_written(2, 3) and not shim.sg_shim_cycle_written(3, 2)
    assert shim.sg_shim_kept(3, 100, 3, 100) and not shim.sg_shim_kept(2, 100, 3, 100) and not shim.sg_shim_kept(3, 99, 3, 100)


def test_element_search(shim):
    rng = np.random.default_rng(3)
    start = np.concatenate([[0], np.cumsum(rng.integers(1, 40, 300))]).astype(np.uint64)
    want = np.searchsorted(start, np.arange(int(start[-1])), side="right") - 1
    for s in range(0, int(start[-1]), 7):
        assert shim.sg_shim_element_of(start.ctypes.data, 0, start.size - 1, s) == want[s]
        a = max(0, int(want[s]) - 3)
        assert shim.sg_shim_element_of(start.ctypes.data, a, min(start.size - 1, int(want[s]) + 2), s) == want[s]


@pytest.mark.parametrize("name,which,key", ag.CALLS)
def test_every_golden_call(shim, name, which, key):
    reads, records, _ = ag.call(name, which, key)
    rows, symbols, fig = run(shim, reads, records, *ag.options(name, key))
    agree(rows, symbols, sg.contigs(reads, records, *ag.options(name, key)))
    if name == "circ" and key != "l":
        assert fig["cycles"] == 1 and fig["cycle_rounds"] >= 1


@pytest.mark.parametrize("name", sorted(ag.generated()))
def test_generated_shapes(shim, name):
    reads, records, min_len, depthcutoff, lengthcutoff = ag.generated()[name]
    sg.check_records(reads, records)
    rows, symbols, fig = run(shim, reads, records, min_len, depthcutoff, lengthcutoff)
    agree(rows, symbols, sg.contigs(reads, records, min_len, depthcutoff, lengthcutoff))
    if name.startswith("chain"):
        count = int(name[5:])
        internal = max(count - 2, 0)                       # internal vertices of one orientation
        assert fig["rounds"] == (0 if internal == 0 else max(1, int(np.ceil(np.log2(internal)))) if internal > 1 else 1)


def test_the_rounds_of_the_chains_reach_from_one_to_eight(shim):
    seen = set()
    for count in (2, 3, 64, 65, 130, 200):
        reads, records = sg.chain(count)
        seen.add(run(shim, reads, records, 0, 1, 1)[2]["rounds"])
    assert {0, 1, 6, 8} <= seen


def test_records_outside_the_read_set_are_refused(shim):
    reads, records = sg.chain(4)
    for bad in ([4, 0, 5, 3], [0, 9, 5, 3], [0, 1, 21, 3], [0, 1, 5, 4], [0, 1, 5, 0]):
        assert run(shim, reads, np.concatenate([records, np.array([bad], dtype=np.uint64)]), 0, 1, 1) == -1
