"""Contigs of the string graph on the device (include/gtamd_strgraph.h,
genometools_amd/strgraph.py): every call recorded from `gt readjoiner assembly`
in tests/golden/golden_assembly.json -- X.contigs.fas by md5, from the
reference's list and from its shuffled order -- and generated shapes against
the brute force of tests/strgraph_reference.py, every contig record and every
symbol.

The shapes are the smallest at which each part can go wrong: chains whose
ranking takes 1 to 8 rounds and is longer than a wave, cycles, a hairpin, a
vertex with three out-edges, a match of a read with itself, a minimum length
that turns internal vertices into ends, depth and length at and below their
cutoffs; and several thousand chains of three reads, which take the edges, the
vertices, the contigs, the separators and the symbols of an emit call past the
first workgroup (strgraph.geometry()), the sort past its first tile and the
offsets scan past its first 256 tile sums."""
import hashlib

import numpy as np
import pytest

import assembly_golden as ag
import spm_reference as sr
import strgraph_reference as sg
from genometools_amd import _lib, strgraph

pytestmark = pytest.mark.gpu

TILE, SEP_TILE, LEAST = strgraph.geometry()


@pytest.fixture(scope="module")
def graph(gpu):
    with strgraph.StringGraph() as g:
        yield g


def joined(reads):
    return sr.joined(reads) if len(reads) else np.zeros(0, dtype=np.uint8)


def run(graph, reads, records, min_len, depthcutoff, lengthcutoff, capacity=strgraph.DEFAULT_CAPACITY):
    graph.set_reads(joined(reads))
    graph.set_matches(records)
    return graph.all_contigs(min_len, depthcutoff, lengthcutoff, capacity)


def agree(rows, symbols, want):
    """contig records and symbols are those of the brute force's contigs"""
    assert rows.shape[0] == len(want)
    at = 0
    for row, (sym, depth, first, last) in zip(rows.tolist(), want):
        assert row == [sym.size, depth, first, last, at]
        assert np.array_equal(symbols[at:at + sym.size], sym)
        at += sym.size
    assert at == symbols.size


@pytest.mark.parametrize("name,which,key", ag.CALLS)
def test_every_golden_call(graph, name, which, key):
    reads, records, want = ag.call(name, which, key)
    rows, symbols, info = run(graph, reads, records, *ag.options(name, key))
    raw = strgraph.fasta(rows, symbols)
    assert (hashlib.md5(raw).hexdigest(), len(raw)) == (want["md5"], want["size"])
    assert sg.stdout_of(info["reads"], rows[:, 0].tolist()).decode() == want["stdout"]
    agree(rows, symbols, sg.contigs(reads, records, *ag.options(name, key)))
    assert info["reads"] == len(reads) and info["vertices"] == 2 * len(reads) and info["matches"] == records.shape[0]
    if name == "circ" and key != "l":
        assert info["cycles"] == 1 and info["cycle_vertices"] == 2 * len(reads) and info["cycle_rounds"] >= 1


SHAPES = ag.generated()


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_generated_shapes(graph, name):
    reads, records, min_len, depthcutoff, lengthcutoff = SHAPES[name]
    want = sg.contigs(reads, records, min_len, depthcutoff, lengthcutoff)
    rows, symbols, info = run(graph, reads, records, min_len, depthcutoff, lengthcutoff)
    agree(rows, symbols, want)
    assert strgraph.fasta(rows, symbols) == sg.fasta(want)
    assert info["contigs"] == len(want) and info["total_length"] == symbols.size
    assert info["elements"] == sum(c[1] for c in want)
    assert info["longest_contig"] == max([c[0].size for c in want], default=0)
    lengths = [len(r) for r in reads]
    adj = sg.build_graph(lengths, records, min_len)
    assert info["edges"] == sum(len(e) for e in adj)
    assert info["internal_vertices"] == sum(sg.is_internal(adj, v) for v in range(len(adj)))
    # the rounds: at most ceil(log2(2R)) + 1, and what a chain of that many internal vertices takes
    assert info["doubling_rounds"] <= int(np.ceil(np.log2(max(2, 2 * len(reads))))) + 1
    if name.startswith("chain"):
        internal = int(name[5:]) - 2
        assert info["doubling_rounds"] == (0 if internal <= 0 else max(1, int(np.ceil(np.log2(internal)))))
    if name == "two_circles":
        assert info["cycles"] == 2 and info["paths"] == 1
    if name == "hairpin":
        assert rows[0, 2] ^ 1 == rows[0, 3]
    if name == "junction3":
        assert max(len(e) for e in adj) == 3
    if name == "empty_list":
        assert info["contigs"] == info["edges"] == 0 and symbols.size == 0


def test_several_thousand_chains_pass_the_first_tiles(graph):
    """9000 chains of three reads: 36 000 slots are more than two tiles of 4096
    pairs of the radix sort, their 72 000 verdicts more than the 256 tile sums of
    256 counts that one step of the 64-bit offsets scan takes (esa_prims.h), and
    edges, vertices, contigs, separators and the symbols of an emit call are
    many workgroups"""
    chains = max(9000, 35 * TILE)
    reads, records = sg.disjoint_chains(chains, length=12, step=5)
    assert joined(reads).size > 2 * SEP_TILE and records.shape[0] * 2 > 2 * 4096 and records.shape[0] * 4 > 256 * 256
    want = sg.contigs(reads, records, 0, 1, 1)
    assert len(want) == chains
    rows, symbols, info = run(graph, reads, records, 0, 1, 1, capacity=LEAST)      # the smallest pieces an emit call gives
    agree(rows, symbols, want)
    assert info["paths"] == chains and info["elements"] == 3 * chains and symbols.size > 2 * LEAST
    assert info["edges"] == 2 * records.shape[0] and info["internal_vertices"] == 2 * chains
    # a piece from the middle, of a size that is no multiple of anything
    got = next(graph.symbols(capacity=LEAST + 31, cursor=LEAST + 5))
    assert np.array_equal(got, symbols[LEAST + 5:2 * LEAST + 36])
    got = next(graph.contigs(capacity=LEAST, cursor=TILE + 3))
    assert np.array_equal(got, rows[TILE + 3:TILE + 3 + LEAST])
    # the same chains in a shuffled list: the sort has work to do in every tile
    order = np.random.default_rng(4).permutation(records.shape[0])
    rows, symbols, _ = run(graph, reads, records[order], 0, 1, 1)
    agree(rows, symbols, sg.contigs(reads, records[order], 0, 1, 1))


def test_the_list_on_the_device_gives_the_same(graph):
    import torch
    for name in ("rep3", "inv", "circ"):
        reads, records, _ = ag.call(name, "calls", "d1l1")
        host = run(graph, reads, records, 0, 1, 1)
        graph.set_reads(torch.from_numpy(joined(reads)).cuda())
        graph.set_matches(torch.from_numpy(records.astype(np.int64)).cuda())
        rows, symbols, _ = graph.all_contigs(0, 1, 1)
        assert np.array_equal(rows, host[0]) and np.array_equal(symbols, host[1]) and rows.shape[0]
        pieces = [c.cpu().numpy().astype(np.uint64) for c in graph.contigs(capacity=LEAST, device=True)]
        assert np.array_equal(np.concatenate(pieces), host[0])
        pieces = [c.cpu().numpy() for c in graph.symbols(capacity=LEAST, device=True)]
        assert np.array_equal(np.concatenate(pieces), host[1])


def test_the_matcher_s_list_on_the_device_gives_the_same(graph):
    """the records IrreducibleMatches hands out in device memory, and the same
    records copied to the host: identical contig records and symbols"""
    import torch
    from genometools_amd import contained, esa, spmred
    reads = ag.reads_of("rep3")
    enc = torch.from_numpy(joined(reads)).cuda()
    with contained.ContainedReads() as ct:
        both = ct.mirrored_device(enc)
    with esa.EsaEngine(both.numel(), 4) as eng, spmred.IrreducibleMatches() as im:
        eng.set_sequence_device(both.data_ptr(), both.numel())
        eng.run(esa.WANT_SUF | esa.WANT_LCP)
        im.set_index_engine(eng, both.data_ptr(), both.numel())
        info = im.prepare(ag.GOLDEN["rep3"]["min_len"])
        on_device = torch.cat([c.clone() for c in im.matches(device=True)])
    assert on_device.shape == (info["kept"], 4) and info["kept"] == ag.GOLDEN["rep3"]["matches"]
    graph.set_reads(enc)
    graph.set_matches(on_device)
    rows, symbols, _ = graph.all_contigs(0, 1, 1)
    host = run(graph, reads, on_device.cpu().numpy().astype(np.uint64), 0, 1, 1)
    assert np.array_equal(rows, host[0]) and np.array_equal(symbols, host[1]) and rows.shape[0] > 3
    agree(rows, symbols, sg.contigs(reads, on_device.cpu().numpy().astype(np.uint64), 0, 1, 1))
    # a tensor of another type or shape is no list
    for bad in (on_device.to(torch.int32), on_device.reshape(-1)):
        with pytest.raises(TypeError):
            graph.set_matches(bad)


@pytest.mark.parametrize("name", ag.E2E_SETS)
def test_reads_to_contigs_on_the_device(gpu, name):
    """assemble(): this project's prefilter (strict), overlaps and string graph.
    Its list stands in table order, not the reference's, so the contigs are
    compared as a multiset of min(sequence, reverse complement) with those of the
    reference's list, at the default cutoffs (tests/test_assembly_reference.py
    holds that this multiset does not depend on the order of the list)"""
    import prefilter_reference as pr
    import os
    reads, records, _ = ag.call(name, "calls", "default")
    want = sg.canonical(sg.contigs(reads, records))
    raw = pr.parse_reads(os.path.join(ag.DIR, name + ".fna"))
    rows, symbols, info = strgraph.assemble(joined(raw), ag.GOLDEN[name]["min_len"])
    got = sorted(min(s.tobytes(), sg.revcomp(s).tobytes())
                 for s in (symbols[o:o + k] for k, _, _, _, o in rows.tolist()))
    assert got == want
    assert info["overlap"].get("kept", 0) == records.shape[0] and info["reads"] == len(reads)


def test_refusals(graph):
    reads, records = sg.chain(4)
    graph.set_reads(joined(reads))
    for bad, word in (([4, 0, 5, 3], "1 of the 4 matches"), ([0, 1, 21, 3], "1 of the 4 matches"), ([0, 1, 5, 0], "flags")):
        graph.set_matches(np.concatenate([records, np.array([bad], dtype=np.uint64)]))
        with pytest.raises(_lib.EsaError, match=word):
            graph.prepare()
        with pytest.raises(_lib.EsaError, match="nothing is prepared"):
            next(graph.contigs())
    graph.set_matches(records)
    graph.prepare(0, 1, 1)
    with pytest.raises(_lib.EsaError, match="capacity"):
        next(graph.symbols(capacity=LEAST - 1))
    with pytest.raises(_lib.EsaError, match="cursor"):
        next(graph.contigs(cursor=2))
    with strgraph.StringGraph() as fresh:
        with pytest.raises(_lib.EsaError, match="no read set"):
            fresh.prepare()
