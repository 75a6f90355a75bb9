#!/usr/bin/env python3
"""Time "filtered reads and their overlaps in, contigs out"
(include/gtamd_strgraph.h) on the synthetic reads of tools/prefilter_probe.py:

  timeout -k 10 900 python tools/assembly_probe.py --n 2e6 --coverage 20 --read-length 100 --duplicates 0.2 -l 45

The reads of tools/prefilter_probe.py (same model, seed, coverage, length and
duplicates), filtered on the device (strict), their irreducible overlaps of at
least -l letters found on the device (spmred.IrreducibleMatches), the list kept
there; then, twice: the string graph, its ranking, the selection and the
scatter (StringGraph.prepare) and the spelling of every symbol.  Printed: the
device time of every stage with the rounds of the ranking, reads per second by
stage, and the figures of the graph.  The contigs of the second call are those
of the first; a sample of them is checked against the reads.  It claims no
number.

  python tools/assembly_probe.py --n 2e6 --duplicates 0.2 --write-fasta DIR

needs no device: it writes DIR/reads.fna, the same reads, for `gt readjoiner
prefilter`, `overlap -l` and `assembly` of the reference on the CPU.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import prefilter_probe  # noqa: E402
import spm_probe  # noqa: E402
from genometools_amd import synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=float, default=2e6)
    ap.add_argument("--model", type=int, default=synth.MODEL_HUMANLIKE_DNA)
    ap.add_argument("--seed", type=int, default=43)
    ap.add_argument("--coverage", type=float, default=20)
    ap.add_argument("--read-length", type=int, default=100)
    ap.add_argument("--duplicates", type=float, default=0.2)
    ap.add_argument("-l", type=int, default=45, dest="min_len")
    ap.add_argument("--write-fasta", metavar="DIR")
    a = ap.parse_args()
    reads = prefilter_probe.with_duplicates(spm_probe.make_reads(a), a.duplicates, a.seed + 2)
    what = "model %d seed %d n %d: %d reads of %d letters (coverage %g), %g of them copies" % (
        a.model, a.seed, int(a.n), reads.shape[0], reads.shape[1], a.coverage, a.duplicates)
    if a.write_fasta:
        os.makedirs(a.write_fasta, exist_ok=True)
        spm_probe.write_fasta(os.path.join(a.write_fasta, "reads.fna"), reads)
        print("%s: written to %s" % (what, a.write_fasta))
        return 0

    import torch
    from genometools_amd import contained, esa, spmred, strgraph
    t0 = time.time()
    kept, _, pre = contained.prefilter(spm_probe.joined(reads), strict=True)
    kept = torch.from_numpy(kept).to("cuda:0")
    R = int((kept == 255).sum().item()) + 1
    print("%s; %d reads left by the strict prefilter in %.1f ms wall" % (what, R, 1e3 * (time.time() - t0)), flush=True)
    with contained.ContainedReads() as ct:
        both = ct.mirrored_device(kept)
    with esa.EsaEngine(both.numel(), 4) as eng, spmred.IrreducibleMatches() as im:
        t0 = time.time()
        eng.set_sequence_device(both.data_ptr(), both.numel())
        eng.run(esa.WANT_SUF | esa.WANT_LCP)
        im.set_index_engine(eng, both.data_ptr(), both.numel())
        over = im.prepare(a.min_len)
        chunks = [c.clone() for c in im.matches(device=True)]
        records = torch.cat(chunks) if chunks else torch.zeros((0, 4), dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        print("%d irreducible matches of at least %d letters in %.1f ms wall (build %.1f ms, matches %.1f ms on the device)"
              % (records.shape[0], a.min_len, 1e3 * (time.time() - t0), eng.timing()["total_ms"], over["device_ms"]),
              flush=True)
    first = None
    with strgraph.StringGraph() as graph:
        graph.set_reads(kept)
        graph.set_matches(records)
        for attempt in ("first call", "second call"):
            t0 = time.time()
            info = graph.prepare(0)
            t1 = time.time()
            symbols = torch.cat([c.clone() for c in graph.symbols(capacity=1 << 26, device=True)]) if info["total_length"] \
                else torch.zeros(0, dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()
            t2 = time.time()
            info = graph.info()
            print("%-11s graph %.3f ms, ranking %.3f ms (%d + %d rounds), selection %.3f ms, scatter %.3f ms, spelling %.3f ms "
                  "on the device; prepare %.2f ms wall, spelling %.2f ms wall" % (
                      attempt, info["build_ms"], info["rank_ms"], info["doubling_rounds"], info["cycle_rounds"],
                      info["select_ms"], info["scatter_ms"], info["spell_ms"], 1e3 * (t1 - t0), 1e3 * (t2 - t1)), flush=True)
            for stage in ("build_ms", "rank_ms", "select_ms", "scatter_ms", "spell_ms"):
                print("    %-10s %8.1f M reads/s" % (stage[:-3], R / max(info[stage], 1e-6) / 1e3))
            print("    %s" % info, flush=True)
            if first is None:
                first = symbols
            assert torch.equal(first, symbols), "the second call spells other contigs"
        rows = np.concatenate(list(graph.contigs()))
    # a sample of the contigs against the reads: the first read of a contig starts it
    host, sym = kept.cpu().numpy(), first.cpu().numpy()
    starts = np.concatenate([[0], np.flatnonzero(host == 255) + 1])
    for length, depth, v, _, offset in rows[:: max(1, rows.shape[0] // 200)].tolist():
        r = host[starts[v >> 1]:starts[v >> 1] + a.read_length]
        r = r if v & 1 else (3 - r[::-1])
        assert np.array_equal(sym[offset:offset + r.size], r), "a contig does not start with its first read"
    lengths = np.sort(rows[:, 0])[::-1]
    half = np.searchsorted(np.cumsum(lengths), lengths.sum() / 2)
    print("%d contigs, %d letters, longest %d, N50 %d; a sample checked against the reads" % (
        rows.shape[0], int(lengths.sum()), int(lengths[0]) if lengths.size else 0, int(lengths[half]) if lengths.size else 0))
    return 0


if __name__ == "__main__":
    sys.exit(main())
