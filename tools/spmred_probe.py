#!/usr/bin/env python3
"""Time "reads in, irreducible overlaps out" (include/gtamd_spmred.h) on the
synthetic reads of tools/spm_probe.py, made free of containment:

  timeout -k 10 900 python tools/spmred_probe.py --n 16e6 --coverage 20 --read-length 100 -l 45

The reads of tools/spm_probe.py (same model, seed, coverage and length) without
those that occur a second time, as they stand or reverse-complemented, and
without those equal to their own reverse complement: of every group of equal
reads the first stays.  With reads of one length that is all the containment
there is, and what `gt readjoiner prefilter` would remove.  The reads are
mirrored; the engine builds .suf and .lcp of the mirrored set; then, twice:
prepare and emit of ALL suffix-prefix matches (spm.SuffixPrefixMatches, what the
reduction is measured against), and prepare and emit of the irreducible ones
(spmred.IrreducibleMatches), each into one device buffer of --capacity records.
Printed: the device times of the steps, the closing figures of `gt readjoiner
overlap`, and the info structs.

  python tools/spmred_probe.py --n 16e6 --write-fasta DIR

needs no device: it writes DIR/reads.fna, the same reads, for `gt encseq encode`
and `gt readjoiner overlap -l 45` of the reference on the CPU.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import spm_probe  # noqa: E402
from genometools_amd import synth  # noqa: E402


def containment_free(reads):
    """the reads (rows of one length) without a second occurrence on either strand"""
    back = 3 - reads[:, ::-1]
    # the smaller of a read and its reverse complement names the group
    first_diff = np.argmax(reads != back, axis=1)
    rows = np.arange(reads.shape[0])
    own = (reads == back).all(axis=1)
    smaller = reads[rows, first_diff] <= back[rows, first_diff]
    name = np.where(smaller[:, None], reads, back)
    keys = np.ascontiguousarray(name).view(np.dtype((np.void, reads.shape[1]))).reshape(-1)
    _, first = np.unique(keys, return_index=True)
    keep = np.zeros(reads.shape[0], dtype=bool)
    keep[first] = True
    keep &= ~own
    return reads[keep]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=float, default=16e6)
    ap.add_argument("--model", type=int, default=synth.MODEL_HUMANLIKE_DNA)
    ap.add_argument("--seed", type=int, default=43)
    ap.add_argument("--coverage", type=float, default=20)
    ap.add_argument("--read-length", type=int, default=100)
    ap.add_argument("-l", "--min-len", type=int, default=45)
    ap.add_argument("--capacity", type=float, default=1 << 22)
    ap.add_argument("--write-fasta", metavar="DIR")
    a = ap.parse_args()
    drawn = spm_probe.make_reads(a)
    reads = containment_free(drawn)
    what = "model %d seed %d n %d: %d reads of %d letters drawn (coverage %g), %d left without containment" % (
        a.model, a.seed, int(a.n), drawn.shape[0], drawn.shape[1], a.coverage, reads.shape[0])
    del drawn
    if a.write_fasta:
        os.makedirs(a.write_fasta, exist_ok=True)
        spm_probe.write_fasta(os.path.join(a.write_fasta, "reads.fna"), reads)
        print("%s: written to %s" % (what, a.write_fasta))
        return 0

    import torch
    from genometools_amd import esa, spm, spmred
    both = spm.mirrored(spm_probe.joined(reads))
    n = both.size
    d_both = torch.from_numpy(both).to("cuda:0")
    torch.cuda.synchronize()
    with esa.EsaEngine(n, 4) as eng, spm.SuffixPrefixMatches() as sp, spmred.IrreducibleMatches() as sr:
        for attempt in ("first build", "second build"):
            t0 = time.time()
            eng.set_sequence_device(d_both.data_ptr(), n)
            eng.run(esa.WANT_SUF | esa.WANT_LCP)
            print("%s; both strands %d symbols; %s %.1f ms (engine total_ms), %.1f ms wall" % (
                what, n, attempt, eng.timing()["total_ms"], 1e3 * (time.time() - t0)), flush=True)
        sp.set_index_engine(eng, d_both.data_ptr(), n)
        sr.set_index_engine(eng, d_both.data_ptr(), n)

        def emit(matcher, total):
            torch.cuda.synchronize()
            t0 = time.time()
            calls = records = 0
            for chunk in matcher.matches(int(a.capacity), device=True):
                calls += 1
                records += chunk.shape[0]
            torch.cuda.synchronize()
            assert records == total
            return calls, 1e3 * (time.time() - t0)

        for attempt in ("first call", "second call"):
            t0 = time.time()
            info = sp.prepare(a.min_len)
            t1 = time.time()
            calls, wall = emit(sp, info["matches"])
            print("%-11s all matches,  min_len %d: prepare %9.2f ms on the device (%.2f ms wall), emit %.2f ms wall in "
                  "%d calls of at most %d records; %s" % (attempt, a.min_len, info["device_ms"], 1e3 * (t1 - t0), wall,
                                                         calls, int(a.capacity), info), flush=True)
            t0 = time.time()
            red = sr.prepare(a.min_len)
            t1 = time.time()
            calls, wall = emit(sr, red["kept"])
            pairs = max(red["matches"], 1)
            print("%-11s irreducible,  min_len %d: prepare %9.2f ms on the device (%.2f ms wall): steps 1 to 4 %.2f ms, "
                  "group, decide and place %.2f ms of which decide %.2f ms; emit %.2f ms wall in %d calls; "
                  "%.2f candidates and %.2f letters per pair; closing figures %s; %s" % (
                      attempt, a.min_len, red["device_ms"], 1e3 * (t1 - t0), red["spm_ms"],
                      red["device_ms"] - red["spm_ms"], red["decide_ms"], wall, calls,
                      red["candidates_examined"] / pairs, red["letters_compared"] / pairs,
                      spmred.closing_figures(red, reads.shape[0]), red), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
