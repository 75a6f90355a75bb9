#!/usr/bin/env python3
"""Time "reads in, filtered reads out" (include/gtamd_contained.h) on the
synthetic reads of tools/spm_probe.py with a given rate of duplicates:

  timeout -k 10 900 python tools/prefilter_probe.py --n 4e6 --coverage 20 --read-length 100 --duplicates 0.2

The reads of tools/spm_probe.py (same model, seed, coverage and length), of
which --duplicates of the rows are overwritten by copies of other rows, half of
them reverse-complemented.  The reads are mirrored on the device; the engine
builds .suf and .lcp of the mirrored set; then, twice: decide
(contained.ContainedReads) and the compaction.  Printed: the engine's build
time, the device time of the decision with its steps 1 and 2, the wall time of
decision and compaction, reads per second of both, and the counts.  The kept
reads are checked against numpy (of every group of equal reads on either strand
the first stays).  It claims no number.

  python tools/prefilter_probe.py --n 4e6 --duplicates 0.2 --write-fasta DIR

needs no device: it writes DIR/reads.fna, the same reads, for `gt readjoiner
prefilter -db reads.fna` of the reference on the CPU.
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


def with_duplicates(reads, rate, seed):
    rng = np.random.default_rng(seed)
    count = int(reads.shape[0] * rate)
    to = rng.choice(reads.shape[0], count, replace=False)
    src = rng.integers(0, reads.shape[0], count)
    copies = reads[src]
    flip = rng.random(count) < 0.5
    copies[flip] = 3 - copies[flip][:, ::-1]
    reads[to] = copies
    return reads


def first_of_each_group(reads):
    """which reads (rows of one length) are the first of their group of equal reads on either strand"""
    back = 3 - reads[:, ::-1]
    first_diff = np.argmax(reads != back, axis=1)
    rows = np.arange(reads.shape[0])
    smaller = reads[rows, first_diff] <= back[rows, first_diff]
    name = np.where(smaller[:, None], reads, back)
    keys = np.ascontiguousarray(name).view(np.dtype((np.void, reads.shape[1]))).reshape(-1)
    _, first = np.unique(keys, return_index=True)
    keep = np.zeros(reads.shape[0], dtype=bool)
    keep[first] = True
    return keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=float, default=4e6)
    ap.add_argument("--model", type=int, default=synth.MODEL_HUMANLIKE_DNA)
    ap.add_argument("--seed", type=int, default=43)
    ap.add_argument("--coverage", type=float, default=20)
    ap.add_argument("--read-length", type=int, default=100)
    ap.add_argument("--duplicates", type=float, default=0.2)
    ap.add_argument("--write-fasta", metavar="DIR")
    a = ap.parse_args()
    reads = with_duplicates(spm_probe.make_reads(a), a.duplicates, a.seed + 2)
    R = reads.shape[0]
    what = "model %d seed %d n %d: %d reads of %d letters (coverage %g), %g of them copies" % (
        a.model, a.seed, int(a.n), R, reads.shape[1], a.coverage, a.duplicates)
    if a.write_fasta:
        os.makedirs(a.write_fasta, exist_ok=True)
        spm_probe.write_fasta(os.path.join(a.write_fasta, "reads.fna"), reads)
        print("%s: written to %s" % (what, a.write_fasta))
        return 0

    import torch
    from genometools_amd import contained, esa
    keep = first_of_each_group(reads)
    enc = torch.from_numpy(spm_probe.joined(reads)).to("cuda:0")
    with contained.ContainedReads() as ct:
        torch.cuda.synchronize()
        t0 = time.time()
        both = ct.mirrored_device(enc)
        torch.cuda.synchronize()
        print("%s; mirrored on the device in %.2f ms wall, %d symbols" % (what, 1e3 * (time.time() - t0), both.numel()),
              flush=True)
        with esa.EsaEngine(both.numel(), 4) as eng:
            for attempt in ("first build", "second build"):
                t0 = time.time()
                eng.set_sequence_device(both.data_ptr(), both.numel())
                eng.run(esa.WANT_SUF | esa.WANT_LCP)
                print("%s %.1f ms (engine total_ms), %.1f ms wall" % (attempt, eng.timing()["total_ms"],
                                                                     1e3 * (time.time() - t0)), flush=True)
            ct.set_index_engine(eng, both.data_ptr(), both.numel())
            for attempt in ("first call", "second call"):
                t0 = time.time()
                info = ct.decide()
                t1 = time.time()
                left = ct.filtered(device=True)
                torch.cuda.synchronize()
                t2 = time.time()
                print("%-11s decide %9.2f ms on the device (%.2f ms wall; steps 1 and 2 %.2f ms): %.1f M reads/s; compact "
                      "%.2f ms wall: %.1f M reads/s, %d symbols left; %s" % (
                          attempt, info["device_ms"], 1e3 * (t1 - t0), info["lists_ms"], R / (t1 - t0) / 1e6,
                          1e3 * (t2 - t1), R / (t2 - t1) / 1e6, left.numel(), info), flush=True)
            v = ct.verdicts()
            assert np.array_equal(v == contained.DUPLICATE, ~keep), "the duplicates are not numpy's"
            assert np.array_equal(left.cpu().numpy(), spm_probe.joined(reads[v != contained.DUPLICATE]))
            print("kept reads checked against numpy: %d of %d" % (int(keep.sum()), R))
    return 0


if __name__ == "__main__":
    sys.exit(main())
