#!/usr/bin/env python3
"""Time "reads in, overlaps out" (include/gtamd_spm.h) on synthetic reads:

  timeout -k 10 900 python tools/spm_probe.py --n 16e6 --coverage 20 --read-length 100 -l 45

Reads of --read-length letters are cut at random places from the --n symbols of
synthetic text --model (default: the human-like DNA of tools/maxpairs_probe.py)
until they cover it --coverage times; a place whose read would hold a special is
drawn again, half of the reads are reverse-complemented.  The reads are
mirrored, as `gt encseq2spm` does; the engine builds .suf and .lcp of the
mirrored set; then prepare and the emit calls into one device buffer of
--capacity records, twice.  Printed: the engine's build time beside prepare and
emit, reads per second and matches per second over prepare + emit (wall), and
the info struct.

  python tools/spm_probe.py --n 16e6 --write-fasta DIR

needs no device: it writes DIR/reads.fna, the same reads, for `gt encseq encode`
and `gt encseq2spm -l 45 -spm count` of the reference on the CPU.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from genometools_amd import synth  # noqa: E402


def make_reads(a):
    """(reads, read length) -- a uint8 matrix, one read a row, on the CPU: the same
    for the device and for the file"""
    n, k = int(a.n), int(a.read_length)
    text = synth.generate(a.model, a.seed, n)
    count = int(n * a.coverage) // k
    rng = np.random.default_rng(a.seed + 1)
    specials = np.concatenate([[0], np.cumsum(text >= 254)])
    starts = rng.integers(0, n - k + 1, count)
    while True:
        bad = np.flatnonzero(specials[starts + k] != specials[starts])
        if bad.size == 0:
            break
        starts[bad] = rng.integers(0, n - k + 1, bad.size)
    reads = np.empty((count, k), dtype=np.uint8)
    for first in range(0, count, 1 << 18):                  # (block by block: the index matrix is 8 bytes a letter)
        block = starts[first:first + (1 << 18)]
        reads[first:first + block.size] = text[block[:, None] + np.arange(k)[None, :]]
    flip = np.flatnonzero(rng.random(count) < 0.5)
    reads[flip] = 3 - reads[flip][:, ::-1]
    return reads


def joined(reads):
    """the reads as one sequence set: a separator between two of them"""
    out = np.full((reads.shape[0], reads.shape[1] + 1), 255, dtype=np.uint8)
    out[:, :-1] = reads
    return out.reshape(-1)[:-1]


def write_fasta(path, reads):
    letters = np.frombuffer(b"acgt", dtype=np.uint8)
    with open(path, "wb") as f:
        for first in range(0, reads.shape[0], 1 << 16):
            block = reads[first:first + (1 << 16)]
            lines = np.full((block.shape[0], block.shape[1] + 1), ord("\n"), dtype=np.uint8)
            lines[:, :-1] = letters[block]
            for k, line in enumerate(lines):
                f.write(b">r%d\n" % (first + k))
                f.write(line.tobytes())


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
    reads = make_reads(a)
    what = "model %d seed %d n %d: %d reads of %d letters (coverage %g)" % (
        a.model, a.seed, int(a.n), reads.shape[0], reads.shape[1], a.coverage)
    if a.write_fasta:
        os.makedirs(a.write_fasta, exist_ok=True)
        write_fasta(os.path.join(a.write_fasta, "reads.fna"), reads)
        print("%s: written to %s" % (what, a.write_fasta))
        return 0

    import torch
    from genometools_amd import esa, spm
    both = spm.mirrored(joined(reads))
    n = both.size
    d_both = torch.from_numpy(both).to("cuda:0")
    torch.cuda.synchronize()
    with esa.EsaEngine(n, 4) as eng, spm.SuffixPrefixMatches() as sp:
        for attempt in ("first build", "second build"):
            t0 = time.time()
            eng.set_sequence_device(d_both.data_ptr(), n)
            eng.run(esa.WANT_SUF | esa.WANT_LCP)
            print("%s; both strands %d symbols; %s %.1f ms (engine total_ms), %.1f ms wall" % (
                what, n, attempt, eng.timing()["total_ms"], 1e3 * (time.time() - t0)), flush=True)
        sp.set_index_engine(eng, d_both.data_ptr(), n)
        for attempt in ("first call", "second call"):
            t0 = time.time()
            info = sp.prepare(a.min_len)
            t1 = time.time()
            calls = records = 0
            for chunk in sp.matches(int(a.capacity), device=True):
                calls += 1
                records += chunk.shape[0]
            torch.cuda.synchronize()
            t2 = time.time()
            assert records == info["matches"]
            wall = max(t2 - t0, 1e-9)
            print("%-11s min_len %d: prepare %9.2f ms on the device (%.2f ms wall), emit %.2f ms wall in %d calls of "
                  "at most %d records: %.3g reads/s, %.3g matches/s; %s" % (
                      attempt, a.min_len, info["device_ms"], 1e3 * (t1 - t0), 1e3 * (t2 - t1), calls, int(a.capacity),
                      reads.shape[0] / wall, records / wall, info), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
