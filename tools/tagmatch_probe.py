#!/usr/bin/env python3
"""Time the approximate matches of short tags (include/gtamd_tagmatch.h) against
the resident suffix table of one build:

  timeout -k 10 900 python tools/tagmatch_probe.py --n 256e6 --tags 1e6 --len 32 -e 0 1 2

The tags are --len letters cut from random places of the subject (a wildcard
inside becomes a letter), every one with --edits random replacements,
insertions or deletions, every second reverse-complemented.  One build with
.suf, then per K: prepare (the count passes and the offsets) and the emit calls
into one device buffer of --capacity records; the info struct, the device time
of the prepare, tags per second over prepare + emit (wall) and the children
examined per tag.

  python tools/tagmatch_probe.py --n 256e6 --tags 1e6 --len 32 --sample 2000 --write-fasta DIR

needs no device: it writes DIR/subject.fna and DIR/tags.fna (the first --sample
of the same tags) for `gt suffixerator -dna -suf -tis -ssp` and `gt tagerator -e
K -esa INDEX -q DIR/tags.fna` of the reference on one core of the CPU.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from genometools_amd import synth  # noqa: E402


def make_tags(a, n):
    """(symbols, offsets) on the CPU: the same for the device and for the files"""
    rng = np.random.default_rng(a.seed + 1)
    count, m = int(a.tags), a.len
    starts = rng.integers(0, n - m, count)
    tags = np.empty((count, m), dtype=np.uint8)
    # the subject is generated piece by piece: only the places of the tags are needed
    order = np.argsort(starts)
    piece = 1 << 24
    for lo in range(0, n, piece):
        hi = min(n, lo + piece + m)
        mine = order[(starts[order] >= lo) & (starts[order] < lo + piece)]
        if mine.size:
            part = synth.generate(a.model, a.seed, n, lo, hi)
            tags[mine] = part[(starts[mine] - lo)[:, None] + np.arange(m)[None, :]]
    special = tags >= 254
    tags[special] = rng.integers(0, 4, int(special.sum()), dtype=np.uint8)
    for _ in range(a.edits):
        at = rng.integers(0, m, count)
        what = rng.integers(0, 3, count)
        rows = np.arange(count)
        sub = what == 0
        tags[rows[sub], at[sub]] = (tags[rows[sub], at[sub]] + rng.integers(1, 4, int(sub.sum()), dtype=np.uint8)) % 4
        for r in rows[what == 1]:          # an insertion: the last letter falls off
            tags[r, at[r] + 1:] = tags[r, at[r]:-1]
            tags[r, at[r]] = rng.integers(0, 4)
        for r in rows[what == 2]:          # a deletion: a random letter joins at the end
            tags[r, at[r]:-1] = tags[r, at[r] + 1:]
            tags[r, -1] = rng.integers(0, 4)
    tags[1::2] = (3 - tags[1::2])[:, ::-1]
    return tags.reshape(-1).copy(), (np.arange(count + 1, dtype=np.uint64) * np.uint64(m))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=float, default=256e6)
    ap.add_argument("--model", type=int, default=synth.MODEL_HUMANLIKE_DNA)
    ap.add_argument("--seed", type=int, default=43)
    ap.add_argument("--tags", type=float, default=1e6)
    ap.add_argument("--len", type=int, default=32)
    ap.add_argument("--edits", type=int, default=1)
    ap.add_argument("-e", type=int, nargs="+", default=[0, 1, 2])
    ap.add_argument("--capacity", type=float, default=1 << 22)
    ap.add_argument("--sample", type=float, default=2000)
    ap.add_argument("--write-fasta", metavar="DIR")
    a = ap.parse_args()
    n = int(a.n)
    symbols, offsets = make_tags(a, n)
    count = offsets.size - 1
    if a.write_fasta:
        os.makedirs(a.write_fasta, exist_ok=True)
        synth.write_fasta(os.path.join(a.write_fasta, "subject.fna"), synth.generate(a.model, a.seed, n))
        with open(os.path.join(a.write_fasta, "tags.fna"), "w") as f:
            for t in range(min(count, int(a.sample))):
                f.write(">\n%s\n" % "".join("acgt"[c] for c in symbols[t * a.len:(t + 1) * a.len]))
        print("model %d seed %d n %d, %d of %d tags of %d letters: written to %s" % (
            a.model, a.seed, n, min(count, int(a.sample)), count, a.len, a.write_fasta))
        return 0

    import torch
    from genometools_amd import _lib, esa, tagmatch
    lib = _lib.load()
    subject = torch.empty(n, dtype=torch.uint8, device="cuda:0")
    _lib.check(lib.gtamd_synth_bytes(0, a.model, a.seed, n, subject.data_ptr()))
    d_symbols = torch.from_numpy(symbols).to("cuda:0")
    d_offsets = torch.from_numpy(offsets.view(np.int64)).to("cuda:0")
    torch.cuda.synchronize()
    with esa.EsaEngine(n, 4) as eng, tagmatch.TagMatches() as tm:
        eng.set_sequence_device(subject.data_ptr(), n)
        eng.run(esa.WANT_SUF)
        print("model %d seed %d n %d: built in %.1f ms (engine total_ms); %d tags of %d letters, %d edits each" % (
            a.model, a.seed, n, eng.timing()["total_ms"], count, a.len, a.edits), flush=True)
        tm.set_index_engine(eng, subject.data_ptr(), n)
        for K in a.e:
            for attempt in ("first call", "second call"):
                t0 = time.time()
                tm.prepare_device(d_symbols.data_ptr(), d_offsets.data_ptr(), count, K)
                t1 = time.time()
                calls = records = 0
                for chunk in tm.records(int(a.capacity), device=True):
                    calls += 1
                    records += chunk.shape[0]
                torch.cuda.synchronize()
                t2 = time.time()
                info = tm.info()
                assert records == info["matches"]
                wall = max(t2 - t0, 1e-9)
                print("K=%d %-11s count %9.2f ms on the device (%.2f ms wall), emit %.2f ms wall in %d calls of at "
                      "most %d records: %.3g tags/s, %.1f children examined per tag, %.2f matches per tag; %s" % (
                          K, attempt, info["device_ms"], 1e3 * (t1 - t0), 1e3 * (t2 - t1), calls, int(a.capacity),
                          count / wall, info["children_examined"] / max(count, 1), records / max(count, 1), info),
                      flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
