#!/usr/bin/env python3
"""Time the local alignments of queries (include/gtamd_locali.h) against the
resident suffix table of one build:

  timeout -k 10 900 python tools/locali_probe.py --n 16e6 --queries 8 --len 100 300 1000 --th 20 30

The queries are --len letters cut from random places of the subject (a
wildcard inside becomes a letter), every one with a replacement, insertion or
deletion at --edits random places.  One build with .suf, then per length and
threshold: prepare (the count pass and the offsets) and the emit calls into one
device buffer of --capacity records; the info struct, the device time of the
prepare, queries and alignments per second over prepare + emit (wall).

  python tools/locali_probe.py --n 16e6 --queries 8 --len 100 --write-fasta DIR

needs no device: it writes DIR/subject.fna and DIR/queries_LEN.fna for `gt
suffixerator -dna -suf -tis -ssp` and `gt dev idxlocali -th T -esa INDEX -q
DIR/queries_LEN.fna` of the reference on one core of the CPU.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from genometools_amd import synth  # noqa: E402


def make_queries(a, n, m):
    """a list of encoded queries on the CPU: the same for the device and for the files"""
    rng = np.random.default_rng(a.seed + m)
    queries = []
    for _ in range(a.queries):
        at = int(rng.integers(0, n - m))
        q = synth.generate(a.model, a.seed, n, at, at + m).copy()
        special = q >= 254
        q[special] = rng.integers(0, 4, int(special.sum()), dtype=np.uint8)
        q = list(q)
        for _ in range(a.edits):
            where, what = int(rng.integers(len(q))), int(rng.integers(3))
            if what == 0:
                q[where] = (q[where] + 1 + int(rng.integers(3))) % 4
            elif what == 1:
                q.insert(where, int(rng.integers(4)))
            elif len(q) > 4:
                del q[where]
        queries.append(np.array(q[:m], dtype=np.uint8))
    return queries


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=float, default=16e6)
    ap.add_argument("--model", type=int, default=synth.MODEL_HUMANLIKE_DNA)
    ap.add_argument("--seed", type=int, default=43)
    ap.add_argument("--queries", type=int, default=8)
    ap.add_argument("--len", type=int, nargs="+", default=[100, 300, 1000])
    ap.add_argument("--edits", type=int, default=4)
    ap.add_argument("--th", type=int, nargs="+", default=[20, 30])
    ap.add_argument("--scores", type=int, nargs=3, default=[1, -3, -2], metavar=("MATCH", "MISMATCH", "GAPEXTEND"))
    ap.add_argument("--capacity", type=float, default=1 << 22)
    ap.add_argument("--write-fasta", metavar="DIR")
    a = ap.parse_args()
    n = int(a.n)
    if a.write_fasta:
        os.makedirs(a.write_fasta, exist_ok=True)
        synth.write_fasta(os.path.join(a.write_fasta, "subject.fna"), synth.generate(a.model, a.seed, n))
        for m in a.len:
            with open(os.path.join(a.write_fasta, "queries_%d.fna" % m), "w") as f:
                for q in make_queries(a, n, m):
                    f.write(">\n%s\n" % "".join("acgt"[c] for c in q))
        print("model %d seed %d n %d, %d queries of each of %s letters: written to %s" % (
            a.model, a.seed, n, a.queries, a.len, a.write_fasta))
        return 0

    import torch
    from genometools_amd import _lib, esa, locali
    lib = _lib.load()
    subject = torch.empty(n, dtype=torch.uint8, device="cuda:0")
    _lib.check(lib.gtamd_synth_bytes(0, a.model, a.seed, n, subject.data_ptr()))
    torch.cuda.synchronize()
    with esa.EsaEngine(n, 4) as eng, locali.LocalAlignments() as lc:
        eng.set_sequence_device(subject.data_ptr(), n)
        eng.run(esa.WANT_SUF)
        t0 = time.time()
        lc.set_index_engine(eng, subject.data_ptr(), n)
        print("model %d seed %d n %d: built in %.1f ms (engine total_ms), table cut into groups in %.1f ms; scores %s" % (
            a.model, a.seed, n, eng.timing()["total_ms"], 1e3 * (time.time() - t0), a.scores), flush=True)
        for m in a.len:
            queries = make_queries(a, n, m)
            for T in a.th:
                t0 = time.time()
                lc.prepare(queries, T, *a.scores)
                t1 = time.time()
                calls = records = 0
                for chunk in lc.records(int(a.capacity), device=True):
                    calls += 1
                    records += chunk.shape[0]
                torch.cuda.synchronize()
                t2 = time.time()
                info = lc.info()
                assert records == info["matches"]
                wall = max(t2 - t0, 1e-9)
                print("m=%d T=%d count %9.2f ms on the device (%.2f ms wall), emit %.2f ms wall in %d calls: %.3g "
                      "queries/s, %.3g alignments/s, %.1f alignments per query; %s" % (
                          m, T, info["device_ms"], 1e3 * (t1 - t0), 1e3 * (t2 - t1), calls, len(queries) / wall,
                          records / wall, records / max(len(queries), 1), info), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
