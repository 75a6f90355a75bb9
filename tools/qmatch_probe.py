#!/usr/bin/env python3
"""Time the maximal exact matches of a query (include/gtamd_qmatch.h) against the
resident suffix table of one build:

  timeout -k 10 600 python tools/qmatch_probe.py --n 16e6 --model 1 --query cut -l 20
  timeout -k 10 600 python tools/qmatch_probe.py --n 16e6 --model 3 --query uniform -l 20

--query cut takes --m symbols from the middle of the subject and substitutes
every hundredth letter (--subst 0.01) by another one; --query uniform is an
unrelated uniform text.  One build with .suf, then prepare and the emit calls
into one device buffer of --capacity records, twice; the info struct, the
device time of the prepare, and positions, candidates and records per second
over prepare + emit (wall).

  python tools/qmatch_probe.py --n 16e6 --model 1 --query cut --write-fasta DIR

needs no device: it writes DIR/subject.fna and DIR/query.fna, the same symbols,
for `gt suffixerator -dna -suf -tis -ssp` and `gt repfind -l 20 -ii INDEX -q
DIR/query.fna` of the reference on the CPU.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from genometools_amd import synth  # noqa: E402


def make_query(a, n):
    """the encoded query, on the CPU: the same for the device and for the files"""
    m = int(a.m)
    if a.query == "uniform":
        return synth.generate(synth.MODEL_UNIFORM_DNA, a.seed + 7, m)
    start = (n - m) // 2
    query = synth.generate(a.model, a.seed, n, start, start + m).copy()
    rng = np.random.default_rng(a.seed + 1)
    at = rng.choice(m, int(m * a.subst), replace=False)
    at = at[query[at] < 254]
    query[at] = (query[at] + rng.integers(1, 4, at.size, dtype=np.uint8)) % 4
    return query


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=float, default=16e6)
    ap.add_argument("--model", type=int, default=synth.MODEL_HUMANLIKE_DNA)
    ap.add_argument("--seed", type=int, default=43)
    ap.add_argument("--query", choices=("cut", "uniform"), default="cut")
    ap.add_argument("--m", type=float, default=1e6)
    ap.add_argument("--subst", type=float, default=0.01)
    ap.add_argument("-l", "--min-len", type=int, default=20)
    ap.add_argument("--capacity", type=float, default=1 << 22)
    ap.add_argument("--write-fasta", metavar="DIR")
    a = ap.parse_args()
    n = int(a.n)
    query = make_query(a, n)
    if a.write_fasta:
        os.makedirs(a.write_fasta, exist_ok=True)
        synth.write_fasta(os.path.join(a.write_fasta, "subject.fna"), synth.generate(a.model, a.seed, n))
        synth.write_fasta(os.path.join(a.write_fasta, "query.fna"), query)
        print("model %d seed %d n %d, query %s of %d symbols: written to %s" % (
            a.model, a.seed, n, a.query, query.size, a.write_fasta))
        return 0

    import torch
    from genometools_amd import _lib, esa, qmatch
    lib = _lib.load()
    subject = torch.empty(n, dtype=torch.uint8, device="cuda:0")
    _lib.check(lib.gtamd_synth_bytes(0, a.model, a.seed, n, subject.data_ptr()))
    d_query = torch.from_numpy(query).to("cuda:0")
    torch.cuda.synchronize()
    with esa.EsaEngine(n, 4) as eng, qmatch.QueryMatches() as qm:
        eng.set_sequence_device(subject.data_ptr(), n)
        eng.run(esa.WANT_SUF)
        print("model %d seed %d n %d: built in %.1f ms (engine total_ms); query %s of %d symbols, min_len %d" % (
            a.model, a.seed, n, eng.timing()["total_ms"], a.query, query.size, a.min_len), flush=True)
        qm.set_index_engine(eng, subject.data_ptr(), n)
        for attempt in ("first call", "second call"):
            t0 = time.time()
            info = qm.prepare_device(d_query.data_ptr(), query.size, a.min_len)
            t1 = time.time()
            calls = records = longest = 0
            for chunk in qm.emit(int(a.capacity), device=True):
                calls += 1
                records += chunk.shape[0]
                longest = max(longest, int(chunk[:, 2].max()))
            torch.cuda.synchronize()
            t2 = time.time()
            info = qm.info()
            assert records == info["matches"]
            wall = max(t2 - t0, 1e-9)
            print("%-11s prepare %9.2f ms on the device (%.2f ms wall), emit %.2f ms wall in %d calls of at most %d "
                  "records: %.3g positions/s, %.3g candidates/s, %.3g records/s; longest %d; %s" % (
                      attempt, info["device_ms"], 1e3 * (t1 - t0), 1e3 * (t2 - t1), calls, int(a.capacity),
                      info["positions"] / wall, info["candidates"] / wall, records / wall, longest, info),
                  flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
