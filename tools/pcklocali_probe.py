#!/usr/bin/env python3
"""Time the local alignments of queries through the packed index
(include/gtamd_pcklocali.h) beside the same calls on the resident suffix table
(include/gtamd_locali.h), in one run:

  python tools/pcklocali_probe.py --n 2e6 16e6 --queries 8 --len 100 300 1000 --th 20 30

The text, the queries and the scores are those of tools/locali_probe.py.  Every
size is a process of its own under --limit seconds (`--one N` is that process).
Per size: one build in forward read mode with .suf, one in reverse read mode
with .suf and the BWT, from which the packed index is built and opened by a
reader (the decode time is the reader's).  Then per length and threshold, on
both paths: prepare (the count pass and the offsets; device time) and the emit
calls into one device buffer of --capacity records (wall).  The record counts of
the two paths must be equal.  Printed: decode, count and emit time of both, the
jobs, jobs_finished_alone, and the time of the count pass per child.
"""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import locali_probe  # noqa: E402
from genometools_amd import synth  # noqa: E402


def timed(lc, queries, T, scores, capacity):
    """(info, wall ms of prepare, wall ms of emit) of one call"""
    import torch
    t0 = time.time()
    lc.prepare(queries, T, *scores)
    t1 = time.time()
    records = 0
    for chunk in lc.records(capacity, device=True):
        records += chunk.shape[0]
    torch.cuda.synchronize()
    t2 = time.time()
    info = lc.info()
    assert records == info["matches"]
    return info, 1e3 * (t1 - t0), 1e3 * (t2 - t1)


def one(a, n):
    import torch
    from genometools_amd import _lib, esa, locali, pck
    lib = _lib.load()
    subject = torch.empty(n, dtype=torch.uint8, device="cuda:0")
    _lib.check(lib.gtamd_synth_bytes(0, a.model, a.seed, n, subject.data_ptr()))
    torch.cuda.synchronize()
    with esa.EsaEngine(n, 4) as eng, esa.EsaEngine(n, 4) as rev, locali.LocalAlignments() as plain, \
            locali.LocalAlignments() as packed, pck.PackedIndex() as builder, pck.PackedIndexReader() as reader:
        eng.set_sequence_device(subject.data_ptr(), n)
        eng.run(esa.WANT_SUF)
        plain.set_index_engine(eng, subject.data_ptr(), n)
        rev.set_readmode(1)
        rev.set_sequence_device(subject.data_ptr(), n)
        rev.run(esa.WANT_SUF | esa.WANT_BWT)
        builder.build_from_esa(rev, bsize=10, blbuck=8, locfreq=32, sprank=True)
        t0 = time.time()
        reader.open_builder(builder)
        torch.cuda.synchronize()
        packed.set_index_packed(reader)
        print("model %d seed %d n %d: reader opened (decode) in %.1f ms wall, %s; scores %s" % (
            a.model, a.seed, n, 1e3 * (time.time() - t0), reader.info(), a.scores), flush=True)
        for m in a.len:
            queries = locali_probe.make_queries(a, n, m)
            for T in a.th:
                timed(packed, queries, T, a.scores, int(a.capacity))          # (a first call: allocations)
                row = []
                for name, lc in (("esa", plain), ("pck", packed)):
                    info, prepare_ms, emit_ms = timed(lc, queries, T, a.scores, int(a.capacity))
                    row.append((name, info, prepare_ms, emit_ms))
                assert row[0][1]["matches"] == row[1][1]["matches"], (row[0][1]["matches"], row[1][1]["matches"])
                for name, info, prepare_ms, emit_ms in row:
                    print("n=%d m=%d T=%d %s: count %9.2f ms on the device (%.2f ms wall), emit %9.2f ms wall, %d matches, "
                          "%d jobs (q=%d), %d finished alone, %d levels, %d children, %d single walks, %.2f ns of the "
                          "count pass per child" % (n, m, T, name, info["device_ms"], prepare_ms, emit_ms,
                                                    info["matches"], info["jobs"], info["cut_depth"],
                                                    info["jobs_finished_alone"], info["levels_pushed"],
                                                    info["children_examined"], info["single_walks"],
                                                    1e6 * info["device_ms"] / max(info["children_examined"], 1)), flush=True)
                print("n=%d m=%d T=%d esa / pck: count %.2f, emit %.2f" % (
                    n, m, T, row[0][1]["device_ms"] / max(row[1][1]["device_ms"], 1e-9), row[0][3] / max(row[1][3], 1e-9)),
                    flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=float, nargs="+", default=[2e6, 16e6])
    ap.add_argument("--model", type=int, default=synth.MODEL_HUMANLIKE_DNA)
    ap.add_argument("--seed", type=int, default=43)
    ap.add_argument("--queries", type=int, default=8)
    ap.add_argument("--len", type=int, nargs="+", default=[100, 300, 1000])
    ap.add_argument("--edits", type=int, default=4)
    ap.add_argument("--th", type=int, nargs="+", default=[20, 30])
    ap.add_argument("--scores", type=int, nargs=3, default=[1, -3, -2], metavar=("MATCH", "MISMATCH", "GAPEXTEND"))
    ap.add_argument("--capacity", type=float, default=1 << 22)
    ap.add_argument("--limit", type=int, default=240, help="seconds one size may take")
    ap.add_argument("--one", type=float, help="run this size in this process")
    a = ap.parse_args()
    if a.one is not None:
        return one(a, int(a.one))
    for n in a.n:
        # a fresh child process per size, under its own time limit; the first that fails ends the run
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--one", repr(n)] + sys.argv[1:]
        run = subprocess.run(cmd)
        if run.returncode != 0:
            print("n=%d: the process ended with %d; nothing more is started" % (int(n), run.returncode), flush=True)
            return run.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
