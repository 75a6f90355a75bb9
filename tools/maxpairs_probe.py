#!/usr/bin/env python3
"""Time the enumeration of maximal pairs (include/gtamd_maxpairs.h) on the
resident tables of one build:

  timeout -k 10 900 python tools/maxpairs_probe.py --n 256e6 --model 0 --plant 20000 --plant-len 500 -l 20
  timeout -k 10 900 python tools/maxpairs_probe.py --n 256e6 --model 3 -l 30

--plant copies that many pieces of --plant-len symbols from one place of the
subject to another before the build (a uniform text has next to no repeat of 20
letters).  Model 3 is the repeat-heavy text with homopolymer and satellite
runs.  One build with .suf and .lcp, then prepare twice and the emit calls into
one device buffer of --capacity records; the info struct, the device time of
the prepare, and pairs per second over prepare + emit (wall).
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from genometools_amd import _lib, esa, maxpairs, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=float, default=256e6)
    ap.add_argument("--model", type=int, default=synth.MODEL_UNIFORM_DNA)
    ap.add_argument("--seed", type=int, default=43)
    ap.add_argument("-l", "--min-len", type=int, default=20)
    ap.add_argument("--plant", type=int, default=0)
    ap.add_argument("--plant-len", type=int, default=500)
    ap.add_argument("--capacity", type=float, default=1 << 24)
    a = ap.parse_args()
    n, sigma = int(a.n), synth.numofchars(a.model)
    lib = _lib.load()
    subject = torch.empty(n, dtype=torch.uint8, device="cuda:0")
    _lib.check(lib.gtamd_synth_bytes(0, a.model, a.seed, n, subject.data_ptr()))
    if a.plant:
        g = torch.Generator(device="cuda:0")
        g.manual_seed(a.seed + 1)
        src = torch.randint(0, n - a.plant_len, (a.plant,), device="cuda:0", generator=g)
        dst = torch.randint(0, n - a.plant_len, (a.plant,), device="cuda:0", generator=g)
        span = torch.arange(a.plant_len, device="cuda:0")[None, :]
        subject[(dst[:, None] + span).reshape(-1)] = subject[(src[:, None] + span).reshape(-1)]
    torch.cuda.synchronize()
    with esa.EsaEngine(n, sigma) as eng, maxpairs.MaxPairs() as mp:
        eng.set_sequence_device(subject.data_ptr(), n)
        eng.run(esa.WANT_SUF | esa.WANT_LCP)
        print("model %d seed %d n %d, %d planted copies of %d: built in %.1f ms (engine total_ms); min_len %d" % (
            a.model, a.seed, n, a.plant, a.plant_len, eng.timing()["total_ms"], a.min_len), flush=True)
        mp.set_index_engine(eng, subject.data_ptr(), n)
        for attempt in ("first call", "second call"):
            t0 = time.time()
            info = mp.prepare(a.min_len)
            t1 = time.time()
            capacity = max(int(a.capacity), info["max_pairs_of_one_suffix"])
            chunks = records = 0
            longest = 0
            for chunk in mp.pairs(capacity, device=True):
                chunks += 1
                records += chunk.shape[0]
                longest = max(longest, int(chunk[:, 2].max()))
            torch.cuda.synchronize()
            t2 = time.time()
            assert records == info["pairs"] and longest == info["max_len"]
            print("%-11s prepare %9.2f ms on the device (%.2f ms wall), emit %.2f ms wall in %d chunks of at most "
                  "%d: %.3g pairs/s; %.2f steps per pair; %s" % (
                      attempt, info["device_ms"], 1e3 * (t1 - t0), 1e3 * (t2 - t1), chunks, capacity,
                      records / max(t2 - t0, 1e-9), info["walk_steps"] / max(records, 1), info), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
