#!/usr/bin/env python3
"""Time the approximate matches of short tags through the packed index
(include/gtamd_pcktag.h) beside the same tags through the suffix table
(include/gtamd_tagmatch.h), in one run:

  timeout -k 10 300 python tools/pcktag_probe.py --n 16e6 --tags 1e5 -e 1

The subject, the tags (--len letters cut from the subject, --edits random
differences each, every second one reverse-complemented) are those of
tools/tagmatch_probe.py.  One build of the reversed subject with .suf and .bwt,
from it the packed index (-sprank -bsize 10, --locfreq 32) and its reader; one
build of the subject with .suf.  Then per K and per path, twice: prepare (the
count passes and the offsets) and the emit calls into one device buffer of
--capacity records.  Printed per call: the device time of the count, the wall
time of the emit calls, tags per second over both, children examined per tag,
and, after both paths, whether their record counts and K' are equal.  --only pck
leaves the suffix table out (to compare locate intervals)."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from genometools_amd import synth  # noqa: E402
from tagmatch_probe import make_tags  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=float, default=16e6)
    ap.add_argument("--model", type=int, default=synth.MODEL_HUMANLIKE_DNA)
    ap.add_argument("--seed", type=int, default=43)
    ap.add_argument("--tags", type=float, default=1e5)
    ap.add_argument("--len", type=int, default=32)
    ap.add_argument("--edits", type=int, default=1)
    ap.add_argument("-e", type=int, nargs="+", default=[0, 1])
    ap.add_argument("--capacity", type=float, default=1 << 22)
    ap.add_argument("--locfreq", type=int, default=32)
    ap.add_argument("--only", choices=["pck", "esa"])
    a = ap.parse_args()
    n = int(a.n)
    symbols, offsets = make_tags(a, n)
    count = offsets.size - 1

    import torch
    from genometools_amd import _lib, esa, pck, tagmatch
    lib = _lib.load()
    subject = torch.empty(n, dtype=torch.uint8, device="cuda:0")
    _lib.check(lib.gtamd_synth_bytes(0, a.model, a.seed, n, subject.data_ptr()))
    d_symbols = torch.from_numpy(symbols).to("cuda:0")
    d_offsets = torch.from_numpy(offsets.view(np.int64)).to("cuda:0")
    torch.cuda.synchronize()
    print("model %d seed %d n %d; %d tags of %d letters, %d edits each" % (a.model, a.seed, n, count, a.len, a.edits),
          flush=True)
    with esa.EsaEngine(n, 4) as eng, pck.PackedIndex() as builder, pck.PackedIndexReader() as reader, \
            tagmatch.TagMatches() as tm:
        paths = []
        if a.only != "esa":
            eng.set_readmode(1)
            eng.set_sequence_device(subject.data_ptr(), n)
            eng.run(esa.WANT_SUF | esa.WANT_BWT)
            builder.build_from_esa(eng, bsize=10, blbuck=8, locfreq=a.locfreq, sprank=True, mkindex=True)
            reader.open_builder(builder)
            info = reader.info()
            print("packed index -sprank -bsize 10 -locfreq %d: image %.3f GB, decoded form %.3f GB in %.1f ms" % (
                a.locfreq, info["image_bytes"] / 1e9, info["decoded_bytes"] / 1e9, info["decode_ms"]), flush=True)
            paths.append("pck")
        if a.only != "pck":
            paths.append("esa")
        seen = {}
        for path in paths:
            if path == "pck":
                tm.set_index_packed(reader)
            else:
                eng.set_readmode(0)
                eng.set_sequence_device(subject.data_ptr(), n)
                eng.run(esa.WANT_SUF)
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
                    print("%s K=%d %-11s count %9.2f ms on the device (%.2f ms wall), emit %.2f ms wall in %d calls: "
                          "%.3g tags/s, %.1f children examined per tag, %.2f matches per tag; %s" % (
                              path, K, attempt, info["device_ms"], 1e3 * (t1 - t0), 1e3 * (t2 - t1), calls,
                              count / wall, info["children_examined"] / max(count, 1), records / max(count, 1), info),
                          flush=True)
                seen[path, K] = (records, tm.best_k())
        for K in a.e:
            if ("pck", K) in seen and ("esa", K) in seen:
                same = seen["pck", K][0] == seen["esa", K][0] and np.array_equal(seen["pck", K][1], seen["esa", K][1])
                print("K=%d: records and K' through -pck and -esa equal: %s (%d records)" % (K, same, seen["pck", K][0]),
                      flush=True)
                if not same:
                    return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
