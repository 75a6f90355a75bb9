#!/usr/bin/env python3
"""Time the reader of the packed index (include/gtamd_pckidx.h): the decode of
an image, and matstat / uniquesub through it beside the same queries through the
suffix table of the same text (include/gtamd_mstat.h):

  timeout -k 10 900 python tools/pckmstat_probe.py --n 256e6 --m 1e7 --json pckmstat_256m.json
  timeout -k 10 900 python tools/pckmstat_probe.py --n 3e9 --m 1e7 --json pckmstat_3g.json

The packed index is the one of the reference's index searches (-sprank -bsize 10
-locfreq 32 -dir rev, mkindex flavour) unless --defaults; the queries are pieces
of --piece symbols cut from the text, every symbol replaced by another letter
with probability --rate, a separator between two pieces.  Every call twice;
positions per second from the device time of the second call.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from genometools_amd import _lib, esa, mstat, pck, synth  # noqa: E402
from tools.mstat_probe import make_query  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=float, default=256e6)
    ap.add_argument("--model", type=int, default=synth.MODEL_HUMANLIKE_DNA)
    ap.add_argument("--seed", type=int, default=43)
    ap.add_argument("--m", type=float, default=1e7)
    ap.add_argument("--rate", type=float, default=0.01)
    ap.add_argument("--piece", type=int, default=1000)
    ap.add_argument("--defaults", action="store_true", help="the default options of gt packedindex")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    a.kind = "sampled"
    n, sigma = int(a.n), synth.numofchars(a.model)
    kw = dict() if a.defaults else dict(bsize=10, blbuck=8, locfreq=32, sprank=True, mkindex=True)
    lib = _lib.load()
    subject = torch.empty(n, dtype=torch.uint8, device="cuda:0")
    _lib.check(lib.gtamd_synth_bytes(0, a.model, a.seed, n, subject.data_ptr()))
    torch.cuda.synchronize()
    query = make_query(a, subject, sigma)
    m = query.numel()
    length = torch.empty(m, dtype=torch.int32, device="cuda:0")
    other = torch.empty(m, dtype=torch.int32, device="cuda:0")
    pos = torch.empty(m, dtype=torch.int64, device="cuda:0")
    res = {"gpu": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName, "n": n, "model": a.model, "m": m, "rate": a.rate, "options": kw}

    def timed(ms, what):
        calls = (("matstat", lambda o: ms.matstat_device(query.data_ptr(), m, o.data_ptr(), pos.data_ptr())),
                 ("matstat, no witness", lambda o: ms.matstat_device(query.data_ptr(), m, o.data_ptr())),
                 ("uniquesub", lambda o: ms.uniquesub_device(query.data_ptr(), m, o.data_ptr())))
        out = {}
        for name, call in calls:
            for _ in range(2):
                call(length if what == "pck" else other)
            info = ms.info()
            out[name] = {"device_ms": info["device_ms"], "positions_per_s": m / info["device_ms"] * 1e3,
                         "symbols_compared": info["symbols_compared"]}
            print("%-4s %-20s %9.2f ms: %.3g positions/s" % (what, name, info["device_ms"],
                                                            out[name]["positions_per_s"]), flush=True)
            if name == "matstat, no witness":
                out["lengths"] = (length if what == "pck" else other).clone()
        return out

    with esa.EsaEngine(n, sigma) as eng, pck.PackedIndex() as builder, pck.PackedIndexReader() as reader, \
            mstat.MatchStats() as ms:
        eng.set_readmode(1)
        eng.set_sequence_device(subject.data_ptr(), n)
        eng.run(esa.WANT_SUF | esa.WANT_BWT)
        builder.build_from_esa(eng, **kw)
        res["image"] = builder.info()
        for _ in range(2):
            reader.open_builder(builder)
        res["reader"] = info = reader.info()
        print("%s (%s): n %d, image %.3f GB built in %.1f ms, decoded in %.1f ms into %.3f GB (%.2f bits a row), %d marks"
              % (res["gpu"], res["arch"], n, info["image_bytes"] / 1e9, res["image"]["build_ms"], info["decode_ms"],
                 info["decoded_bytes"] / 1e9, 8.0 * info["decoded_bytes"] / info["rows"], info["marks"]), flush=True)
        ms.set_index_packed(reader)
        res["pck"] = timed(ms, "pck")
        eng.set_readmode(0)
        eng.set_sequence_device(subject.data_ptr(), n)
        eng.run(esa.WANT_SUF)
        ms.set_index_engine(eng, subject.data_ptr(), n)
        res["esa"] = timed(ms, "esa")
    same = bool(torch.equal(res["pck"].pop("lengths"), res["esa"].pop("lengths")))
    res["lengths_equal"] = same
    for name in ("matstat", "matstat, no witness", "uniquesub"):
        r = res["esa"][name]["device_ms"] / res["pck"][name]["device_ms"]
        print("%-20s -pck takes %.2f times the time of -esa" % (name, 1 / r), flush=True)
    print("lengths through -pck and -esa equal: %s" % same, flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
            f.write("\n")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
