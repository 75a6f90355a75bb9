#!/usr/bin/env python3
"""Time matching statistics and minimum unique prefixes (include/gtamd_mstat.h)
against the resident suffix table of one build:

  timeout -k 10 900 python tools/mstat_probe.py --n 256e6 --model 0 --m 1e7 --kind sampled --rate 0.01
  timeout -k 10 900 python tools/mstat_probe.py --n 3e9 --model 1 --m 1e7 --kind sampled --rate 0.01
  timeout -k 10 900 python tools/mstat_probe.py --n 1e8 --model 1 --m 1e7 --kind copy --max-len 20

The kinds of query: `random` (letters of the alphabet, uniform), `sampled` (pieces
of --piece symbols taken from the subject, every symbol replaced by another letter
with probability --rate, a separator between two pieces) and `copy` (the first
--m symbols of the subject, verbatim: give --max-len).  One build, then matstat
and uniquesub twice each; positions per second from the device time of the second
call, and the info struct of each.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from genometools_amd import _lib, esa, mstat, synth  # noqa: E402


def make_query(a, subject, sigma):
    """uint8 tensor on the device"""
    g = torch.Generator(device="cuda:0")
    g.manual_seed(a.seed + 1)
    m, n = int(a.m), subject.numel()
    if a.kind == "random":
        return torch.randint(0, sigma, (m,), dtype=torch.uint8, device="cuda:0", generator=g)
    if a.kind == "copy":
        return subject[:min(m, n)].clone()
    piece = a.piece
    pieces = max(1, m // (piece + 1))
    starts = torch.randint(0, n - piece, (pieces,), device="cuda:0", generator=g)
    q = subject[(starts[:, None] + torch.arange(piece, device="cuda:0")[None, :])]
    letter = q < 254
    hit = (torch.rand(q.shape, device="cuda:0", generator=g) < a.rate) & letter
    shift = torch.randint(1, sigma, q.shape, dtype=torch.uint8, device="cuda:0", generator=g)
    q = torch.where(hit, (q + shift) % sigma, q)
    sep = torch.full((pieces, 1), 255, dtype=torch.uint8, device="cuda:0")
    return torch.cat([q, sep], dim=1).reshape(-1)[:-1].contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=float, default=256e6)
    ap.add_argument("--model", type=int, default=synth.MODEL_HUMANLIKE_DNA)
    ap.add_argument("--seed", type=int, default=43)
    ap.add_argument("--m", type=float, default=1e7)
    ap.add_argument("--kind", choices=("random", "sampled", "copy"), default="sampled")
    ap.add_argument("--rate", type=float, default=0.01)
    ap.add_argument("--piece", type=int, default=1000)
    ap.add_argument("--max-len", type=int, default=0)
    a = ap.parse_args()
    n, sigma = int(a.n), synth.numofchars(a.model)
    lib = _lib.load()
    subject = torch.empty(n, dtype=torch.uint8, device="cuda:0")
    _lib.check(lib.gtamd_synth_bytes(0, a.model, a.seed, n, subject.data_ptr()))
    torch.cuda.synchronize()
    query = make_query(a, subject, sigma)
    m = query.numel()
    length = torch.empty(m, dtype=torch.int32, device="cuda:0")
    pos = torch.empty(m, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    with esa.EsaEngine(n, sigma) as eng, mstat.MatchStats() as ms:
        eng.set_sequence_device(subject.data_ptr(), n)
        eng.run(esa.WANT_SUF)
        print("model %d seed %d n %d: built in %.1f ms (engine total_ms); query: %s, %d symbols, max_len %d" % (
            a.model, a.seed, n, eng.timing()["total_ms"], a.kind, m, a.max_len), flush=True)
        ms.set_index_engine(eng, subject.data_ptr(), n)
        for name, call in (
                ("matstat", lambda: ms.matstat_device(query.data_ptr(), m, length.data_ptr(), pos.data_ptr(),
                                                      a.max_len)),
                ("matstat, no witness", lambda: ms.matstat_device(query.data_ptr(), m, length.data_ptr(), None,
                                                                  a.max_len)),
                ("uniquesub", lambda: ms.uniquesub_device(query.data_ptr(), m, length.data_ptr(), a.max_len))):
            for attempt in ("first call", "second call"):
                t0 = time.time()
                call()
                wall = time.time() - t0
                info = ms.info()
                print("%-20s %-11s %9.2f ms on the device (%.2f ms wall): %.3g positions/s; %s" % (
                    name, attempt, info["device_ms"], 1e3 * wall, m / info["device_ms"] * 1e3, info), flush=True)
            hist = torch.bincount(length.clamp(max=63).to(torch.int64), minlength=64).tolist()
            print("  lengths: mean %.2f, largest %d, zero at %d positions; 0..31: %s" % (
                length.double().mean().item(), int(length.max()), hist[0], hist[:32]), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
