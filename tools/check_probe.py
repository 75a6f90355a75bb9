#!/usr/bin/env python3
"""Time the index checker (include/gtamd_check.h) on the resident tables of one
full-size build, beside the torch restatement of the same checks
(tests/device_check.py) in the same process and the engine's build time:

  timeout -k 10 900 python tools/check_probe.py --n 3e9 --model 1 --seed 43
  timeout -k 10 900 python tools/check_probe.py --n 1e9 --model 2 --seed 43    (protein)

One build and one check of each kind per invocation.  Both checkers must accept
the tables; the bytes each phase of the HIP checker has to move are printed
beside its time (counted from the sizes, not measured).
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import device_check as dc  # noqa: E402
from genometools_amd import _lib, check, esa, synth  # noqa: E402

PHASES = ("suf: range and permutation", "suf: order", "bwt", "lcp/llv: structure", "lcp/llv: values")


def phase_bytes(N, m):
    """what each phase reads and writes at least, per table entry: streamed
    bytes, and gathers (an access of 1 to 8 bytes at an address that depends
    on a table, each costing a memory transaction of its own)"""
    return (
        # memset 4, suf 8, rank scatter 4 | rank 4, suf gather 8
        ((4 + 8 + 4) * N, 2 * N),
        # suf 8 (twice, neighbours share), 2 symbols and 2 ranks gathered
        (8 * N, 4 * N),
        # suf 8, bwt 1, one symbol gathered
        (9 * N, N),
        # lcp 1, the pairs 16 with one byte gathered each
        (N + 16 * m, m),
        # rank 4; gathered: lcp byte, suf entry, two symbols of (a), the symbols of (b)
        (4 * N, 4 * N),
    )


def torch_checks(sa, enc, lcp, bwt, llv_idx, llv_val):
    """the same criteria with tests/device_check.py; seconds per check"""
    out = []

    def timed(name, fn):
        torch.cuda.synchronize()
        t0 = time.time()
        ok, msg = fn()
        torch.cuda.synchronize()
        out.append((name, time.time() - t0))
        assert ok, (name, msg)
    rank = [None]

    def ranks():
        rank[0], msg = dc.suffix_ranks(sa)
        return rank[0] is not None, msg
    timed("suf: range and permutation", ranks)
    timed("suf: order", lambda: dc.check_suffix_array_exact(sa, enc, rank[0]))
    timed("bwt", lambda: dc.check_bwt_exact(sa, enc, bwt))
    timed("lcp/llv: structure and values", lambda: dc.check_lcp_exact(sa, enc, lcp, llv_idx, llv_val, rank[0]))
    peak = torch.cuda.max_memory_allocated()
    del rank
    torch.cuda.empty_cache()
    return out, peak


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=float, default=3e9)
    ap.add_argument("--model", type=int, default=synth.MODEL_HUMANLIKE_DNA)
    ap.add_argument("--seed", type=int, default=43)
    a = ap.parse_args()
    n = int(a.n)
    N = n + 1
    lib = _lib.load()
    buf = torch.empty(n, dtype=torch.uint8, device="cuda:0")
    _lib.check(lib.gtamd_synth_bytes(0, a.model, a.seed, n, buf.data_ptr()))
    torch.cuda.synchronize()
    want = esa.WANT_SUF | esa.WANT_LCP | esa.WANT_BWT
    with esa.EsaEngine(n, synth.numofchars(a.model)) as eng, check.EsaChecker() as chk:
        eng.set_sequence_device(buf.data_ptr(), n)
        eng.run(want)
        st, tm = eng.stats(), eng.timing()
        m = eng.entries(esa.TAB_LLV)
        print("model %d seed %d n %d: built in %.1f ms (engine total_ms); %d .llv entries, largest value %d" % (
            a.model, a.seed, n, tm["total_ms"], m, st["maxbranchdepth"]), flush=True)
        free0 = torch.cuda.mem_get_info()[0]
        t0 = time.time()
        res = chk.check_engine(eng, buf.data_ptr(), n, want)
        wall = time.time() - t0
        extra = free0 - torch.cuda.mem_get_info()[0]
        assert res.ok, res
        assert (res.longest, res.largelcpvalues, res.maxbranchdepth) == \
            (st["longest"], st["largelcpvalues"], st["maxbranchdepth"]), (res, st)
        print("HIP checker: accepted; %.1f ms on the device (%.1f ms wall, first call, with its allocations)" % (
            res.check_ms, 1e3 * wall))
        for name, ms, (streamed, gathers) in zip(PHASES, res.phase_ms, phase_bytes(N, m)):
            print("  %-28s %9.1f ms   %7.1f GB streamed (%5.2f TB/s), %5.1f G gathers (%5.1f G/s)" % (
                name, ms, streamed / 1e9, streamed / ms / 1e9, gathers / 1e9, gathers / ms / 1e6))
        print("  positions on the work list: %d; device memory taken by the checker: %.2f GB (inverse %.2f GB)" % (
            res.long_claims, extra / 1e9, 4 * N / 1e9), flush=True)
        # once more, with everything allocated and the code loaded
        res2 = chk.check_engine(eng, buf.data_ptr(), n, want)
        assert res2.ok
        print("HIP checker, second call: %.1f ms on the device (%s)" % (
            res2.check_ms, ", ".join("%.1f" % t for t in res2.phase_ms)), flush=True)
        sa = dc.as_tensor(eng.device_pointer(esa.TAB_SUF), N, "<i8")
        lcp = dc.as_tensor(eng.device_pointer(esa.TAB_LCP), N, "|u1")
        bwt = dc.as_tensor(eng.device_pointer(esa.TAB_BWT), N, "|u1")
        llv = (dc.as_tensor(eng.device_pointer(esa.TAB_LLV), 2 * m, "<i8") if m else
               torch.empty(0, dtype=torch.int64, device="cuda:0")).view(-1, 2)
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        times, peak = torch_checks(sa, buf, lcp, bwt, llv[:, 0].contiguous(), llv[:, 1].contiguous())
        total = sum(t for _, t in times)
        print("torch checker (tests/device_check.py): accepted; %.1f ms, peak extra device memory %.2f GB" % (
            1e3 * total, (peak - base) / 1e9))
        for name, t in times:
            print("  %-28s %9.1f ms" % (name, 1e3 * t))
        print("summary: build %.1f ms, HIP check %.1f ms, torch check %.1f ms (%.1fx)" % (
            tm["total_ms"], res.check_ms, 1e3 * total, 1e3 * total / res.check_ms))
    return 0


if __name__ == "__main__":
    sys.exit(main())
