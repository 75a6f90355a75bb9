#!/usr/bin/env python3
"""Differential fuzzing on the GPU box: random structured sequences (repeats,
tandem repeats, special runs, separators; DNA and protein) through
  * the engine (all tables + bucket table, random prefix length),
  * the same build through the MSD first sort (forced; DNA: random depth; protein:
    the 40-bit code of esa_msd.h), with random rank-window sizes and, one case in
    four, without the pair path (everything through the doubling rounds),
  * a part build with 2..5 parts (thread transport on one device),
  * the device FASTA reader (random line widths, CRLF, blank lines) and the device
    FASTQ reader (four-line records, random qualities),
  * the packed-index builder (INDEX.bdx image: random block size, blocks per
    bucket, locate interval and mode, -sprank, both flavours),
each compared with the CPU oracle / host reader.  Dev tool; stops at the first
difference and prints the seed.

  python tools/fuzz_gpu.py --seconds 300 [--seed 1] [--first CASE]
"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import oracle_util as ou  # noqa: E402
import thread_comm  # noqa: E402
from fuzz_cases import (msd_switches, parts_switches, pck_options, prefix_length,  # noqa: E402
                        random_sequence, write_fasta, write_fastq)
from genometools_amd import encode, esa, pck  # noqa: E402


def check_engine(rng, enc, sigma):
    ora = ou.esa(enc, sigma)
    with esa.EsaEngine(enc.size, sigma) as eng:
        eng.set_sequence(enc)
        eng.set_prefixlength(prefix_length(rng, sigma))
        wide = os.environ.get("GTAMD_FORCE_WIDE") == "1"   # (no bucket table from a part build)
        eng.run(esa.WANT_SUF | esa.WANT_LCP | esa.WANT_BWT | (0 if wide else esa.WANT_BCK))
        res = eng.result()
        for name in ("suf", "lcp", "llv", "bwt"):
            assert np.array_equal(getattr(res, name), ora[name]), name
        kk = res.stats["prefixlength"]
        if not wide:
            for got, want in zip(eng.bcktab(), ou.bcktab(enc, sigma, kk)):
                assert np.array_equal(got, want), "bck k=%d" % kk
        assert res.stats["longest"] == ora["stats"]["longest"]
        assert res.stats["largelcpvalues"] == ora["stats"]["largelcpvalues"]
        assert res.stats["maxbranchdepth"] == ora["stats"]["maxbranchdepth"]
    return ora


_pck = None


def check_pck(rng, enc, sigma, ora):
    """INDEX.bdx from the tables of a fresh build against the oracle's restatement
    (skipped for a one-symbol sequence... no: total length 2 is fine)"""
    global _pck
    if _pck is None:
        _pck = pck.PackedIndex()
    kw = pck_options(rng, sigma)
    with esa.EsaEngine(enc.size, sigma) as eng:
        eng.set_sequence(enc)
        eng.run(esa.WANT_SUF | esa.WANT_BWT)
        _pck.build_from_esa(eng, **kw)
        got = _pck.image().tobytes()
    want = ou.pck_bdx(enc, sigma, ora["suf"], ora["bwt"], **kw)
    assert got == want, "packed index %r" % (kw,)


def check_msd(rng, enc, ora, sigma=4):
    """the most-significant-digit-first sort of big builds (esa_msd.h), forced
    at this size, with a random depth of level C, a random limit of the
    one-workgroup path and, one case in four, the LDS radix fallback in every run;
    the rank table of the rounds in windows of a random size (one case in three the
    whole table), random chunks of the pair comparison, the pairs' table entries at
    random places of the flow, a random crowded-bin limit, one case in four without
    the pair path"""
    env = msd_switches(rng)
    os.environ.update(env)
    try:
      try:
        with esa.EsaEngine(enc.size, sigma) as eng:
            eng.set_sequence(enc)
            eng.run(esa.WANT_SUF | esa.WANT_LCP | esa.WANT_BWT)
            res = eng.result()
            for name in ("suf", "lcp", "llv", "bwt"):
                assert np.array_equal(getattr(res, name), ora[name]), "msd %s %s" % (name, env)
            for k in ("longest", "largelcpvalues", "maxbranchdepth"):
                assert res.stats[k] == ora["stats"][k], "msd %s %s" % (k, env)
            assert res.stats["lcptabsum"] == int(ora["stats"]["lcptabsum"]), "msd lcptabsum %s" % env
      except Exception:
        print("check_msd: sigma %d %s" % (sigma, env), flush=True)
        raise
    finally:
        for k in env:
            os.environ.pop(k, None)


def check_parts(rng, enc, sigma, ora):
    parts, env = parts_switches(rng)
    os.environ.update(env)
    try:
        tabs = thread_comm.build_in_parts(enc, sigma, parts)[0]
        for name in ("suf", "lcp", "llv", "bwt"):
            assert np.array_equal(tabs[name], ora[name]), "parts=%d %s %s" % (parts, name, env)
    except Exception:
        print("check_parts: parts %d sigma %d %s" % (parts, sigma, env), flush=True)
        raise
    finally:
        for k in env:
            os.environ.pop(k, None)


def check_encoder(rng, enc, sigma, tmp):
    protein = sigma == 20
    path = os.path.join(tmp, "f.fa")
    write_fasta(rng, enc, sigma, path)
    with open(path, "rb") as f:
        written = f.read()
    try:
        want = ou.encode_fasta(path, protein)
    except ValueError as e:
        # round 1 stopped here once (seed 43038423): the stdio reader reported a
        # byte the file does not contain.  Tell a wrong file from a reader that
        # saw something else than the file: read it again, both ways.
        with open(path, "rb") as f:
            again = f.read()
        try:
            second = ou.encode_fasta(path, protein)
            verdict = "second read ok (%s)" % np.array_equal(second, enc)
        except ValueError as e2:
            verdict = "second read fails too: %s" % e2
        with open(os.path.join(ROOT, "gpurun_out", "fuzz_reader_failure.txt"), "w") as out:
            out.write("first: %s\nfile stable: %s, bytes in file not in alphabet: %s\n%s\n" % (
                e, written == again, sorted(set(written) - set(b">seq0123456789 sometxt\t\r\n"
                                                              b"ACGTNSYWRKVBDHMacgtnsywrkvbdhm"
                                                              b"LVIFKREDAGSTNQYWPHMCXUBZJO*-")),
                verdict))
            out.write(open("/proc/self/maps").read())
        raise
    if not np.array_equal(want, enc):
        # the writer above and the oracle's reader disagree -- or a read saw something else
        # than the file (round 1 met that once on a GPU box): keep what is needed to tell
        with open(path, "rb") as f:
            again = f.read()
        second = ou.encode_fasta(path, protein)
        with open(os.path.join(ROOT, "gpurun_out", "fuzz_decode_failure.fa"), "wb") as out:
            out.write(again)
        np.save(os.path.join(ROOT, "gpurun_out", "fuzz_decode_failure_first.npy"), want)
        raise AssertionError("the FASTA the fuzzer wrote does not decode back: file stable %s, second "
                             "decoding equals the sequence %s, first decoding equals the second %s, "
                             "sizes %d %d %d" % (written == again, np.array_equal(second, enc),
                                                 np.array_equal(second, want), enc.size, want.size,
                                                 second.size))
    # the same sequences as four-line FASTQ records
    qpath = os.path.join(tmp, "f.fastq")
    records = write_fastq(rng, enc, sigma, qpath)
    with encode.DeviceEncoder(protein=protein) as de:
        de.encode([qpath])
        assert np.array_equal(de.symbols(), enc), "device FASTQ reader symbols"
        assert int(de.fastq_records()[1].sum()) + records - 1 == enc.size
    with encode.DeviceEncoder(protein=protein) as de:
        de.encode([path])
        assert np.array_equal(de.symbols(), enc), "device reader symbols"
        s = de.summary()
        st = ou.seqstats(enc, sigma)
        for k in ("specialcharacters", "realspecialranges", "wildcards", "realwildcardranges",
                  "lengthofspecialprefix", "lengthofspecialsuffix", "numofsequences"):
            assert s[k] == st[k], k


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=120)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--first", type=int, default=0, help="first case number (to replay a stretch)")
    a = ap.parse_args()
    t0, case = time.time(), a.first
    with tempfile.TemporaryDirectory() as tmp:
        while time.time() - t0 < a.seconds:
            seed = a.seed * 1000003 + case
            rng = np.random.default_rng(seed)
            sigma = 20 if rng.integers(0, 4) == 0 else 4
            enc = random_sequence(rng, sigma)
            # every seventh case through the 64-bit position kernels / the
            # exchange machinery of a part build
            if case % 7 == 3:
                os.environ["GTAMD_FORCE_WIDE"] = "1"
            else:
                os.environ.pop("GTAMD_FORCE_WIDE", None)
            try:
                ora = check_engine(rng, enc, sigma)
                if case % 7 != 3 and enc.size >= 64:
                    check_msd(rng, enc, ora, sigma)
                if case % 3 == 0:
                    check_parts(rng, enc, sigma, ora)
                if enc.size <= 20000 and case % 2 == 0:
                    check_encoder(rng, enc, sigma, tmp)
                if case % 7 != 3:
                    check_pck(rng, enc, sigma, ora)
            except Exception:
                print("FAILED: seed %d case %d sigma %d n %d" % (seed, case, sigma, enc.size),
                      flush=True)
                np.save(os.path.join(ROOT, "gpurun_out", "fuzz_fail_%d.npy" % seed), enc)
                raise
            case += 1
            if case % 50 == 0:
                print("%d cases, %.0f s" % (case, time.time() - t0), flush=True)
    print("fuzz ok: %d cases in %.0f s" % (case, time.time() - t0))
    return 0


if __name__ == "__main__":
    sys.exit(main())
