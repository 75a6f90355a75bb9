"""Regenerate tests/golden/correct/ and tests/golden/golden_correct.json with a
GenomeTools binary:

    python tests/golden/make_golden_correct.py /path/to/bin/gt

Per set the reads are written as FASTA under tests/golden/correct/, and in a
working directory, with bare file names so that no path appears,

    gt suffixerator -mirrored -suf -lcp -ssp -indexname reads -db F
    gt readjoiner correct -k K -c C -ii reads

are run.  Recorded: md5 and size of reads.esq before and after, the reads it
decodes to afterwards (`gt encseq decode`), stdout, exit code and the seconds.
A second call of the reference would walk the tables of the reads as they were,
which this project builds anew: it is not recorded.  The reads after the call
are ASSERTED to be those of the restatement
tests/kcorrect_reference.py: the reference is the definition, and where the two
part the maker stops.

errors_1 is the reference's own test set (testdata/readjoiner/errors_1.fas and
errors_1.corrected.fas, k 12, c 2), copied here as data.  The sets `live`,
`chain`, `conflict` and `group_once` are found by a seeded search with the
restatement: a source that an earlier record wrote with another letter, a chain
of two such records, two records that write different letters to one position,
and a group that writes to its own source (the trusted letter is read once,
before the group's edits)."""
import hashlib
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import kcorrect_reference as kr  # noqa: E402

OUT = os.path.join(HERE, "correct")


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def searched():
    """name -> (reads, k, c) of the sets that pin the order rules"""
    sets = {}

    def find(name, length, count, k, c, seeds, want):
        seed = kr.search(want, length, count, k, c, seeds)
        assert seed is not None, name
        sets[name] = (kr.coverage_reads(seed, length, count), k, c)

    find("live", 20, 24, 6, 2, range(0, 400), lambda ia, ib, a, b: not same(a, b) and ia["chain"] == 1)
    find("chain", 12, 40, 4, 2, range(1000, 1400), lambda ia, ib, a, b: ia["chain"] >= 2 and not same(a, b))
    find("conflict", 20, 24, 6, 2, range(0, 400), lambda ia, ib, a, b: ia["conflicts"] >= 1 and ia["chain"] == 0)
    for seed in range(1000, 1400):
        reads = kr.coverage_reads(seed, 12, 40)
        a = kr.correct_reads(reads, 4, 2)[0]
        b = kr.correct_reads(reads, 4, 2, broken=("source_once_per_group",))[0]
        if not same(a, b):
            sets["group_once"] = (reads, 4, 2)
            break
    assert "group_once" in sets
    return sets


def all_sets(reference_testdata):
    sets = {"errors_1": (kr.parse_fasta(os.path.join(reference_testdata, "errors_1.fas")), 12, 2)}
    planted = kr.coverage_reads(7, 40, 120, errors=0.3, genome=200)
    clean = kr.coverage_reads(8, 40, 120, errors=0.0, genome=200)
    sets["planted"] = (planted, 13, 3)                  # the defaults 31 / 3 scaled to reads of 40 letters
    sets["clean"] = (clean, 13, 3)
    sets["c1"] = (planted, 13, 1)
    sets["k_is_length"] = (planted, 40, 2)
    sets["k_above_length"] = (planted, 41, 2)
    sets["k1"] = (planted, 1, 2)
    sets["none_trusted"] = (planted, 13, 1000)
    sets.update(searched())
    return sets


def digest(path):
    with open(path, "rb") as f:
        raw = f.read()
    return {"md5": hashlib.md5(raw).hexdigest(), "size": len(raw)}


def letters(reads):
    return ["".join("acgt"[int(x)] for x in r) for r in reads]


def call(gt, cwd, *args):
    p = subprocess.run([gt] + list(args), cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    return p.returncode, p.stdout.decode(), p.stderr.decode()


def index(gt, cwd, fasta):
    rc, _, err = call(gt, cwd, "suffixerator", "-mirrored", "-suf", "-lcp", "-ssp", "-indexname", "reads", "-db", fasta)
    assert rc == 0, err


def decoded(gt, cwd):
    rc, out, err = call(gt, cwd, "encseq", "decode", "reads")
    assert rc == 0, err
    path = os.path.join(cwd, "decoded.fas")
    with open(path, "w") as f:
        f.write(out)
    return kr.parse_fasta(path)


def main(gt, reference_testdata):
    gt = os.path.abspath(gt)
    os.makedirs(OUT, exist_ok=True)
    for name in ("errors_1.fas", "errors_1.corrected.fas"):
        shutil.copy(os.path.join(reference_testdata, name), OUT)
    golden = {"sets": {}, "refusals": {}}
    for name, (reads, k, c) in all_sets(reference_testdata).items():
        fasta = name + ".fas"
        if name != "errors_1":
            kr.write_fasta(os.path.join(OUT, fasta), reads)
        with tempfile.TemporaryDirectory() as tmp:
            shutil.copy(os.path.join(OUT, fasta), tmp)
            index(gt, tmp, fasta)
            entry = {"file": fasta, "k": k, "c": c, "reads": len(reads), "esq_before": digest(os.path.join(tmp, "reads.esq"))}
            want = reads
            for run in ("first",):
                began = time.time()
                rc, out, err = call(gt, tmp, "readjoiner", "correct", "-k", str(k), "-c", str(c), "-ii", "reads")
                seconds = time.time() - began
                assert rc == 0, (name, err)
                got = decoded(gt, tmp)
                want, _, info = kr.correct_reads(want, k, c)
                assert same(got, want), (name, run)          # the reference is the definition
                entry[run] = {"esq": digest(os.path.join(tmp, "reads.esq")), "reads": letters(got), "stdout": out, "exit": rc,
                              "records": info["records"], "changed": info["changed"], "chain": info["chain"],
                              "conflicts": info["conflicts"], "dependent": info["dependent"]}
                if run == "first":
                    entry["seconds"] = round(seconds, 4)
            if name == "errors_1":
                assert same(kr.parse_fasta(os.path.join(OUT, "errors_1.corrected.fas")),
                            [np.array(["acgt".index(ch) for ch in r], dtype=np.uint8) for r in entry["first"]["reads"]])
            golden["sets"][name] = entry
    for name in ("clean", "c1", "k_is_length", "k_above_length", "k1", "none_trusted"):
        assert golden["sets"][name]["first"]["records"] == 0, name
    # reads of two lengths: refused in words
    rng = np.random.default_rng(11)
    reads = [rng.integers(0, 4, 30 if i % 2 else 36, dtype=np.uint8) for i in range(12)]
    kr.write_fasta(os.path.join(OUT, "two_lengths.fas"), reads)
    with tempfile.TemporaryDirectory() as tmp:
        shutil.copy(os.path.join(OUT, "two_lengths.fas"), tmp)
        index(gt, tmp, "two_lengths.fas")
        before = digest(os.path.join(tmp, "reads.esq"))
        rc, out, err = call(gt, tmp, "readjoiner", "correct", "-k", "8", "-c", "2", "-ii", "reads")
        assert rc != 0 and digest(os.path.join(tmp, "reads.esq")) == before
        # the message alone: the line starts with the path of the binary
        golden["refusals"]["two_lengths"] = {"file": "two_lengths.fas", "k": 8, "c": 2, "exit": rc, "stdout": out,
                                             "message": err.strip().split("\n")[-1].split(": error: ", 1)[1]}
    with open(os.path.join(HERE, "golden_correct.json"), "w") as f:
        json.dump(golden, f, indent=1, sort_keys=True)
        f.write("\n")
    for name, e in sorted(golden["sets"].items()):
        print(name, e["k"], e["c"], {k: v for k, v in e["first"].items() if k not in ("reads", "esq")}, e["seconds"])
    print(golden["refusals"])


if __name__ == "__main__":
    binary = sys.argv[1]
    main(binary, sys.argv[2] if len(sys.argv) > 2 else
         os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(binary))), "testdata", "readjoiner"))
