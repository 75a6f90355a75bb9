"""Regenerate tests/golden/prefilter/ and tests/golden/golden_prefilter.json with a
GenomeTools binary:

    python tests/golden/make_golden_prefilter.py /path/to/bin/gt

The read sets are made here, by the seeded generators of
tests/prefilter_reference.py, and written as FASTA or FASTQ under
tests/golden/prefilter/.  Per set of reads of ONE length the calls `gt readjoiner
prefilter -db FILES -readset NAME` are recorded, run with bare file names in the
working directory so that no path appears: the stdout of the default call, of
the -v call (with `-libtable no`: X.rlt holds an address of the process and its
line is not part of what this project prints) and of the -encodeonly -v call,
verbatim; md5 and size of X.esq, X.p.fas and X.cnt of the call with -fasta -cnt,
and of X.esq of the -encodeonly call; the seconds the default call took.  The
reference's kept reads are ASSERTED to be those of the brute force of the
definition (tests/prefilter_reference.py) for every such set; X.rlt is never
recorded.

For two sets of reads of SEVERAL lengths only what the reference keeps is
recorded (from -fasta), asserted to hold every read the definition keeps, with
the number of reads it keeps beyond them: the reference departs from its
definition there (include/gtamd_contained.h), and these entries pin nothing of
this project's output."""
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
import prefilter_reference as pr  # noqa: E402
from spmred_reference import revcomp  # noqa: E402

OUT = os.path.join(HERE, "prefilter")


def _random(seed, count, length=36):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 4, length, dtype=np.uint8) for _ in range(count)]


def equal_sets():
    """name -> [(file name, format, reads, width of a FASTA line or None)]"""
    sets = {}
    r = _random(1, 12)
    sets["dups"] = [("dups.fna", "fasta", r[:8] + [r[2], r[5]] + r[8:] + [r[2], r[11]], None)]
    r = _random(2, 10)
    sets["mirror"] = [("mirror.fna", "fasta", [revcomp(r[0]), r[1], r[0], r[2], revcomp(r[2]), r[3], revcomp(r[0])] + r[4:],
                       None)]
    rng = np.random.default_rng(3)
    p = pr.self_complementary(rng, 36)
    r = _random(4, 8)
    sets["selfc1"] = [("selfc1.fna", "fasta", r[:3] + [p] + r[3:], None)]
    sets["selfc2"] = [("selfc2.fna", "fasta", r[:3] + [p] + r[3:6] + [p] + r[6:], None)]
    sets["run70"] = [("run70.fna", "fasta", pr.copies_on_both_strands(70, 70), None)]
    a, b = pr.seeded_reads(101, 36), pr.seeded_reads(102, 36)
    sets["twofiles"] = [("two_a.fna", "fasta", a[:30] + [b[3]], 20), ("two_b.fq", "fastq", b[:25] + [a[4], revcomp(a[7])], None)]
    r = pr.seeded_reads(103, 36)
    wild = r[5].copy()
    wild[11] = 254
    other = r[9].copy()
    other[[0, 35]] = 254
    sets["wildcard"] = [("wildcard.fna", "fasta", r[:20] + [wild] + r[20:40] + [other] + r[40:], None)]
    r = _random(5, 1)[0]
    sets["one"] = [("one.fna", "fasta", [r, revcomp(r), r, r, revcomp(r)], None)]
    sets["len1"] = [("len1.fna", "fasta", _random(6, 40, 1), None)]
    sets["seeded"] = [("seeded.fna", "fasta", pr.seeded_reads(100, 36), None)]
    return sets


def write_set(files, where):
    for name, form, reads, width in files:
        path = os.path.join(where, name)
        if form == "fasta":
            pr.write_fasta(path, reads, width)
        else:
            pr.write_fastq(path, reads)


def digest(path):
    with open(path, "rb") as f:
        raw = f.read()
    return {"md5": hashlib.md5(raw).hexdigest(), "size": len(raw)}


def run(gt, cwd, names, readset, *options):
    p = subprocess.run([gt, "readjoiner", "prefilter", "-db"] + names + ["-readset", readset] + list(options), cwd=cwd,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    return p.returncode, p.stdout


def kept_of(path):
    return [r.tobytes() for r in pr.parse_reads(path)] if os.path.getsize(path) else []


def main(gt):
    gt = os.path.abspath(gt)
    os.makedirs(OUT, exist_ok=True)
    golden = {"equal": {}, "variable": {}}
    with tempfile.TemporaryDirectory() as tmp:
        for name, files in equal_sets().items():
            write_set(files, OUT)
            names = [f[0] for f in files]
            for n in names:
                shutil.copy(os.path.join(OUT, n), tmp)
            began = time.time()
            rc, default = run(gt, tmp, names, name)
            seconds = time.time() - began
            assert rc == 0, name
            rc, verbose = run(gt, tmp, names, name, "-v", "-libtable", "no", "-fasta", "-cnt")
            assert rc == 0, name
            entry = {"files": names, "stdout": default.decode(), "stdout_v": verbose.decode(), "seconds": round(seconds, 4)}
            for ext in ("esq", "p.fas", "cnt"):
                path = os.path.join(tmp, "%s.%s" % (name, ext))
                if os.path.exists(path):
                    entry[ext] = digest(path)
            # the reference is the definition here
            _, valid = pr.file_figures([os.path.join(tmp, n) for n in names])
            reads = [r for r, _ in valid]
            v = pr.verdicts(reads)
            want = [r.tobytes() for r in pr.kept_reads(reads, v)]
            assert kept_of(os.path.join(tmp, name + ".p.fas")) == want, name
            entry["kept"] = len(want)
            for gone in ("esq", "ssp"):
                if os.path.exists(os.path.join(tmp, "%s.%s" % (name, gone))):
                    os.remove(os.path.join(tmp, "%s.%s" % (name, gone)))
            rc, only = run(gt, tmp, names, name, "-v", "-libtable", "no", "-encodeonly")
            assert rc == 0, name
            entry["stdout_encodeonly"] = only.decode()
            entry["esq_encodeonly"] = digest(os.path.join(tmp, name + ".esq"))
            assert not os.path.exists(os.path.join(tmp, name + ".ssp")), name
            assert not any(k.endswith("rlt") for k in entry), name
            golden["equal"][name] = entry
        seed = 200
        while len(golden["variable"]) < 2:
            name = "var%d" % seed
            reads = pr.seeded_reads(seed, (20, 60))
            pr.write_fasta(os.path.join(tmp, name + ".fna"), reads)
            rc, _ = run(gt, tmp, [name + ".fna"], name, "-fasta")
            seed += 1
            if rc != 0:                                  # (the reference ends on an assertion for some)
                continue
            shutil.copy(os.path.join(tmp, name + ".fna"), OUT)
            got = kept_of(os.path.join(tmp, name + ".p.fas"))
            want = [r.tobytes() for r in pr.kept_reads(reads, pr.verdicts(reads))]
            at = 0
            for r in got:                                # the definition's kept reads, in order, among the reference's
                at += at < len(want) and r == want[at]
            assert at == len(want), name
            golden["variable"][name] = {"files": [name + ".fna"], "reference_keeps": len(got),
                                        "definition_keeps": len(want), "more": len(got) - len(want)}
    with open(os.path.join(HERE, "golden_prefilter.json"), "w") as f:
        json.dump(golden, f, indent=1, sort_keys=True)
        f.write("\n")
    for kind in ("equal", "variable"):
        for name, e in sorted(golden[kind].items()):
            print(kind, name, {k: v for k, v in e.items() if not k.startswith("stdout")})


if __name__ == "__main__":
    main(sys.argv[1])
