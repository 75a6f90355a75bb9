"""Regenerate tests/golden/assembly/ and tests/golden/golden_assembly.json with a
GenomeTools binary:

    python tests/golden/make_golden_assembly.py /path/to/bin/gt

The read sets are made here from seeds and written as FASTA under
tests/golden/assembly/ (NAME.fna).  Per set the reference's `readjoiner
prefilter -fasta`, `readjoiner overlap -l L` and `readjoiner assembly` are run
with bare file names in a scratch directory, and recorded are: the reads the
prefilter kept (NAME.p.fas: the read set of the list's read numbers), the list
NAME.0.spm the overlap step wrote, and per call of the assembly step -- default
options, `-depthcutoff 1 -lengthcutoff 1`, and these with `-l` at the median
match length, which is above the shortest match -- md5 and size of NAME.contigs.fas and the
stdout verbatim, with the seconds of the default call.  Then the same list in a
seeded shuffled order (NAME.shuffled.0.spm, written here) and what the
reference assembles from it with the first two calls: the order of the list
decides the contig numbers at junctions.

    python tests/golden/make_golden_assembly.py /path/to/bin/gt --probe reads.fna L

records nothing of the above: it runs the three steps once on a large read set
-- the reads `tools/assembly_probe.py --write-fasta DIR` writes, the set its
device times are for -- and writes tests/golden/golden_assembly_probe.json: the
seconds of every step on one core, the CPU as /proc/cpuinfo names it, reads,
matches, and md5, size and statistics block of X.contigs.fas.  DESIGN.md 9o
sets these seconds beside the device times."""
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
import spmred_reference as rr  # noqa: E402

OUT = os.path.join(HERE, "assembly")
CALLS = {"default": [], "d1l1": ["-depthcutoff", "1", "-lengthcutoff", "1"]}


def _tiles(text, length, step, rng, flip=0.4):
    reads, at = [], 0
    while True:
        k = length if isinstance(length, int) else int(rng.integers(length[0], length[1] + 1))
        if at + k > text.size:
            break
        r = text[at:at + k].copy()
        reads.append(rr.revcomp(r) if rng.random() < flip else r)
        at += step + int(rng.integers(0, 2))
    return [reads[k] for k in rng.permutation(len(reads))]


def read_sets():
    """name -> (reads, minimum match length of the overlap step)"""
    sets = {}
    rng = np.random.default_rng(701)
    text = rng.integers(0, 4, 3600, dtype=np.uint8)
    text[2200:2500] = text[600:900]
    sets["rep2"] = (_tiles(text, 100, 10, rng), 45)
    rng = np.random.default_rng(702)
    starts = np.concatenate([[0], np.cumsum(rng.integers(6, 11, 50))])
    ring = rng.integers(0, 4, int(starts[-1]), dtype=np.uint8)
    text = np.concatenate([ring, ring[:40]])
    reads = [text[a:a + 40].copy() for a in starts[:-1].tolist()]
    sets["circ"] = ([rr.revcomp(r) if rng.random() < 0.5 else r for r in reads], 20)
    rng = np.random.default_rng(703)
    text = rng.integers(0, 4, 900, dtype=np.uint8)
    text[600:680] = text[200:280]
    # (reads of several lengths: the reference's prefilter leaves contained reads in, its overlap step lists
    # them in X.0.cnt and its assembly step skips their matches; this set has none)
    sets["var"] = (rr.containment_free(_tiles(text, (30, 49), 6, rng)), 20)
    rng = np.random.default_rng(704)
    text = rng.integers(0, 4, 800, dtype=np.uint8)
    text[500:560] = rr.revcomp(text[200:260])
    sets["inv"] = (_tiles(text, 40, 6, rng), 20)
    rng = np.random.default_rng(705)
    sets["none"] = ([rng.integers(0, 4, 40, dtype=np.uint8) for _ in range(30)], 20)
    rng = np.random.default_rng(706)
    text = rng.integers(0, 4, 1500, dtype=np.uint8)
    text[700:760] = text[300:360]
    text[1100:1160] = text[300:360]
    sets["rep3"] = (_tiles(text, 40, 5, rng, flip=0.0), 22)
    return sets


def run(gt, cwd, *args):
    p = subprocess.run([gt, "readjoiner"] + list(args), cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0, (args, p.stderr)
    return p.stdout


def assemble(gt, cwd, name, options):
    fas = os.path.join(cwd, name + ".contigs.fas")
    if os.path.exists(fas):
        os.remove(fas)
    began = time.time()
    out = run(gt, cwd, "assembly", "-readset", name, *options)
    seconds = time.time() - began
    with open(fas, "rb") as f:
        raw = f.read()
    return {"md5": hashlib.md5(raw).hexdigest(), "size": len(raw), "stdout": out.decode()}, seconds


def main(gt):
    gt = os.path.abspath(gt)
    os.makedirs(OUT, exist_ok=True)
    golden = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, (reads, min_len) in read_sets().items():
            pr.write_fasta(os.path.join(OUT, name + ".fna"), reads)
            shutil.copy(os.path.join(OUT, name + ".fna"), tmp)
            run(gt, tmp, "prefilter", "-db", name + ".fna", "-readset", name, "-fasta")
            run(gt, tmp, "overlap", "-readset", name, "-l", str(min_len))
            shutil.copy(os.path.join(tmp, name + ".p.fas"), OUT)
            spm = os.path.join(tmp, name + ".0.spm")
            shutil.copy(spm, OUT)
            with open(spm, "rb") as f:
                raw = f.read()
            words = np.frombuffer(raw[1:], dtype="<u4").reshape(-1, 3)
            entry = {"min_len": min_len, "reads": len(pr.parse_reads(os.path.join(tmp, name + ".p.fas"))),
                     "matches": int(words.shape[0]), "calls": {}, "shuffled": {}}
            calls = dict(CALLS)
            if words.shape[0]:
                entry["l"] = int(np.median(words[:, 2] >> 2))
                assert entry["l"] > int((words[:, 2] >> 2).min()), name
                calls["l"] = ["-l", str(entry["l"])] + CALLS["d1l1"]
            for key, options in calls.items():
                entry["calls"][key], seconds = assemble(gt, tmp, name, options)
                if key == "default":
                    entry["seconds"] = round(seconds, 4)
            order = np.random.default_rng(900).permutation(words.shape[0])
            shuffled = raw[:1] + np.ascontiguousarray(words[order]).tobytes()
            with open(os.path.join(OUT, name + ".shuffled.0.spm"), "wb") as f:
                f.write(shuffled)
            with open(spm, "wb") as f:
                f.write(shuffled)
            for key, options in CALLS.items():
                entry["shuffled"][key], _ = assemble(gt, tmp, name, options)
            golden[name] = entry
    with open(os.path.join(HERE, "golden_assembly.json"), "w") as f:
        json.dump(golden, f, indent=1, sort_keys=True)
        f.write("\n")
    for name, e in sorted(golden.items()):
        print(name, {k: v for k, v in e.items() if k not in ("calls", "shuffled")},
              {k: (c["size"], c["stdout"].count("\n")) for k, c in e["calls"].items()},
              {k: c["md5"] == e["calls"][k]["md5"] for k, c in e["shuffled"].items()})


def cpu():
    """the CPU as /proc/cpuinfo names it: the name alone may hold no number"""
    fields = {}
    with open("/proc/cpuinfo") as f:
        for line in f:
            key, _, value = line.partition(":")
            if key.strip() in ("model name", "cpu family", "model", "stepping", "cpu MHz") and key.strip() not in fields:
                fields[key.strip()] = value.strip()
    return fields


def probe(gt, fasta, min_len):
    gt = os.path.abspath(gt)
    entry = {"min_len": min_len, "cpu": cpu(), "seconds": {}}
    with tempfile.TemporaryDirectory() as tmp:
        shutil.copy(fasta, os.path.join(tmp, "reads.fna"))
        for step, args in (("prefilter", ["prefilter", "-db", "reads.fna", "-readset", "x", "-q"]),
                           ("overlap", ["overlap", "-readset", "x", "-l", str(min_len), "-q"])):
            began = time.time()
            run(gt, tmp, *args)
            entry["seconds"][step] = round(time.time() - began, 3)
        entry["contigs"], seconds = assemble(gt, tmp, "x", [])
        entry["seconds"]["assembly"] = round(seconds, 3)
        lines = entry["contigs"]["stdout"].splitlines()
        entry["reads"] = int(lines[1].split("=")[1])
        entry["matches"] = (os.path.getsize(os.path.join(tmp, "x.0.spm")) - 1) // 12
    with open(os.path.join(HERE, "golden_assembly_probe.json"), "w") as f:
        json.dump(entry, f, indent=1, sort_keys=True)
        f.write("\n")
    print({k: v for k, v in entry.items() if k != "contigs"}, entry["contigs"]["md5"], entry["contigs"]["size"])


if __name__ == "__main__":
    if len(sys.argv) == 5 and sys.argv[2] == "--probe":
        probe(sys.argv[1], sys.argv[3], int(sys.argv[4]))
    else:
        main(sys.argv[1])
