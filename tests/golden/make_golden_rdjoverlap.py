"""Regenerate tests/golden/rdj/ and tests/golden/golden_rdjoverlap.json with a
GenomeTools binary:

    python tests/golden/make_golden_rdjoverlap.py /path/to/bin/gt

The read sets are made here, by the seeded generator of
tests/spmred_reference.py, and written as FASTA under tests/golden/rdj/: reads
tiled over a random text with a planted repeat and its reverse complement, four
in ten reverse-complemented, and free of containment on both strands (no
duplicate, no read inside another one or its reverse complement, no read equal to
its own reverse complement), which is what `gt readjoiner overlap` is made for:
`equal.fna`, reads of 36 letters; `mixed.fna`, of 25 to 60 letters; `long.fna`, of
300 to 600 letters, so that LCP values pass a byte.  Recorded per call `gt
readjoiner overlap -readset X -l L [-elimtrans no] -showspm` (X from `gt encseq
encode`): its `#` lines verbatim, md5 and line count of its match lines SORTED as
text (the order of the reference's traversal is not part of the semantics:
include/gtamd_spmred.h), and, from the call without -showspm, the md5 of the
sorted records of X.0.spm, each as the line -showspm prints for it.  Two small
sorted outputs lie whole under tests/golden/rdj/."""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import spmred_reference as rr  # noqa: E402

OUT = os.path.join(HERE, "rdj")
SETS = {"equal.fna": dict(seed=31, text_len=1100, length=36, step=5, repeat=80),
        "mixed.fna": dict(seed=32, text_len=1100, length=(25, 60), step=5, repeat=80),
        "long.fna": dict(seed=59, text_len=6000, length=(300, 600), step=55, repeat=400)}
CALLS = {"equal.fna": (12, 20), "mixed.fna": (12, 20), "long.fna": (100, 260)}
TEXTS = {"equal-l20.spm": "equal.fna|20|yes", "mixed-l20.spm": "mixed.fna|20|yes"}


def split_output(raw):
    """(`#` lines in order, match lines sorted)"""
    lines = raw.decode().splitlines()
    return [l for l in lines if l.startswith("#")], sorted(l for l in lines if not l.startswith("#"))


def text_of(lines):
    return "".join(l + "\n" for l in lines).encode()


def check_set(name, reads, lines):
    """what a set must hold at its smaller minimum length, by the reference's own lines"""
    forms = {tuple(l.split()[1::2]) for l in lines}
    assert {("+", "+"), ("+", "-"), ("-", "+")} <= forms, (name, forms)
    # the successors of a read on a strand, from both mirror images of every line
    out = {}
    for l in lines:
        sn, sd, pn, pd, _ = l.split()
        out.setdefault((sn, sd), set()).add((pn, pd))
        out.setdefault((pn, "-" if pd == "+" else "+"), set()).add((sn, "-" if sd == "+" else "+"))
    assert max(len(v) for v in out.values()) >= 2, name
    assert len(rr.containment_free(reads)) == len(reads), name


def main(gt):
    os.makedirs(OUT, exist_ok=True)
    calls = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, how in SETS.items():
            reads = rr.tiled_reads(**how)
            with open(os.path.join(OUT, name), "w") as f:
                for k, r in enumerate(reads):
                    f.write(">read%d\n%s\n" % (k, "".join("acgt"[c] for c in r)))
            idx = os.path.join(tmp, name[:-4])
            subprocess.run([gt, "encseq", "encode", "-indexname", idx, os.path.join(OUT, name)], check=True,
                           stdout=subprocess.DEVNULL)
            for L in CALLS[name]:
                for elim in ("yes", "no"):
                    base = [gt, "readjoiner", "overlap", "-readset", idx, "-l", str(L), "-elimtrans", elim]
                    hashes, lines = split_output(subprocess.run(base + ["-showspm"], check=True,
                                                                stdout=subprocess.PIPE).stdout)
                    assert len(set(lines)) == len(lines)
                    quiet = subprocess.run(base + ["-q"], check=True, stdout=subprocess.PIPE).stdout
                    assert quiet == b""
                    with open(idx + ".0.spm", "rb") as f:
                        records = rr.parse_bin32(f.read())
                    from_file = sorted("%d %s %d %s %d" % (sn, "+" if fl & 2 else "-", pn, "+" if fl & 1 else "-", k)
                                       for sn, pn, k, fl in records)
                    assert from_file == lines, (name, L, elim)
                    key = "%s|%d|%s" % (name, L, elim)
                    calls[key] = {"hash_lines": hashes, "md5": hashlib.md5(text_of(lines)).hexdigest(),
                                  "lines": len(lines), "spm_md5": hashlib.md5(text_of(from_file)).hexdigest(),
                                  "reads": len(reads)}
                    if elim == "yes" and L == CALLS[name][0]:
                        transitive = int(hashes[-1].split("=")[1])
                        assert len(lines) >= 50 and transitive >= 100, (key, len(lines), transitive)
                        check_set(name, reads, lines)
                    for out, want in TEXTS.items():
                        if want == key:
                            with open(os.path.join(OUT, out), "wb") as f:
                                f.write(text_of(lines))
    assert all(k in calls for k in TEXTS.values())
    with open(os.path.join(HERE, "golden_rdjoverlap.json"), "w") as f:
        json.dump({"calls": calls, "texts": TEXTS}, f, indent=1, sort_keys=True)
        f.write("\n")
    for k in sorted(calls):
        print(k, calls[k]["lines"], calls[k]["hash_lines"][2:])


if __name__ == "__main__":
    main(sys.argv[1])
