"""Regenerate tests/golden/spm/ and tests/golden/golden_spm.json with a
GenomeTools binary:

    python tests/golden/make_golden_spm.py /path/to/bin/gt

The read sets are made here, by a seeded generator, and written as FASTA under
tests/golden/spm/: `mixed.fna`, reads of 25 to 60 letters cut from a random 1.5
kbp text, three in ten reverse-complemented, with exact duplicates, a
reverse-complemented duplicate, reads contained in other reads, a homopolymer, a
tandem repeat and a reverse-complement palindrome; `equal.fna`, the same with
reads of 36 letters throughout.  None holds a wildcard: the reference aborts on
one.  Recorded per call `gt encseq2spm -l L -ii X -spm show` (X from `gt encseq
encode`): md5 and line count of its stdout SORTED as text (the order of the
reference's traversal is not part of the semantics: include/gtamd_spm.h), and
the number `-spm count` prints.  Every set is called with four minimum lengths,
the last above every read length; the fixtures Reads1.fna, Reads2.fna and
Reads3.fna -- 100 reads of 50 letters, nearly all of them duplicates -- with L =
20.  Two small sorted outputs lie whole under tests/golden/spm/."""
import hashlib
import json
import os
import random
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "spm")
COMPLEMENT = {"a": "t", "c": "g", "g": "c", "t": "a"}
CALLS = {"spm/mixed.fna": (12, 20, 30, 61), "spm/equal.fna": (12, 20, 36, 37),
         "fixtures/Reads1.fna": (20,), "fixtures/Reads2.fna": (20,), "fixtures/Reads3.fna": (20,)}
TEXTS = {"mixed-l30.spm": "spm/mixed.fna|30", "equal-l36.spm": "spm/equal.fna|36"}


def revcomp(s):
    return "".join(COMPLEMENT[c] for c in reversed(s))


def read_set(seed, lengths, contained):
    """about 250 reads; lengths() gives the length of the next one"""
    rng = random.Random(seed)
    text = "".join(rng.choice("acgt") for _ in range(1500))
    reads = []
    for _ in range(236):
        k = lengths(rng)
        at = rng.randrange(len(text) - k + 1)
        r = text[at:at + k]
        reads.append(revcomp(r) if rng.random() < 0.3 else r)
    for k in range(6):                                   # exact duplicates
        reads.append(reads[7 * k + 3])
    reads.append(revcomp(reads[5]))                      # a reverse-complemented duplicate
    for k in range(4 if contained else 0):               # reads inside other reads
        r = reads[11 * k + 2]
        reads.append(r[3:len(r) - 2])
    reads.append("a" * lengths(rng))                     # a homopolymer
    reads.append(("acg" * 30)[:lengths(rng)])            # a tandem repeat
    half = "".join(rng.choice("acgt") for _ in range(lengths(rng) // 2))
    reads.append(half + revcomp(half))                   # a reverse-complement palindrome
    rng.shuffle(reads)
    return reads


def write_sets():
    os.makedirs(OUT, exist_ok=True)
    sets = {"mixed.fna": read_set(20261, lambda rng: rng.randint(25, 60), True),
            "equal.fna": read_set(20262, lambda rng: 36, False)}
    for name, reads in sets.items():
        assert all(set(r) <= set("acgt") for r in reads)
        with open(os.path.join(OUT, name), "w") as f:
            for k, r in enumerate(reads):
                f.write(">read%d\n%s\n" % (k, r))
    assert len({len(r) for r in sets["equal.fna"]}) == 1 and len({len(r) for r in sets["mixed.fna"]}) > 20


def read_lengths(path):
    """the lengths of the sequences of the mirrored set of a FASTA file"""
    lengths = []
    with open(path) as f:
        for line in f:
            if line.startswith(">"):
                lengths.append(0)
            else:
                lengths[-1] += len(line.strip())
    return lengths + lengths[::-1]


def main(gt):
    write_sets()
    calls = {}
    with tempfile.TemporaryDirectory() as tmp:
        for k, (name, lengths) in enumerate(CALLS.items()):
            idx = os.path.join(tmp, "reads%d" % k)
            subprocess.run([gt, "encseq", "encode", "-indexname", idx, os.path.join(HERE, name)], check=True,
                           stdout=subprocess.DEVNULL)
            nontrivial = []
            for L in lengths:
                base = [gt, "encseq2spm", "-l", str(L), "-ii", idx, "-spm"]
                show = subprocess.run(base + ["show"], check=True, stdout=subprocess.PIPE).stdout.decode()
                lines = sorted(show.splitlines())
                assert len(set(lines)) == len(lines)
                text = "".join(l + "\n" for l in lines).encode()
                count = subprocess.run(base + ["count"], check=True, stdout=subprocess.PIPE).stdout.decode()
                assert count == "number of suffix-prefix matches=%d\n" % len(lines), count
                # the trivial triples: a sequence with itself in its whole length
                seqlen = read_lengths(os.path.join(HERE, name))
                trivial = sum(s == t and k == seqlen[s] for s, t, k in (map(int, l.split()) for l in lines))
                key = "%s|%d" % (name, L)
                calls[key] = {"md5": hashlib.md5(text).hexdigest(), "lines": len(lines), "count": len(lines),
                              "trivial": trivial}
                nontrivial.append(len(lines) - trivial)
                for out, want in TEXTS.items():
                    if want == key:
                        with open(os.path.join(OUT, out), "wb") as f:
                            f.write(text)
            # every set has more than 100 lines that are no trivial triple, its last
            # generated call none at all
            assert nontrivial[0] > 100, (name, nontrivial)
            if name.startswith("spm/"):
                assert calls["%s|%d" % (name, lengths[-1])]["lines"] == 0
    assert any(c["trivial"] > 0 for c in calls.values())
    assert all(calls[k]["lines"] > 0 for k in TEXTS.values())
    with open(os.path.join(HERE, "golden_spm.json"), "w") as f:
        json.dump({"calls": calls, "texts": TEXTS}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%d calls, %d lines" % (len(calls), sum(c["lines"] for c in calls.values())))
    for k in sorted(calls):
        print(k, calls[k])


if __name__ == "__main__":
    main(sys.argv[1])
