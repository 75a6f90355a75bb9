"""Regenerate tests/golden/golden_repfind.json with a GenomeTools binary:

    python tests/golden/make_golden_repfind.py /path/to/bin/gt

For the nine DNA fixtures the reference's suite searches at -l 8, 14 and 20,
and sw100K1.fsa as protein at -l 6 and 10, with the index `gt suffixerator
-dna|-protein -suf -lcp -tis -ssp`: md5 and line count of the stdout of
`gt repfind -l L -ii INDEX`, its lines starting with `#` dropped, runs of white
space made one blank, the lines sorted and each ended by a newline (the
reference emits in the order of its traversal, which is not part of the
semantics).  The two results the reference itself records
(testdata/repfind-result/) lie whole under tests/golden/repfind/."""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURES = os.path.join(HERE, "fixtures")
DNA = ["Atinsert.fna", "Duplicate.fna", "Random-Small.fna", "Random.fna", "Random159.fna",
       "Random160.fna", "RandomN.fna", "TTT-small.fna", "trna_glutamine.fna"]
CASES = [(name, "dna", l) for name in DNA for l in (8, 14, 20)] + \
        [("sw100K1.fsa", "protein", l) for l in (6, 10)]


def digest(raw):
    lines = sorted(" ".join(l.split()) for l in raw.decode("latin-1").splitlines()
                   if l.strip() and not l.startswith("#"))
    text = "".join(l + "\n" for l in lines).encode("latin-1")
    return {"md5": hashlib.md5(text).hexdigest(), "lines": len(lines)}


def main(gt):
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        built = None
        for name, alphabet, minlen in CASES:
            idx = os.path.join(tmp, "sfx")
            if built != name:
                subprocess.run([gt, "suffixerator", "-" + alphabet, "-suf", "-lcp", "-tis", "-ssp",
                                "-indexname", idx, "-db", os.path.join(FIXTURES, name)], check=True,
                               stdout=subprocess.DEVNULL)
                built = name
            raw = subprocess.run([gt, "repfind", "-l", str(minlen), "-ii", idx], check=True,
                                 stdout=subprocess.PIPE).stdout
            out["%s|%s|%d" % (name, alphabet, minlen)] = digest(raw)
    with open(os.path.join(HERE, "golden_repfind.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%d calls, %d lines" % (len(out), sum(e["lines"] for e in out.values())))


if __name__ == "__main__":
    main(sys.argv[1])
