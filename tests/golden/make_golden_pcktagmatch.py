"""Regenerate tests/golden/golden_pcktagmatch.json and tests/golden/pcktagmatch/
with a GenomeTools binary:

    python tests/golden/make_golden_pcktagmatch.py /path/to/bin/gt

The tag files are those of make_golden_tagmatch.py (tests/golden/tagmatch/), the
calls those of its calls that have no wildcard option, with `-pck INDEX` in the
place of `-esa INDEX`.  The index is the one of the reference's index searches
(gt_idxsearch_include.rb:67-68):

    gt packedindex mkindex -tis -ssp -sprank -bsize 10 -locfreq 32 -dir rev -dna -pl

(-protein for sw100K1.fsa); for Atinsert.fna and trna_glutamine.fna the same
calls run on two more flavours, the defaults and -locbitmap.  Kept per call, as
golden_tagmatch.json keeps them: the exit code and the error, and md5 and line
count of the stdout with the `# indexname` and `# queryfile` lines dropped and
the match lines SORTED inside each tag's block; and whether that md5 is the one
golden_tagmatch.json has for the same call with -esa ("as_esa").  The two calls
with a wildcard option (-e 2 -withwildcards [no], on RandomN and Atinsert) are
recorded under "wildcard_calls": no test holds the device to them.  Three small
outputs lie whole under tests/golden/pcktagmatch/, and so does the INDEX.bdx the
reference wrote for trna_glutamine.fna (trna_glutamine.bdx)."""
import hashlib
import json
import os
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_tagmatch as esa_side  # noqa: E402

FIXTURES = esa_side.FIXTURES
TAGS = esa_side.OUT
OUT = os.path.join(HERE, "pcktagmatch")
SUITE = ["-sprank", "-bsize", "10", "-locfreq", "32"]
FLAVOURS = {"suite": SUITE, "defaults": [], "locbitmap": ["-locbitmap"]}
MORE_FLAVOURS = ("Atinsert.fna", "trna_glutamine.fna")
TEXTS = {"trna-e1": "trna_glutamine.fna|dna|-e 1|trna_glutamine.fna|suite",
         "duplicate-e0": "Duplicate.fna|dna|-e 0|Duplicate.fna|suite",
         "ttt-best": "TTT-small.fna|dna|-e 2 -best|TTT-small.fna|suite"}
IMAGE = ("trna_glutamine.fna", "suite", "trna_glutamine.bdx")


def cases():
    for subject, alphabet, args, tagsof in esa_side.cases():
        wild = "-withwildcards" in args
        for flavour in FLAVOURS:
            if flavour == "suite" or (subject in MORE_FLAVOURS and not wild):
                yield subject, alphabet, args, tagsof, flavour, wild


def main(gt):
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(HERE, "golden_tagmatch.json")) as f:
        esa_calls = json.load(f)["calls"]
    calls, wildcard_calls = {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        built = {}
        for subject, alphabet, args, tagsof, flavour, wild in cases():
            if (subject, flavour) not in built:
                built[subject, flavour] = os.path.join(tmp, "pck%d" % len(built))
                subprocess.run([gt, "packedindex", "mkindex", "-tis", "-ssp"] + FLAVOURS[flavour] +
                               ["-dir", "rev", "-" + alphabet, "-pl", "-indexname", built[subject, flavour],
                                "-db", os.path.join(FIXTURES, subject)], check=True, stdout=subprocess.DEVNULL)
                if (subject, flavour) == IMAGE[:2]:
                    shutil.copyfile(built[subject, flavour] + ".bdx", os.path.join(OUT, IMAGE[2]))
            cmd = [gt, "tagerator"] + args + ["-pck", built[subject, flavour], "-q"] + \
                  [os.path.join(TAGS, t + ".tags.fna") for t in tagsof]
            run = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
            text = esa_side.compared(run.stdout)
            esa_key = "%s|%s|%s|%s" % (subject, alphabet, " ".join(args), ",".join(tagsof))
            key = esa_key + "|" + flavour
            error = run.stderr.decode("latin-1").strip()
            md5 = hashlib.md5(text).hexdigest()
            (wildcard_calls if wild else calls)[key] = {
                "md5": md5, "lines": text.count(b"\n"), "exit": run.returncode,
                "error": error[error.index("error: ") + 7:] if "error: " in error else "",
                "as_esa": md5 == esa_calls[esa_key]["md5"] and run.returncode == esa_calls[esa_key]["exit"]}
            for name, k in TEXTS.items():
                if k == key:
                    with open(os.path.join(OUT, name), "wb") as f:
                        f.write(text)
    assert all(k in calls for k in TEXTS.values())
    with open(os.path.join(HERE, "golden_pcktagmatch.json"), "w") as f:
        json.dump({"calls": calls, "wildcard_calls": wildcard_calls, "texts": TEXTS, "image": list(IMAGE)}, f,
                  indent=1, sort_keys=True)
        f.write("\n")
    both = dict(calls, **wildcard_calls)
    print("%d calls and %d with a wildcard option, %d lines, %d end with an error, %d differ from -esa: %s" % (
        len(calls), len(wildcard_calls), sum(c["lines"] for c in both.values()),
        sum(c["exit"] != 0 for c in both.values()), sum(not c["as_esa"] for c in both.values()),
        sorted(k for k, c in both.items() if not c["as_esa"])))


if __name__ == "__main__":
    main(sys.argv[1])
