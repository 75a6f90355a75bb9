"""Regenerate tests/golden/golden_pcklocali.json and tests/golden/pcklocali/ with a
GenomeTools binary:

    python tests/golden/make_golden_pcklocali.py /path/to/bin/gt

The query files are those of make_golden_locali.py (tests/golden/locali/), the
calls those of its calls that reach a query, with `-pck INDEX` in the place of
`-esa INDEX`.  The index is the one of the reference's index searches
(gt_idxsearch_include.rb:67-68):

    gt packedindex mkindex -tis -ssp -sprank -bsize 10 -locfreq 32 -dir rev -dna -pl

(-protein for sw100K1.fsa); for Atinsert.fna and trna_glutamine.fna the same
calls run on two more flavours, the defaults and -locbitmap.  Kept per call, as
golden_locali.json keeps them: the exit code and the error, and md5 and line
count of the stdout with the `# indexname` and `# queryfile` lines dropped and
the match blocks SORTED inside each query; and whether that md5 and exit code
are those golden_locali.json has for the same call with -esa ("as_esa").  Three
small outputs lie whole under tests/golden/pcklocali/."""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_locali as esa_side  # noqa: E402

FIXTURES = esa_side.FIXTURES
QUERIES = esa_side.OUT
OUT = os.path.join(HERE, "pcklocali")
SUITE = ["-sprank", "-bsize", "10", "-locfreq", "32"]
FLAVOURS = {"suite": SUITE, "defaults": [], "locbitmap": ["-locbitmap"]}
MORE_FLAVOURS = ("Atinsert.fna", "trna_glutamine.fna")
TEXTS = {"trna-th25": "trna_glutamine.fna|dna|-th 25|trna_glutamine.fna|suite",
         "atinsert-s": "Atinsert.fna|dna|-th 18 -s|Atinsert.fna|suite",
         "ttt-th60": "TTT-small.fna|dna|-th 60|TTT-small.fna|suite"}


def cases():
    with open(os.path.join(HERE, "golden_locali.json")) as f:
        esa_calls = json.load(f)["calls"]
    for subject, alphabet, args, queriesof in esa_side.cases():
        key = "%s|%s|%s|%s" % (subject, alphabet, " ".join(args), ",".join(queriesof))
        if esa_calls[key]["exit"] != 0:          # (ends before a query is read)
            continue
        for flavour in FLAVOURS:
            if flavour == "suite" or subject in MORE_FLAVOURS:
                yield subject, alphabet, args, queriesof, flavour, key


def main(gt):
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(HERE, "golden_locali.json")) as f:
        esa_calls = json.load(f)["calls"]
    calls = {}
    with tempfile.TemporaryDirectory() as tmp:
        built = {}
        for subject, alphabet, args, queriesof, flavour, esa_key in cases():
            if (subject, flavour) not in built:
                built[subject, flavour] = os.path.join(tmp, "pck%d" % len(built))
                subprocess.run([gt, "packedindex", "mkindex", "-tis", "-ssp"] + FLAVOURS[flavour] +
                               ["-dir", "rev", "-" + alphabet, "-pl", "-indexname", built[subject, flavour],
                                "-db", os.path.join(FIXTURES, subject)], check=True, stdout=subprocess.DEVNULL)
            cmd = [gt, "dev", "idxlocali"] + args + ["-pck", built[subject, flavour], "-q"] + \
                  [os.path.join(QUERIES, t + ".queries.fna") for t in queriesof]
            run = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
            text = esa_side.compared(run.stdout)
            key = esa_key + "|" + flavour
            error = run.stderr.decode("latin-1").strip()
            md5 = hashlib.md5(text).hexdigest()
            calls[key] = {"md5": md5, "lines": text.count(b"\n"), "exit": run.returncode,
                          "error": error[error.index("error: ") + 7:] if "error: " in error else error[-300:],
                          "as_esa": md5 == esa_calls[esa_key]["md5"] and run.returncode == esa_calls[esa_key]["exit"]}
            for name, k in TEXTS.items():
                if k == key:
                    with open(os.path.join(OUT, name), "wb") as f:
                        f.write(text)
    assert all(k in calls for k in TEXTS.values())
    with open(os.path.join(HERE, "golden_pcklocali.json"), "w") as f:
        json.dump({"calls": calls, "texts": TEXTS}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%d calls, %d lines, %d end with an error, %d differ from -esa: %s" % (
        len(calls), sum(c["lines"] for c in calls.values()), sum(c["exit"] != 0 for c in calls.values()),
        sum(not c["as_esa"] for c in calls.values()), sorted(k for k, c in calls.items() if not c["as_esa"])))


if __name__ == "__main__":
    main(sys.argv[1])
