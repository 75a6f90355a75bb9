"""Regenerate tests/golden/golden_locali.json and tests/golden/locali/ with a
GenomeTools binary:

    python tests/golden/make_golden_locali.py /path/to/bin/gt

Query files come from a seeded generator and are committed under
tests/golden/locali/ (NAME.queries.fna): per fixture, four pieces of 20 to 300
letters cut from it, copies of three of them with replacements, insertions and
deletions, one piece with a wildcard put in, one random query and one of a
single letter.

For each of six DNA fixtures, index `gt suffixerator -dna -tis -suf -ssp`:
`gt dev idxlocali -esa INDEX -q QUERIES` with -th at a low, a middle and a high
value (chosen so that no call prints more than some 50 k lines), once with
-match 2 -mismatch -1 -gapextend -1, once with -gapstart given (it changes
nothing: the same threshold as a call without it), once with -s, once with two
query files; sw100K1.fsa as protein; and the calls that end with an error
before a query is read.  Kept per call: the exit code, the error text, the
seconds the reference took on one core, and md5 and line count of the stdout
with the `# indexname` and `# queryfile` lines dropped (they hold paths) and the
match blocks -- a match line with the alignment lines behind it -- SORTED inside
each query (their order is the reference's stack order, a by-product).  Three
small outputs lie whole under tests/golden/locali/."""
import hashlib
import json
import os
import random
import re
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURES = os.path.join(HERE, "fixtures")
OUT = os.path.join(HERE, "locali")
DNA = ("Atinsert.fna", "Duplicate.fna", "Random.fna", "RandomN.fna", "TTT-small.fna", "trna_glutamine.fna")
PROTEIN = "sw100K1.fsa"
PROTEIN_LETTERS = "LVIFKREDAGSTNQYWPHMC"
LOW, MIDDLE, HIGH = "14", "25", "60"
TEXTS = {"trna-th25": "trna_glutamine.fna|dna|-th 25|trna_glutamine.fna",
         "atinsert-s": "Atinsert.fna|dna|-th 18 -s|Atinsert.fna",
         "ttt-th60": "TTT-small.fna|dna|-th 60|TTT-small.fna"}
MATCH_LINE = re.compile(r"^\d+\t\d+\t\d+\t\t\d+\t\d+\t\d+\t\d+$")


def sequences(path):
    out, cur = [], None
    with open(path) as f:
        for line in f:
            if line.startswith(">"):
                if cur:
                    out.append(cur)
                cur = ""
            elif cur is not None:
                cur += "".join(line.split())
    if cur:
        out.append(cur)
    return out


def make_queries(name, protein, rng):
    letters = PROTEIN_LETTERS if protein else "acgt"
    seqs = [s.upper() if protein else s.lower() for s in sequences(os.path.join(FIXTURES, name))]

    def cut(lo, hi):
        best = None                       # of 200 windows the one with the fewest wildcards
        for _ in range(200):
            s = rng.choice(seqs)
            want = rng.randint(lo, hi)
            if len(s) >= want:
                at = rng.randrange(len(s) - want + 1)
                bad = sum(c not in letters for c in s[at:at + want])
                if best is None or bad < best[0]:
                    best = (bad, s[at:at + want])
        if best is None:
            return "".join(rng.choice(letters) for _ in range(rng.randint(lo, hi)))
        return "".join(c if c in letters else rng.choice(letters) for c in best[1])

    def edited(query):
        query = list(query)
        for _ in range(rng.randint(2, 6)):
            at, what = rng.randrange(len(query)), rng.randrange(3)
            if what == 0:
                query[at] = rng.choice(letters)
            elif what == 1:
                query.insert(at, rng.choice(letters))
            elif len(query) > 4:
                del query[at]
        return "".join(query)

    pieces = [cut(20, 40), cut(60, 120), cut(150, 300), cut(30, 80)]
    wild = list(cut(40, 70))
    wild[len(wild) // 2] = "X" if protein else "n"
    queries = pieces + [edited(q) for q in pieces[:3]] + ["".join(wild)]
    queries.append("".join(rng.choice(letters) for _ in range(rng.randint(30, 60))))
    queries.append(rng.choice(letters))
    return queries


def compared(raw):
    lines = [l for l in raw.decode("latin-1").splitlines()
             if not l.startswith("# indexname") and not l.startswith("# queryfile")]
    out, blocks = [], []
    for line in lines + ["#"]:
        if line.startswith("#") or line.startswith("process sequence "):
            for block in sorted(blocks):
                out.extend(block)
            blocks = []
            out.append(line)
        elif MATCH_LINE.match(line) or not blocks:
            blocks.append([line])
        else:
            blocks[-1].append(line)
    return "".join(l + "\n" for l in out[:-1]).encode("latin-1")


def cases():
    for name in DNA:
        for th in (LOW, MIDDLE, HIGH):
            yield name, "dna", ["-th", th], (name,)
        yield name, "dna", ["-th", "30", "-match", "2", "-mismatch", "-1", "-gapextend", "-1"], (name,)
    yield "Atinsert.fna", "dna", ["-th", MIDDLE, "-gapstart", "-1"], ("Atinsert.fna",)
    yield "Random.fna", "dna", ["-th", LOW, "-gapstart", "-20"], ("Random.fna",)
    yield "Atinsert.fna", "dna", ["-th", "18", "-s"], ("Atinsert.fna",)
    yield "Duplicate.fna", "dna", ["-th", "50", "-s", "-match", "2", "-mismatch", "-2", "-gapextend", "-1"], ("Duplicate.fna",)
    yield "Duplicate.fna", "dna", ["-th", MIDDLE], ("trna_glutamine.fna", "Duplicate.fna")
    for th in ("8", "20"):
        yield PROTEIN, "protein", ["-th", th], (PROTEIN,)
    yield "Atinsert.fna", "dna", ["-th", "0"], ("Atinsert.fna",)
    yield "Atinsert.fna", "dna", [], ("Atinsert.fna",)
    yield "Atinsert.fna", "dna", ["-th", "-3"], ("Atinsert.fna",)
    yield "Atinsert.fna", "dna", ["-th", "x"], ("Atinsert.fna",)


def main(gt):
    os.makedirs(OUT, exist_ok=True)
    rng = random.Random(20261018)
    for name in DNA + (PROTEIN,):
        with open(os.path.join(OUT, name + ".queries.fna"), "w") as f:
            for query in make_queries(name, name == PROTEIN, rng):
                f.write(">\n%s\n" % query)
    calls = {}
    with tempfile.TemporaryDirectory() as tmp:
        built = {}
        for subject, alphabet, args, queriesof in cases():
            if subject not in built:
                built[subject] = os.path.join(tmp, "sfx%d" % len(built))
                subprocess.run([gt, "suffixerator", "-" + alphabet, "-tis", "-suf", "-ssp", "-indexname",
                                built[subject], "-db", os.path.join(FIXTURES, subject)], check=True,
                               stdout=subprocess.DEVNULL)
            cmd = [gt, "dev", "idxlocali"] + args + ["-esa", built[subject], "-q"] + \
                  [os.path.join(OUT, t + ".queries.fna") for t in queriesof]
            start = time.time()
            run = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
            seconds = time.time() - start
            text = compared(run.stdout)
            key = "%s|%s|%s|%s" % (subject, alphabet, " ".join(args), ",".join(queriesof))
            error = run.stderr.decode("latin-1").strip()
            calls[key] = {"md5": hashlib.md5(text).hexdigest(), "lines": text.count(b"\n"), "exit": run.returncode,
                          "error": error[error.index("error: ") + 7:] if "error: " in error else "",
                          "reference_seconds": round(seconds, 3)}
            for name, k in TEXTS.items():
                if k == key:
                    with open(os.path.join(OUT, name), "wb") as f:
                        f.write(text)
    assert all(k in calls for k in TEXTS.values())
    with open(os.path.join(HERE, "golden_locali.json"), "w") as f:
        json.dump({"calls": calls, "texts": TEXTS}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%d calls, %d lines, %d end with an error" % (len(calls), sum(c["lines"] for c in calls.values()),
                                                        sum(c["exit"] != 0 for c in calls.values())))


if __name__ == "__main__":
    main(sys.argv[1])
