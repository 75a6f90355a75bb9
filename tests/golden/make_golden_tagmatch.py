"""Regenerate tests/golden/golden_tagmatch.json and tests/golden/tagmatch/ with
a GenomeTools binary:

    python tests/golden/make_golden_tagmatch.py /path/to/bin/gt

Tag files come from a seeded generator and are committed under
tests/golden/tagmatch/ (NAME.tags.fna): per fixture, substrings of 12 to 15 and
of 30 to 64 letters cut from it (where it has the fewest wildcards; a wildcard
inside is replaced by a random letter), four of 3 to 8 letters (the fixtures
made of a, c and n have no longer run of letters), copies of these with 1 to 3 random replacements, insertions and
deletions, some of them reverse-complemented, some purely random tags, one tag
of 64 letters and, as the LAST one, a tag of one letter: with -e 1 and more the
reference ends at it with an error, after the blocks of all tags before it.

For each of six DNA fixtures, index `gt suffixerator -dna -tis -suf -ssp`:
`gt tagerator -esa INDEX -q TAGS` with -e 0, -e 1, -e 2, -e 2 -best, -e 1 -nod,
-e 1 -nop; on RandomN and Atinsert also -e 2 -withwildcards and -e 2
-withwildcards no (the option is a switch whose value the tool stores as "no
wildcards": only `no` lets wildcards pass, src/tools/gt_tagerator.c:170-174);
once every -output keyword, once without tagnum and dblength, once two tag
files; sw100K1.fsa as protein with -nop.  Kept per call: the exit code, and md5
and line count of the stdout with the `# indexname` and `# queryfile` lines
dropped (they hold paths) and the match lines SORTED inside each tag's block
(their order is the reference's stack order, a by-product).  Three small outputs
lie whole under tests/golden/tagmatch/."""
import hashlib
import json
import os
import random
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURES = os.path.join(HERE, "fixtures")
OUT = os.path.join(HERE, "tagmatch")
DNA = ("Atinsert.fna", "Duplicate.fna", "Random.fna", "RandomN.fna", "TTT-small.fna", "trna_glutamine.fna")
PROTEIN = "sw100K1.fsa"
PROTEIN_LETTERS = "LVIFKREDAGSTNQYWPHMC"
CALLS = (["-e", "0"], ["-e", "1"], ["-e", "2"], ["-e", "2", "-best"], ["-e", "1", "-nod"], ["-e", "1", "-nop"])
WILD = (["-e", "2", "-withwildcards"], ["-e", "2", "-withwildcards", "no"])
EVERY = ["-e", "1", "-output", "tagnum", "tagseq", "dblength", "dbstartpos", "abspos", "dbsequence", "strand", "edist"]
FEW = ["-e", "1", "-output", "tagseq", "dbstartpos", "strand", "edist"]
TEXTS = {"trna-e1": "trna_glutamine.fna|dna|-e 1|trna_glutamine.fna",
         "duplicate-e0": "Duplicate.fna|dna|-e 0|Duplicate.fna",
         "ttt-best": "TTT-small.fna|dna|-e 2 -best|TTT-small.fna"}


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


def make_tags(name, protein, rng):
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

    def edited(tag):
        tag = list(tag)
        for _ in range(rng.randint(1, 3)):
            at, what = rng.randrange(len(tag)), rng.randrange(3)
            if what == 0:
                tag[at] = rng.choice(letters)
            elif what == 1:
                tag.insert(at, rng.choice(letters))
            elif len(tag) > 4:
                del tag[at]
        return "".join(tag)[:64]

    def rc(tag):
        return "".join("acgt"[3 - "acgt".index(c)] for c in reversed(tag))

    short = [cut(12, 15) for _ in range(6)]
    long = [cut(30, 64) for _ in range(4)]
    tags = short + long + [edited(t) for t in short[:3] + long[:3]] + [cut(3, 8) for _ in range(4)]
    if not protein:
        tags += [rc(t) for t in (short[3], long[3], edited(short[4]))]
    tags += ["".join(rng.choice(letters) for _ in range(rng.randint(12, 20))) for _ in range(3)]
    tags.append((cut(40, 64) + "".join(rng.choice(letters) for _ in range(64)))[:64])
    tags.append(rng.choice(letters))
    return tags


def compared(raw):
    lines = [l for l in raw.decode("latin-1").splitlines()
             if not l.startswith("# indexname") and not l.startswith("# queryfile")]
    out, block = [], []
    for line in lines + ["#"]:
        if line.startswith("#"):
            out.extend(sorted(block))
            block = []
            out.append(line)
        else:
            block.append(line)
    return "".join(l + "\n" for l in out[:-1]).encode("latin-1")


def cases():
    for name in DNA:
        for args in CALLS:
            yield name, "dna", args, (name,)
        if name in ("RandomN.fna", "Atinsert.fna"):
            for args in WILD:
                yield name, "dna", args, (name,)
    yield "Duplicate.fna", "dna", EVERY, ("Duplicate.fna",)
    yield "Atinsert.fna", "dna", FEW, ("Atinsert.fna",)
    yield "Duplicate.fna", "dna", ["-e", "0"], ("trna_glutamine.fna", "Duplicate.fna")
    for k in ("0", "1"):
        yield PROTEIN, "protein", ["-e", k, "-nop"], (PROTEIN,)


def main(gt):
    os.makedirs(OUT, exist_ok=True)
    rng = random.Random(20261018)
    for name in DNA + (PROTEIN,):
        with open(os.path.join(OUT, name + ".tags.fna"), "w") as f:
            for tag in make_tags(name, name == PROTEIN, rng):
                f.write(">\n%s\n" % tag)
    calls = {}
    with tempfile.TemporaryDirectory() as tmp:
        built = {}
        for subject, alphabet, args, tagsof in cases():
            if subject not in built:
                built[subject] = os.path.join(tmp, "sfx%d" % len(built))
                subprocess.run([gt, "suffixerator", "-" + alphabet, "-tis", "-suf", "-ssp", "-indexname",
                                built[subject], "-db", os.path.join(FIXTURES, subject)], check=True,
                               stdout=subprocess.DEVNULL)
            cmd = [gt, "tagerator"] + args + ["-esa", built[subject], "-q"] + \
                  [os.path.join(OUT, t + ".tags.fna") for t in tagsof]
            run = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
            text = compared(run.stdout)
            key = "%s|%s|%s|%s" % (subject, alphabet, " ".join(args), ",".join(tagsof))
            error = run.stderr.decode("latin-1").strip()
            calls[key] = {"md5": hashlib.md5(text).hexdigest(), "lines": text.count(b"\n"), "exit": run.returncode,
                          "error": error[error.index("error: ") + 7:] if "error: " in error else ""}
            for name, k in TEXTS.items():
                if k == key:
                    with open(os.path.join(OUT, name), "wb") as f:
                        f.write(text)
    assert all(k in calls for k in TEXTS.values())
    with open(os.path.join(HERE, "golden_tagmatch.json"), "w") as f:
        json.dump({"calls": calls, "texts": TEXTS}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%d calls, %d lines, %d end with an error" % (len(calls), sum(c["lines"] for c in calls.values()),
                                                        sum(c["exit"] != 0 for c in calls.values())))


if __name__ == "__main__":
    main(sys.argv[1])
