"""Regenerate tests/golden/golden_qmatch.json and tests/golden/qmatch/ with a
GenomeTools binary:

    python tests/golden/make_golden_qmatch.py /path/to/bin/gt

For each of five DNA subjects with two other fixtures as query, index `gt
suffixerator -dna -suf -lcp -tis -ssp`: `gt repfind -l 8 -q Q`, `-l 14 -q Q`,
`-l 8 -r -q Q`, `-l 8 -p -q Q` and `-l 8 -f -r -p -q Q`; for each of the same
subjects without a query `-l 8 -r` and `-l 8 -p`; once two query files
(`-l 8 -p`, the only reverse-complement call of these fixtures with more than
100 lines); and sw100K1.fsa as protein against sw100K2.fsa at -l 6, forward
and reverse -- where the two share nothing -- and at -l 4.  Kept
per call: md5 and line count of the stdout, its lines starting with `#`
dropped, runs of white space made one blank, each line ended by a newline, the
ORDER AS PRINTED (it is part of the semantics: include/gtamd_qmatch.h).  Three
small outputs, one per mode, lie whole under tests/golden/qmatch/; so does the
result the reference itself records for `-l 8 -r -ii Duplicate.fna`
(testdata/repfind-result/Duplicate.fna-r.result, under tests/golden/repfind/)."""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURES = os.path.join(HERE, "fixtures")
SUBJECTS = {"Atinsert.fna": ("Atinsert_seqrange_3-7.fna", "Random.fna"),
            "Duplicate.fna": ("Atinsert.fna", "RandomN.fna"),
            "Random.fna": ("RandomN.fna", "Atinsert.fna"),
            "RandomN.fna": ("Random.fna", "trna_glutamine.fna"),
            "trna_glutamine.fna": ("Atinsert.fna", "Random159.fna")}
WITH_QUERY = (["-l", "8"], ["-l", "14"], ["-l", "8", "-r"], ["-l", "8", "-p"], ["-l", "8", "-f", "-r", "-p"])
SELF = (["-l", "8", "-r"], ["-l", "8", "-p"])
TEXTS = {"duplicate-atinsert-f": "Duplicate.fna|dna|-l 8|Atinsert.fna",
         "duplicate-atinsert-r": "Duplicate.fna|dna|-l 8 -r|Atinsert.fna",
         "trna-atinsert-p": "trna_glutamine.fna|dna|-l 8 -p|Atinsert.fna"}


def cases():
    for subject, queries in SUBJECTS.items():
        for q in queries:
            for args in WITH_QUERY:
                yield subject, "dna", args, (q,)
        for args in SELF:
            yield subject, "dna", args, ()
    yield "Atinsert.fna", "dna", ["-l", "8", "-p"], ("Duplicate.fna", "Atinsert_seqrange_3-7.fna")
    for minlen in ("6", "4"):
        yield "sw100K1.fsa", "protein", ["-l", minlen], ("sw100K2.fsa",)
        yield "sw100K1.fsa", "protein", ["-l", minlen, "-r"], ("sw100K2.fsa",)


def compared(raw):
    lines = [" ".join(l.split()) for l in raw.decode("latin-1").splitlines() if l.strip() and not l.startswith("#")]
    return "".join(l + "\n" for l in lines).encode("latin-1")


def main(gt):
    calls, most = {}, {}
    os.makedirs(os.path.join(HERE, "qmatch"), exist_ok=True)
    with tempfile.TemporaryDirectory() as tmp:
        built = {}
        for subject, alphabet, args, queries in cases():
            if subject not in built:
                built[subject] = os.path.join(tmp, "sfx%d" % len(built))
                subprocess.run([gt, "suffixerator", "-" + alphabet, "-suf", "-lcp", "-tis", "-ssp", "-indexname",
                                built[subject], "-db", os.path.join(FIXTURES, subject)], check=True,
                               stdout=subprocess.DEVNULL)
            cmd = [gt, "repfind"] + args + (["-q"] + [os.path.join(FIXTURES, q) for q in queries] if queries else [])
            text = compared(subprocess.run(cmd + ["-ii", built[subject]], check=True, stdout=subprocess.PIPE).stdout)
            key = "%s|%s|%s|%s" % (subject, alphabet, " ".join(args), ",".join(queries))
            calls[key] = {"md5": hashlib.md5(text).hexdigest(), "lines": text.count(b"\n")}
            for name, k in TEXTS.items():
                if k == key:
                    with open(os.path.join(HERE, "qmatch", name), "wb") as f:
                        f.write(text)
            for letter in b"FRP":               # the lines of one mode in this call
                kind = "protein" if alphabet == "protein" else ("" if queries else "self-") + chr(letter)
                count = sum(l.split()[3] == bytes([letter]) for l in text.splitlines())
                most[kind] = max(most.get(kind, 0), count)
    # every mode has a call with more than 100 of its lines, and one call has none
    assert all(most.get(k, 0) > 100 for k in ("F", "R", "P", "self-R", "self-P", "protein")), most
    assert any(c["lines"] == 0 for c in calls.values())
    assert all(calls[k]["lines"] > 0 for k in TEXTS.values())
    with open(os.path.join(HERE, "golden_qmatch.json"), "w") as f:
        json.dump({"calls": calls, "texts": TEXTS}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%d calls, %d lines" % (len(calls), sum(c["lines"] for c in calls.values())))


if __name__ == "__main__":
    main(sys.argv[1])
