"""Regenerate tests/golden/golden_mstat.json and the text fixtures under
tests/golden/mstat/ with a GenomeTools binary:

    python tests/golden/make_golden_mstat.py /path/to/bin/gt

For all 72 ordered pairs subject != query of the nine fixtures the reference's
suite searches (testsuite/gt_idxsearch_include.rb, createandcheckgreedyfwdmat),
with the index `gt suffixerator -tis -suf -ssp -dna`: md5 and line count of the
stdout of `gt matstat` and `gt uniquesub` with every output flag and -min 1,
and of the suite's own call (-output querypos -min 1 -max 20); the same for one
protein pair.  Three outputs are kept whole."""
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
PROTEIN = ("sw100K1.fsa", "sw100K2.fsa")
CALLS = {
    "matstat": ["matstat", "-output", "querypos", "subjectpos", "sequence", "-min", "1"],
    "uniquesub": ["uniquesub", "-output", "querypos", "sequence", "-min", "1"],
    "matstat_max20": ["matstat", "-output", "querypos", "-min", "1", "-max", "20"],
    "uniquesub_max20": ["uniquesub", "-output", "querypos", "-min", "1", "-max", "20"],
}
# (subject, query, call) -> file under tests/golden/mstat/
TEXTS = {("Duplicate.fna", "trna_glutamine.fna", "matstat"): "dna_matstat.txt",
         ("Random160.fna", "Random159.fna", "uniquesub"): "dna_uniquesub.txt",
         ("sw100K1.fsa", "sw100K2.fsa", "matstat_max20"): "protein_matstat_max20.txt"}


def main(gt):
    out = {"dna": {}, "protein": {}, "texts": {}}
    os.makedirs(os.path.join(HERE, "mstat"), exist_ok=True)
    with tempfile.TemporaryDirectory() as tmp:
        def pairs(kind, flag, wanted):
            for subject in sorted({s for s, _ in wanted}):
                idx = os.path.join(tmp, "sfx")
                subprocess.run([gt, "suffixerator", "-tis", "-suf", "-ssp", flag, "-indexname", idx,
                                "-db", os.path.join(FIXTURES, subject)], check=True,
                               stdout=subprocess.DEVNULL)
                for query in [q for s, q in wanted if s == subject]:
                    entry = {}
                    for call, args in CALLS.items():
                        raw = subprocess.run([gt] + args + ["-esa", idx, "-query",
                                                            os.path.join(FIXTURES, query)],
                                             check=True, stdout=subprocess.PIPE).stdout
                        entry[call] = {"md5": hashlib.md5(raw).hexdigest(), "lines": raw.count(b"\n")}
                        name = TEXTS.get((subject, query, call))
                        if name is not None:
                            with open(os.path.join(HERE, "mstat", name), "wb") as f:
                                f.write(raw)
                            out["texts"][name] = {"subject": subject, "query": query, "call": call,
                                                  "alphabet": kind}
                    out[kind]["%s|%s" % (subject, query)] = entry
        pairs("dna", "-dna", [(s, q) for s in DNA for q in DNA if s != q])
        pairs("protein", "-protein", [PROTEIN])
    out["calls"] = {k: v[1:] for k, v in CALLS.items()}
    with open(os.path.join(HERE, "golden_mstat.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%d DNA pairs, %d protein pairs, %d texts" % (len(out["dna"]), len(out["protein"]),
                                                         len(out["texts"])))


if __name__ == "__main__":
    main(sys.argv[1])
