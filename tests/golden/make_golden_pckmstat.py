"""Regenerate tests/golden/golden_pckmstat.json and the text fixtures under
tests/golden/pckmstat/ with a GenomeTools binary:

    python tests/golden/make_golden_pckmstat.py /path/to/bin/gt

`gt matstat -pck` and `gt uniquesub -pck` as the reference's suite runs them
(testsuite/gt_idxsearch_include.rb:13-33, 62-72): for all 72 ordered pairs
subject != query of its nine DNA fixtures and for one protein pair, the index is
`gt packedindex mkindex -tis -ssp -sprank -bsize 10 -locfreq 32 -dir rev` with
`-dna -pl` or `-protein`.  For three subjects the index is built in four more
flavours: the defaults, -locbitmap, -locfreq 0 and -dir fwd (nothing may
special-case the read mode).  Recorded: md5 and line count of the stdout of
matstat and uniquesub with every output flag and -min 1 and of the suite's own
call (-output querypos -min 1 -max 20); for -locfreq 0, which has no positions,
the querypos-only calls.  Three outputs are kept whole."""
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
SUITE = ["-sprank", "-bsize", "10", "-locfreq", "32", "-dir", "rev"]
FLAVOURS = {"suite": SUITE, "defaults": ["-dir", "rev"], "locbitmap": ["-locbitmap", "-dir", "rev"],
            "locfreq0": ["-locfreq", "0", "-dir", "rev"],
            "fwd": ["-sprank", "-bsize", "10", "-locfreq", "32", "-dir", "fwd"]}
MORE_SUBJECTS = ["Atinsert.fna", "RandomN.fna", "trna_glutamine.fna"]
CALLS = {
    "matstat": ["matstat", "-output", "querypos", "subjectpos", "sequence", "-min", "1"],
    "uniquesub": ["uniquesub", "-output", "querypos", "sequence", "-min", "1"],
    "matstat_max20": ["matstat", "-output", "querypos", "-min", "1", "-max", "20"],
    "uniquesub_max20": ["uniquesub", "-output", "querypos", "-min", "1", "-max", "20"],
}
WITHOUT_POSITIONS = ("matstat_max20", "uniquesub_max20")
# (flavour, subject, query, call) -> file under tests/golden/pckmstat/
TEXTS = {("suite", "Duplicate.fna", "trna_glutamine.fna", "matstat"): "dna_matstat.txt",
         ("locbitmap", "Atinsert.fna", "trna_glutamine.fna", "uniquesub"): "dna_uniquesub_locbitmap.txt",
         ("fwd", "Atinsert.fna", "Random160.fna", "matstat"): "dna_matstat_fwd.txt"}


def main(gt):
    out = {"dna": {}, "protein": {}, "texts": {}}
    os.makedirs(os.path.join(HERE, "pckmstat"), exist_ok=True)
    with tempfile.TemporaryDirectory() as tmp:
        def pairs(kind, alphabet, flavour, wanted):
            for subject in sorted({s for s, _ in wanted}):
                idx = os.path.join(tmp, "pck")
                subprocess.run([gt, "packedindex", "mkindex", "-tis", "-ssp"] + FLAVOURS[flavour] + alphabet +
                               ["-indexname", idx, "-db", os.path.join(FIXTURES, subject)], check=True,
                               stdout=subprocess.DEVNULL)
                for query in [q for s, q in wanted if s == subject]:
                    entry = {}
                    for call, args in CALLS.items():
                        if flavour == "locfreq0" and call not in WITHOUT_POSITIONS:
                            continue
                        raw = subprocess.run([gt] + args + ["-pck", idx, "-query", os.path.join(FIXTURES, query)],
                                             check=True, stdout=subprocess.PIPE).stdout
                        entry[call] = {"md5": hashlib.md5(raw).hexdigest(), "lines": raw.count(b"\n")}
                        name = TEXTS.get((flavour, subject, query, call))
                        if name is not None:
                            with open(os.path.join(HERE, "pckmstat", name), "wb") as f:
                                f.write(raw)
                            out["texts"][name] = {"flavour": flavour, "subject": subject, "query": query,
                                                  "call": call, "alphabet": kind}
                    out[kind]["%s|%s|%s" % (flavour, subject, query)] = entry
        pairs("dna", ["-dna", "-pl"], "suite", [(s, q) for s in DNA for q in DNA if s != q])
        for flavour in ("defaults", "locbitmap", "locfreq0", "fwd"):
            pairs("dna", ["-dna", "-pl"], flavour, [(s, q) for s in MORE_SUBJECTS for q in DNA if s != q])
        pairs("protein", ["-protein"], "suite", [PROTEIN])
    out["calls"] = {k: v[1:] for k, v in CALLS.items()}
    out["flavours"] = FLAVOURS
    with open(os.path.join(HERE, "golden_pckmstat.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%d DNA entries, %d protein pairs, %d texts" % (len(out["dna"]), len(out["protein"]), len(out["texts"])))


if __name__ == "__main__":
    main(sys.argv[1])
