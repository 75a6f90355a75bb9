"""What the two tests of the recorded reference calls share
(tests/golden/golden_locali.json, written by tests/golden/make_golden_locali.py):
the calls, the query files, and the normal form in which outputs are compared --
the two path lines dropped, the match blocks of one query sorted."""
import json
import os
import re

import numpy as np

import oracle_util as ou

QUERYDIR = os.path.join(ou.GOLDEN_DIR, "locali")
PROTEIN_LETTERS = "LVIFKREDAGSTNQYWPHMC"
MATCH_LINE = re.compile(r"^\d+\t\d+\t\d+\t\t\d+\t\d+\t\d+\t\d+$")

with open(os.path.join(ou.GOLDEN_DIR, "golden_locali.json")) as _f:
    GOLDEN = json.load(_f)


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


def parse(key):
    """(subject, protein?, the tool's arguments, the query file paths) of a recorded call"""
    subject, alphabet, args, files = key.split("|")
    return subject, alphabet == "protein", args.split(), [os.path.join(QUERYDIR, f + ".queries.fna")
                                                          for f in files.split(",")]


def options(args):
    """(T, match, mismatch, gapextend, -s?) of the arguments of a call that runs"""
    value = {"-th": None, "-match": 1, "-mismatch": -3, "-gapstart": -5, "-gapextend": -2}
    for k, a in enumerate(args):
        if a in value:
            value[a] = int(args[k + 1])
    return value["-th"], value["-match"], value["-mismatch"], value["-gapextend"], "-s" in args


def read_queries(paths, protein):
    letters = PROTEIN_LETTERS if protein else "acgt"
    code = {c: k for k, c in enumerate(letters)}
    queries = []
    for path in paths:
        with open(path) as f:
            for line in f:
                if not line.startswith(">"):
                    queries.append(np.array([code.get(c, 254) for c in line.strip()], dtype=np.uint8))
    return queries
