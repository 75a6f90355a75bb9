#!/usr/bin/env python3
"""Generate tests/golden/golden_sain.json from the REFERENCE itself.

For every stored suffixerator fixture of golden.json this runs
oracle/_ref/gt_ref_sfx -sain -- the reference's other construction, SA-IS
(gt_sain_encseq_sortsuffixes, src/match/sfx-sain.c:1577) + the Phi algorithm
(gt_plain_lcp_phialgorithm, src/match/sfx-linlcp.c:131), `-sain` of
oracle/ref_driver.c -- with `-suf -lcp -bwt` and stores md5 + size of every
table, so that tests/test_oracle_golden.py can hold both constructions of the
reference against each other and against the CPU restatement on machines where
oracle/_ref cannot be built.  Only expected outputs are stored.
"""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import oracle_util as ou  # noqa: E402

OUT = os.path.join(ou.GOLDEN_DIR, "golden_sain.json")


def main():
    if not os.path.exists(ou.REF_BIN):
        sys.exit("build oracle/_ref first: make -f oracle/Makefile.ref")
    golden = ou.golden()
    sain = {}
    for name in sorted(k for k in golden if golden[k]["fixture"]):
        with tempfile.TemporaryDirectory() as tmp:
            idx = os.path.join(tmp, "s")
            subprocess.run([ou.REF_BIN, "-" + golden[name]["alphabet"], "-sain", "-suf", "-lcp",
                            "-bwt", "-db", ou.fixture_path(name), "-indexname", idx], check=True)
            tables = {}
            for ext in ("suf", "lcp", "llv", "bwt"):
                with open(idx + "." + ext, "rb") as f:
                    raw = f.read()
                tables[ext] = {"bytes": len(raw), "md5": hashlib.md5(raw).hexdigest()}
        sain[name] = {"alphabet": golden[name]["alphabet"], "tables": tables}
    with open(OUT, "w") as f:
        json.dump(sain, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%d fixtures -> %s" % (len(sain), OUT))


if __name__ == "__main__":
    main()
