"""Regenerate tests/golden/golden_esq_edges.json with the reference's encoder:

    python tests/golden/make_golden_esq_edges.py

It needs oracle/_ref/gt_ref_sfx (the reference's own sources, compiled by
oracle/Makefile.ref).  The inputs are made here, by tests/esq_edge_cases.py:
GOLDEN_CASES names the cases -- special runs of 65535, 65536 and 65537, inputs of
32, 64, 4096 and 4097 symbols, wildcards at both ends, wildcard and separator on
every third position, an equal-length set, three run ends on one tile border --
and fasta_bytes() writes each as FASTA of 70 columns with one description per
sequence.  Per case the reference runs once with every `-sat` it takes for that
input (direct, bit, uchar, ushort, uint32 for DNA, eqlen where all sequences are
equally long and without wildcard; direct and bytecompress for protein), from the
input's directory, so that INDEX.esq stores the bare file name.  Recorded: the
md5 of the input, and per access type md5 and size of INDEX.esq and INDEX.ssp
and the text of INDEX.prj.  No file of the reference's is kept."""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
import esq_edge_cases as ec  # noqa: E402
import esq_sections_reference as ref  # noqa: E402

BIN = os.path.join(ROOT, "oracle", "_ref", "gt_ref_sfx")


def md5(path):
    with open(path, "rb") as f:
        return hashlib.md5(f.read()).hexdigest()


def main():
    if not os.path.exists(BIN):
        sys.exit("build oracle/_ref first: make -f oracle/Makefile.ref")
    golden = {}
    for name in ec.GOLDEN_CASES:
        case = ec.by_name(name)
        assert ref.first_empty_sequence(case.enc) is None, name
        equal = ref._expected_summary(case.enc, case.sigma)["equallength"]
        with tempfile.TemporaryDirectory() as tmp:
            src = os.path.join(tmp, ec.fasta_name(case))
            with open(src, "wb") as f:
                f.write(ec.fasta_bytes(case))
            entry = {"input_md5": md5(src), "input_bytes": os.path.getsize(src),
                     "totallength": int(case.enc.size), "sat": {}}
            for sat in ec.legal_access_types(case, equal):
                idx = os.path.join(tmp, "idx-" + sat)
                subprocess.run([BIN, "-protein" if case.alphabet == "protein" else "-dna",
                                "-sat", sat, "-indexname", idx, "-db", os.path.basename(src)],
                               check=True, cwd=tmp, stdout=subprocess.DEVNULL)
                rec = {ext: {"md5": md5(idx + "." + ext), "bytes": os.path.getsize(idx + "." + ext)}
                       for ext in ("esq", "ssp") if os.path.exists(idx + "." + ext)}
                with open(idx + ".prj") as f:
                    rec["prj"] = f.read()
                entry["sat"][sat] = rec
        golden[name] = entry
        print(name, entry["totallength"], " ".join(sorted(entry["sat"])))
    with open(os.path.join(HERE, "golden_esq_edges.json"), "w") as f:
        json.dump(golden, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
