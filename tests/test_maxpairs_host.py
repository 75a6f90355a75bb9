"""The brute force of tests/maxpairs_reference.py against what the reference
prints: the two results it records itself (tests/golden/repfind/) and every
call of tests/golden/golden_repfind.json.  No GPU, no table: this pins the
semantics include/gtamd_maxpairs.h states before any kernel is compared with
the brute force."""
import hashlib
import json
import os

import numpy as np
import pytest

import maxpairs_reference as mp
import oracle_util as ou

REPFIND_DIR = os.path.join(ou.GOLDEN_DIR, "repfind")
with open(os.path.join(ou.GOLDEN_DIR, "golden_repfind.json")) as _f:
    GOLDEN = json.load(_f)
RECORDED = {"Duplicate.fna.result": ("Duplicate.fna", 8, 29), "Atinsert-8-8": ("Atinsert.fna", 8, 452)}


@pytest.mark.parametrize("result", sorted(RECORDED))
def test_recorded_results(result):
    name, minlen, count = RECORDED[result]
    with open(os.path.join(REPFIND_DIR, result), "rb") as f:
        want = mp.normalised(f.read())
    enc = mp.encoded(name)
    got = sorted(mp.format_lines(mp.brute_force(enc, minlen), enc))
    assert len(want) == count and got == want


@pytest.mark.parametrize("call", sorted(GOLDEN))
def test_golden_calls(call):
    name, alphabet, minlen = call.split("|")
    enc = mp.encoded(name, alphabet == "protein")
    lines = sorted(mp.format_lines(mp.brute_force(enc, int(minlen)), enc))
    text = "".join(l + "\n" for l in lines).encode("latin-1")
    assert (hashlib.md5(text).hexdigest(), len(lines)) == (GOLDEN[call]["md5"], GOLDEN[call]["lines"])


def test_golden_covers_the_issue():
    assert len(GOLDEN) == 9 * 3 + 2
    assert sum(e["lines"] > 0 for e in GOLDEN.values()) >= 5      # (not a table of empty outputs)


def test_definition_on_a_small_text():
    """every property of the definition, checked pair by pair on a text with
    wildcards and separators; and every pair of positions that has them is listed"""
    rng = np.random.default_rng(5)
    enc = rng.integers(0, 2, 300, dtype=np.uint8)
    enc[[40, 41, 170]] = 254
    enc[[99, 250]] = 255
    n, L = enc.size, 3
    rec = mp.brute_force(enc, L)
    listed = {tuple(r) for r in rec.tolist()}
    assert len(listed) == rec.shape[0]

    def sym(p):
        return int(enc[p]) if 0 <= p < n and enc[p] < 254 else None

    want = set()
    for p in range(n):
        for q in range(p + 1, n):
            if sym(p - 1) is not None and sym(p - 1) == sym(q - 1):
                continue
            ln = 0
            while sym(p + ln) is not None and sym(p + ln) == sym(q + ln):
                ln += 1
            if ln >= L:
                want.add((p, q, ln))
    assert listed == want
