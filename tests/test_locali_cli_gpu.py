"""`gt-suffixerator-amd idxlocali` against every call of `gt dev idxlocali`
recorded in tests/golden/golden_locali.json: exit code, error text and the md5 of
the stdout in the normal form of tests/locali_golden.py; the three texts kept
whole byte for byte.  The indexes are written by this project's suffixerator
tool in the same run.  And one call that no recording has: a query of 16384
letters, the most the library takes, with a short one behind it, against the
numpy statement's text; and a query of 16385 letters, which ends the tool."""
import hashlib
import os
import subprocess

import numpy as np
import pytest

import locali_golden as lg
import locali_reference as lr
import oracle_util as ou
from genometools_amd import _lib

pytestmark = pytest.mark.gpu

CLI = os.path.join(_lib.HERE, "gt-suffixerator-amd")


@pytest.fixture(scope="module")
def indexes(gpu, tmp_path_factory):
    ou.build()
    tmp = tmp_path_factory.mktemp("locali")
    built = {}
    for key in lg.GOLDEN["calls"]:
        subject, protein, _, _ = lg.parse(key)
        if subject not in built:
            built[subject] = str(tmp / ("sfx%d" % len(built)))
            subprocess.run([CLI, "-protein" if protein else "-dna", "-tis", "-suf", "-ssp", "-indexname", built[subject],
                            "-db", ou.fixture_path(subject)], check=True, stdout=subprocess.DEVNULL)
    return built


def _run(indexes, key):
    subject, _, args, files = lg.parse(key)
    p = subprocess.run([CLI, "idxlocali"] + args + ["-esa", indexes[subject], "-q"] + files, capture_output=True)
    return p.returncode, lg.compared(p.stdout), p.stderr.decode("latin-1").strip()


@pytest.mark.parametrize("key", sorted(lg.GOLDEN["calls"]))
def test_every_recorded_call(indexes, key):
    want = lg.GOLDEN["calls"][key]
    rc, text, err = _run(indexes, key)
    assert rc == want["exit"], err
    assert (err[err.index("error: ") + 7:] if "error: " in err else "") == want["error"]
    assert text.count(b"\n") == want["lines"]
    assert hashlib.md5(text).hexdigest() == want["md5"]


@pytest.mark.parametrize("name", sorted(lg.GOLDEN["texts"]))
def test_the_texts_kept_whole(indexes, name):
    rc, text, err = _run(indexes, lg.GOLDEN["texts"][name])
    with open(os.path.join(lg.QUERYDIR, name), "rb") as f:
        assert rc == 0 and text == f.read(), err


def test_the_longest_query_through_the_tool(gpu, tmp_path):
    """two sequences of 17 and 10 letters, written here; the query of 16384
    letters over a, c, g ends with the last twelve letters of the first sequence
    and begins with its first ten.  The reference takes 8 s."""
    ou.build()
    rng = np.random.default_rng(48)
    tail = np.array([3, 0, 3, 3, 1, 3, 2, 3, 3, 0, 1, 3], dtype=np.uint8)
    first, second = np.concatenate([rng.integers(0, 3, 5, dtype=np.uint8), tail]), np.concatenate([tail[:7], [1, 3, 3]])
    enc = np.concatenate([first, [255], second]).astype(np.uint8)
    longest = rng.integers(0, 3, 16384, dtype=np.uint8)
    longest[-12:] = tail
    longest[:5] = first[:5]
    longest[5:10] = tail[:5]
    queries = [longest, tail[2:9].copy()]
    text = lambda codes: "".join("acgt"[c] for c in codes)
    (tmp_path / "subject.fna").write_text(">one\n%s\n>two\n%s\n" % (text(first), text(second)))
    (tmp_path / "queries.fna").write_text("".join(">q%d\n%s\n" % (k, text(q)) for k, q in enumerate(queries)))
    (tmp_path / "beyond.fna").write_text(">q\n%s\n" % text(rng.integers(0, 4, 16385)))
    index = str(tmp_path / "sfx")
    subprocess.run([CLI, "-dna", "-tis", "-suf", "-ssp", "-indexname", index, "-db", str(tmp_path / "subject.fna")],
                   check=True, stdout=subprocess.DEVNULL)
    call = [CLI, "idxlocali", "-th", "6", "-match", "1", "-mismatch", "-2", "-gapextend", "-2", "-esa", index, "-q"]
    p = subprocess.run(call + [str(tmp_path / "queries.fna")], capture_output=True)
    assert p.returncode == 0, p.stderr
    lines = [l for l in p.stdout.decode().splitlines(True) if not l.startswith(("# indexname", "# queryfile"))]
    want = lr.tool_stdout(enc, ou.esa(enc, 4)["suf"], queries, 6, 1, -2, -2)
    assert "".join(lines) == want and want.count("\n") > 5
    positions = [int(l.split("\t")[5]) for l in lines if l.split("\t")[4:5] == ["0"]]         # qstart of query 0
    assert max(positions) > 16000 and min(positions) < 16
    p = subprocess.run(call + [str(tmp_path / "beyond.fna")], capture_output=True)
    assert p.returncode != 0
    assert b"query number 0 of length 16385; queries must not be longer than 16384" in p.stderr
