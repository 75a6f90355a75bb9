"""`gt-suffixerator-amd idxlocali` against every call of `gt dev idxlocali`
recorded in tests/golden/golden_locali.json: exit code, error text and the md5 of
the stdout in the normal form of tests/locali_golden.py; the three texts kept
whole byte for byte.  The indexes are written by this project's suffixerator
tool in the same run."""
import hashlib
import os
import subprocess

import pytest

import locali_golden as lg
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
