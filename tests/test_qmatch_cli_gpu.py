"""`gt-suffixerator-amd querymatch` on indexes the tool itself built: its output,
unsorted, against every call of tests/golden/golden_qmatch.json (md5 and line
count of the reference's output) and against the result the reference records
for `gt repfind -l 8 -r -ii Duplicate.fna`; on an index with 4-byte suffix
entries; with two query files; all three modes in one call; and the options and
indexes it refuses."""
import hashlib
import json
import os
import subprocess

import pytest

import oracle_util as ou
import qmatch_reference as qr
from genometools_amd import _lib
from test_qmatch_host import REFUSED

pytestmark = pytest.mark.gpu

CLI = os.path.join(_lib.HERE, "gt-suffixerator-amd")
with open(os.path.join(ou.GOLDEN_DIR, "golden_qmatch.json")) as _f:
    GOLDEN = json.load(_f)


@pytest.fixture(scope="module")
def cli(gpu):
    subprocess.run(["make", "-C", os.path.join(_lib.HERE, "csrc", "host")], check=True,
                   stdout=subprocess.DEVNULL)
    return CLI


@pytest.fixture(scope="module")
def indexes(cli, tmp_path_factory):
    """name|alphabet -> index built by the tool, once; .suf and the sequence are all it needs"""
    root, built = tmp_path_factory.mktemp("querymatch"), {}

    def get(name, alphabet="dna", extra=()):
        key = (name, alphabet) + tuple(extra)
        if key not in built:
            idx = str(root / ("idx%d" % len(built)))
            src = ou.fixture_path(name)
            subprocess.run([cli, "-" + alphabet, "-tis", "-suf", "-ssp", "-indexname", idx, "-db",
                            os.path.basename(src)] + list(extra), check=True, cwd=os.path.dirname(src),
                           stdout=subprocess.DEVNULL)
            built[key] = idx
        return built[key]
    return get


def _run(cli, idx, args=(), queries=()):
    cmd = [cli, "querymatch"] + list(args) + (["-q"] + [ou.fixture_path(q) for q in queries] if queries else [])
    p = subprocess.run(cmd + ["-ii", idx], capture_output=True)
    assert p.returncode == 0 and p.stderr == b"", (args, p.stderr)
    return p.stdout


def _fails(cli, args):
    p = subprocess.run([cli, "querymatch"] + list(args), capture_output=True)
    assert p.returncode == 1 and p.stdout == b"", (args, p.stdout[:200])
    lines = p.stderr.decode().splitlines()
    assert len(lines) == 1 and lines[0].startswith("gt repfind: error: "), p.stderr
    return lines[0][len("gt repfind: error: "):]


def _parts(key):
    subject, alphabet, args, queries = key.split("|")
    return subject, alphabet, args.split(), tuple(queries.split(",")) if queries else ()


SUBJECTS = sorted({k.split("|")[0] for k in GOLDEN["calls"]})


@pytest.mark.parametrize("subject", SUBJECTS)
def test_every_golden_call(cli, indexes, subject):
    calls = [k for k in sorted(GOLDEN["calls"]) if k.split("|")[0] == subject]
    assert len(GOLDEN["calls"]) == 65 and len(SUBJECTS) == 6 and len(calls) in (4, 12, 13)
    for key in calls:
        name, alphabet, args, queries = _parts(key)
        out = _run(cli, indexes(name, alphabet), args, queries)
        assert not out.startswith(b"#")
        text = "".join(l + "\n" for l in qr.normalised(out)).encode("latin-1")
        want = GOLDEN["calls"][key]
        assert (hashlib.md5(text).hexdigest(), text.count(b"\n")) == (want["md5"], want["lines"]), key


def test_recorded_result_and_text_fixtures(cli, indexes):
    with open(os.path.join(ou.GOLDEN_DIR, "repfind", "Duplicate.fna-r.result"), "rb") as f:
        want = qr.normalised(f.read())
    assert len(want) == 64
    assert qr.normalised(_run(cli, indexes("Duplicate.fna"), ["-l", "8", "-r"])) == want
    for name, key in GOLDEN["texts"].items():
        subject, alphabet, args, queries = _parts(key)
        with open(os.path.join(ou.GOLDEN_DIR, "qmatch", name), "rb") as f:
            assert _run(cli, indexes(subject, alphabet), args, queries) == f.read(), name


def test_suftabuint_gives_the_same_output(cli, indexes):
    a, b = indexes("Atinsert.fna"), indexes("Atinsert.fna", extra=["-suftabuint"])
    assert os.path.getsize(a + ".suf") == 2 * os.path.getsize(b + ".suf")
    for args, queries, count in ((["-l", "8"], ("Atinsert_seqrange_3-7.fna",), 543), (["-l", "8", "-r"], (), 326),
                                 (["-l", "8", "-p"], ("Duplicate.fna",), 82)):
        out = _run(cli, b, args, queries)
        assert out == _run(cli, a, args, queries) and out.count(b"\n") == count


def test_two_query_files_number_their_units_on(cli, indexes):
    idx = indexes("Atinsert.fna")
    both = _run(cli, idx, ["-l", "8", "-p"], ("Duplicate.fna", "Atinsert_seqrange_3-7.fna")).decode().splitlines()
    first = _run(cli, idx, ["-l", "8", "-p"], ("Duplicate.fna",)).decode().splitlines()
    second = _run(cli, idx, ["-l", "8", "-p"], ("Atinsert_seqrange_3-7.fna",)).decode().splitlines()
    assert (len(first), len(second), len(both)) == (82, 61, 143)
    assert both[:82] == first                       # Duplicate.fna holds units 0 and 1
    renumbered = [" ".join(f[:5] + [str(int(f[5]) + 2)] + f[6:]) for f in (l.split() for l in second)]
    assert both[82:] == renumbered


def test_all_modes_in_one_call(cli, indexes):
    idx, q = indexes("Atinsert.fna"), ("Atinsert_seqrange_3-7.fna",)
    parts = [_run(cli, idx, ["-l", "8"] + mode, q) for mode in ([], ["-r"], ["-p"])]
    assert [p.count(b"\n") for p in parts] == [543, 221, 61]
    assert _run(cli, idx, ["-l", "8", "-f", "-r", "-p"], q) == b"".join(parts)
    assert _run(cli, idx, ["-p", "-l", "8", "-r", "-f"], q) == b"".join(parts)       # (always f, r, p)
    assert _run(cli, idx, ["-l", "8", "-f"], q) == parts[0]
    assert _run(cli, idx, ["-l", "8", "-r", "-p"], q) == parts[1] + parts[2]


def test_default_length_and_verbose(cli, indexes):
    idx, q = indexes("Atinsert.fna"), ("Atinsert_seqrange_3-7.fna",)
    want = _run(cli, idx, ["-l", "20"], q)
    assert 0 < want.count(b"\n") < 105
    assert _run(cli, idx, [], q) == want                               # default -l 20
    verbose = _run(cli, idx, ["-v", "-r", "-f"], q)
    marks = [l for l in verbose.splitlines() if l.startswith(b"#")]
    assert len(marks) == 2 and marks[0].startswith(b"# F:") and marks[1].startswith(b"# R:")
    assert b"".join(l for l in verbose.splitlines(True) if not l.startswith(b"#")) == \
        want + _run(cli, idx, ["-r"], q)


@pytest.mark.parametrize("option", REFUSED)
def test_refused_options(cli, indexes, option):
    msg = _fails(cli, ["-l", "8", "-r", "-ii", indexes("Duplicate.fna"), option])
    assert msg == 'option "%s" is not supported by the MI355X engine' % option


def test_other_refusals(cli, indexes, tmp_path):
    idx = indexes("Duplicate.fna")
    assert "repfind" in _fails(cli, ["-l", "8", "-ii", idx])
    assert "repfind" in _fails(cli, ["-l", "8", "-f", "-r", "-ii", idx])
    assert _fails(cli, ["-ii", idx, "-r", "-l", "0"]) == 'argument to option "-l" must be an integer >= 1'
    assert "DNA" in _fails(cli, ["-ii", indexes("sw100K1.fsa", "protein"), "-p", "-q", ou.fixture_path("sw100K2.fsa")])
    # a read mode other than forward, a mirrored index
    src = ou.fixture_path("Duplicate.fna")
    for extra, word in ((["-dir", "rev"], "read mode"), (["-mirrored"], "mirrored")):
        other = str(tmp_path / ("x" + extra[0][1:]))
        subprocess.run([cli, "-dna", "-tis", "-suf", "-ssp", "-indexname", other, "-db",
                        os.path.basename(src)] + extra, check=True, cwd=os.path.dirname(src),
                       stdout=subprocess.DEVNULL)
        assert word in _fails(cli, ["-l", "8", "-r", "-ii", other])
    # the table it needs
    idx = str(tmp_path / "nosuf")
    subprocess.run([cli, "-dna", "-tis", "-ssp", "-suf", "-indexname", idx, "-db", os.path.basename(src)],
                   check=True, cwd=os.path.dirname(src), stdout=subprocess.DEVNULL)
    os.remove(idx + ".suf")
    assert _fails(cli, ["-l", "8", "-r", "-ii", idx]) == \
        'cannot open file "%s.suf": No such file or directory' % idx


def test_repfind_still_refuses_these_options(cli, indexes):
    for option in ("-r", "-p", "-q"):
        p = subprocess.run([cli, "repfind", "-l", "8", "-ii", indexes("Duplicate.fna"), option], capture_output=True)
        assert p.returncode == 1 and p.stderr.decode() == \
            'gt repfind: error: option "%s" is not supported by the MI355X engine\n' % option
