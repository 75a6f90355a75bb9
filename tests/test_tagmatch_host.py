"""CPU-side checks of the tag match boundary: include/gtamd_tagmatch.h is
exported and bound, its host-only entry point works without a device,
`gt-suffixerator-amd tagerator` words the errors that end before the device as
`gt tagerator` does, and the brute-force restatement with its line formatter
(tests/tagmatch_reference.py) reproduces every output of the reference recorded
in tests/golden/golden_tagmatch.json (the match lines of one tag sorted) --
before a device is involved.  The brute force itself is held against a plain
table of edit distances."""
import ctypes
import hashlib
import json
import os
import re
import subprocess

import numpy as np
import pytest

import oracle_util as ou
import tagmatch_reference as tr
from genometools_amd import _lib, tagmatch

HEADER = os.path.join(_lib.ROOT, "include", "gtamd_tagmatch.h")
CLI = os.path.join(_lib.HERE, "gt-suffixerator-amd")
REFUSED = ["-pck", "-online", "-cmp", "-maxocc", "-skpp", "-maxdepth"]
TAGDIR = os.path.join(ou.GOLDEN_DIR, "tagmatch")

with open(os.path.join(ou.GOLDEN_DIR, "golden_tagmatch.json")) as _f:
    GOLDEN = json.load(_f)


def _header_text():
    with open(HEADER) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


def test_every_declared_symbol_is_exported_and_bound():
    """the nine entry points of the enumeration and the getter of K'"""
    lib = _lib.load()
    declared = sorted(set(re.findall(r"\b(gtamd_[a-z_0-9]+)\s*\(", _header_text())))
    assert len(declared) == 10, declared
    for name in declared:
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes == _lib.TAGMATCH_ABI[name][1], name
    assert sorted(_lib.TAGMATCH_ABI) == declared
    assert sorted(set(declared) - {"gtamd_tagmatch_best_k"}) == sorted(
        "gtamd_tagmatch_" + n for n in ("create", "destroy", "geometry", "set_index", "set_index_host",
                                        "set_index_esa", "prepare", "emit", "get_info"))
    assert HEADER in _lib.HEADERS
    assert os.path.join(_lib.HERE, "csrc", "esa_tagmatch.hip") in _lib.SOURCES
    assert os.path.join(_lib.HERE, "csrc", "esa_tagmatch_core.h") in _lib.HEADERS


def test_info_structure_and_flags_match_the_header():
    text = _header_text()
    body = text[text.index("typedef struct {\n  uint64_t jobs"):text.index("} gtamd_tagmatch_info;")]
    names = re.findall(r"\b(?:u?int\d+_t|float)\s+([a-z_]+);", body)
    assert names == [n for n, _ in _lib.TagmatchInfo._fields_]
    assert ctypes.sizeof(_lib.TagmatchInfo) == 8 * 8 + 8
    flags = dict(re.findall(r"GTAMD_TAGMATCH_([A-Z_]+) = (\d+)", text))
    assert flags == {"FORWARD": "1", "REVCOMP": "2", "BEST": "4", "WITH_WILDCARDS": "8"}
    assert (tagmatch.FORWARD, tagmatch.REVCOMP, tagmatch.BEST, tagmatch.WITH_WILDCARDS) == (1, 2, 4, 8)
    assert (tr.FORWARD, tr.REVCOMP, tr.BEST, tr.WITH_WILDCARDS) == (1, 2, 4, 8)
    assert "#define GTAMD_TAGMATCH_NO_K 0xffffffffu" in text and tagmatch.NO_K == tr.NO_K == 0xffffffff


def test_geometry_needs_no_device():
    waves, least, levels = tagmatch.geometry()
    assert waves >= 1 and least >= 1
    assert levels >= 64 + 63          # depths 0 .. m + K - 1


def test_no_cpu_fallback():
    lib = _lib.load()
    if lib.gtamd_device_count() > 0:
        pytest.skip("a device is present")
    assert not lib.gtamd_tagmatch_create(0)
    assert b"no HIP device" in lib.gtamd_esa_last_error()
    with pytest.raises(_lib.EsaError, match="no HIP device"):
        tagmatch.TagMatches()


def test_pack_and_unpack():
    symbols, offsets = tagmatch.pack_tags([[0, 1, 2], [3], []])
    assert symbols.tolist() == [0, 1, 2, 3] and offsets.tolist() == [0, 3, 4, 4] and offsets.dtype == np.uint64
    tag, rc, p, length, dist = tagmatch.unpack([[7, 5, 12 | 2 << 32]])
    assert (tag[0], rc[0], p[0], length[0], dist[0]) == (3, True, 5, 12, 2)


# ---- the brute force against the table of edit distances ----

def test_bit_vector_brute_force_against_the_plain_table():
    rng = np.random.default_rng(11)
    cases = 0
    for _ in range(200):
        sigma = int(rng.choice([2, 4]))
        n = int(rng.integers(1, 40))
        enc = rng.integers(0, sigma, n).astype(np.uint8)
        enc[rng.random(n) < 0.08] = 254
        enc[rng.random(n) < 0.05] = 255
        m = int(rng.integers(1, 9))
        tag = rng.integers(0, sigma, m).astype(np.uint8)
        K = int(rng.integers(0, m))
        wild = bool(K > 0 and rng.integers(2))
        p, length, dist = tr.strand_matches(enc, tag, K, wild)
        got = {int(a): (int(b), int(c)) for a, b, c in zip(p, length, dist)}
        want = {}
        for start in range(n):
            hit = tr.dp_match(tag, enc, start, K, wild)
            if hit is not None:
                want[start] = hit
        assert got == want, (enc.tolist(), tag.tolist(), K, wild)
        assert all(d == K for _, d in got.values())        # the first depth at which row m is <= K holds K
        cases += len(want)
    assert cases > 300


_CODE = {"a": 0, "c": 1, "g": 2, "t": 3, "n": 254, "|": 255}


def test_a_case_worked_by_hand():
    """acgt with one difference in acgtacct|agtnacg: at 0 acg (t deleted: the
    shortest length counts, not acgt itself), at 1 cgt (a deleted: every start is
    judged on its own), at 4 acct (acc needs two); in the second sequence agt at
    9 (c deleted); acg at 13 ends the text.  The wildcard passes only when asked
    to."""
    enc = np.array([_CODE[c] for c in "acgtacct|agtnacg"], dtype=np.uint8)
    suf = ou.esa(enc, 4)["suf"]
    tag = tr.encode_tag("acgt")
    rec, best = tr.expected(enc, suf, [tag], 1, tr.FORWARD)
    by_p = sorted((int(r[1]), int(r[2]) & 0xffffffff, int(r[2]) >> 32) for r in rec)
    assert by_p == [(0, 3, 1), (1, 3, 1), (4, 4, 1), (9, 3, 1), (13, 3, 1)]
    assert best.tolist() == [1]
    # the records are in table order: acct.., acgt.., acg(end: behind every letter), agt.., cgt..
    assert [int(r[1]) for r in rec] == [4, 0, 13, 9, 1]
    exact, best0 = tr.expected(enc, suf, [tag], 1, tr.FORWARD | tr.BEST)
    assert [(int(r[1]), int(r[2])) for r in exact] == [(0, 4)] and best0.tolist() == [0]
    # gtn: with the wildcard as a symbol, g t + one replacement
    wild, _ = tr.expected(enc, suf, [tr.encode_tag("gta")], 1, tr.FORWARD | tr.WITH_WILDCARDS)
    assert (10, 2 | 1 << 32) in [(int(r[1]), int(r[2])) for r in wild]
    none, nobest = tr.expected(enc, suf, [tr.encode_tag("tttt")], 1, tr.FORWARD | tr.BEST)
    assert none.shape == (0, 3) and nobest.tolist() == [tr.NO_K]


# ---- the restatement against the reference's outputs ----

def parse_call(key):
    subject, alphabet, args, tagfiles = key.split("|")
    args = args.split()
    K = int(args[args.index("-e") + 1])
    flags = (0 if "-nod" in args else tr.FORWARD) | (0 if "-nop" in args else tr.REVCOMP) | \
        (tr.BEST if "-best" in args else 0)
    # the switch stores "no wildcards": only `-withwildcards no` lets them pass, and only with K > 0
    if "-withwildcards" in args and args[args.index("-withwildcards") + 1:][:1] == ["no"] and K > 0:
        flags |= tr.WITH_WILDCARDS
    output = tuple(args[args.index("-output") + 1:]) if "-output" in args else tr.DEFAULT_OUTPUT
    return subject, alphabet == "protein", K, flags, output, tagfiles.split(",")


_FIXTURES = {}


def fixture(name, protein):
    if name not in _FIXTURES:
        _FIXTURES[name] = tr.fixture(name, protein)
    return _FIXTURES[name]


def expected_text(key):
    """what the reference prints, its `# indexname` and `# queryfile` lines
    dropped and the blocks sorted: up to the `#` line of the first tag that is
    not longer than K"""
    subject, protein, K, flags, output, tagfiles = parse_call(key)
    enc, suf = fixture(subject, protein)
    tags = tr.read_tags([os.path.join(TAGDIR, t + ".tags.fna") for t in tagfiles])
    stop = next((i for i, t in enumerate(tags) if K > 0 and len(t) <= K), len(tags))
    pre = tr.preamble(K, "", [], output)
    lines = [pre[0], pre[-1]] + tr.tool_lines(enc, suf, tr.PROTEIN if protein else tr.DNA, tags[:stop], K, flags, output)
    if stop < len(tags):
        lines.append("#" + ("\t%d" % stop if "tagnum" in output else "") +
                     (("\t" if "tagnum" in output else "") + tags[stop] if "tagseq" in output else ""))
    return "".join(l + "\n" for l in tr.block_sorted(lines)).encode("latin-1")


SUBJECTS = sorted({k.split("|")[0] for k in GOLDEN["calls"]})


@pytest.mark.parametrize("subject", SUBJECTS)
def test_brute_force_and_formatter_reproduce_the_reference(subject):
    assert len(GOLDEN["calls"]) == 45 and len(SUBJECTS) == 7
    calls = [k for k in sorted(GOLDEN["calls"]) if k.split("|")[0] == subject]
    assert len(calls) in (2, 6, 8, 9)
    for key in calls:
        text, want = expected_text(key), GOLDEN["calls"][key]
        assert (hashlib.md5(text).hexdigest(), text.count(b"\n")) == (want["md5"], want["lines"]), key


def test_the_goldens_cover_every_option():
    calls = GOLDEN["calls"]
    seen = set()
    for key, entry in calls.items():
        _, _, K, flags, output, tagfiles = parse_call(key)
        if entry["lines"] > 40:
            seen.add((K, flags & 3, bool(flags & tr.BEST), bool(flags & tr.WITH_WILDCARDS)))
        # a tag of one letter ends every call with K > 0, after the blocks in front of it
        assert (entry["exit"], "must be longer than the allowed number of errors" in entry["error"]) == \
            ((1, True) if K > 0 else (0, False)), key
    assert {(0, 3, False, False), (1, 3, False, False), (2, 3, False, False), (2, 3, True, False),
            (1, 2, False, False), (1, 1, False, False), (2, 3, False, True)} <= seen
    with_wild = calls["Atinsert.fna|dna|-e 2 -withwildcards no|Atinsert.fna"]
    without = calls["Atinsert.fna|dna|-e 2|Atinsert.fna"]
    assert with_wild["lines"] > without["lines"]
    assert calls["Atinsert.fna|dna|-e 2 -withwildcards|Atinsert.fna"] == without
    assert any(set(parse_call(k)[4]) == set(tr.OUTPUT_KEYWORDS) for k in calls)
    assert any(len(parse_call(k)[5]) == 2 for k in calls)


def test_text_fixtures_are_those_of_the_json():
    assert len(GOLDEN["texts"]) == 3
    for name, key in GOLDEN["texts"].items():
        raw = open(os.path.join(TAGDIR, name), "rb").read()
        want = GOLDEN["calls"][key]
        assert (hashlib.md5(raw).hexdigest(), raw.count(b"\n")) == (want["md5"], want["lines"]) and want["lines"] > 30
        assert raw == expected_text(key)


# ---- the tool: what ends before a device is asked for ----

@pytest.fixture(scope="module")
def index(tmp_path_factory):
    """projects without tables, written by the tool's host side: DNA, protein"""
    subprocess.run(["make", "-C", os.path.join(_lib.HERE, "csrc", "host")], check=True,
                   stdout=subprocess.DEVNULL)
    root = tmp_path_factory.mktemp("tagmatch")
    out = {}
    for kind, name in (("dna", "Duplicate.fna"), ("protein", "sw100K1.fsa")):
        out[kind] = str(root / kind)
        subprocess.run([CLI, "-" + kind, "-db", ou.fixture_path(name), "-indexname", out[kind]], check=True)
    return out


def _run(*args):
    return subprocess.run([CLI, "tagerator"] + list(args), capture_output=True, text=True)


def _error(*args, stdout=""):
    p = _run(*args)
    prefix = "gt tagerator: error: "
    assert p.returncode == 1 and p.stderr.startswith(prefix) and p.stderr.endswith("\n") and \
        p.stderr.count("\n") == 1, (p.returncode, p.stdout, p.stderr)
    if stdout is not None:
        assert p.stdout == stdout, p.stdout
    return p.stderr[len(prefix):-1]


TAGS = os.path.join(TAGDIR, "Duplicate.fna.tags.fna")


def test_argument_errors(index):
    idx = index["dna"]
    assert _error("-e", "1", "-esa", idx) == 'option "-q" is mandatory'
    assert _error("-e", "1", "-q", TAGS) == 'either option "-esa" or option "-pck" is mandatory'
    assert _error("-q", TAGS, "-esa", idx, "-e") == 'missing argument to option "-e"'
    assert _error("-e", "1", "-esa", idx, "-q") == 'missing argument to option "-q"'
    assert _error("-e", "1", "-esa", idx, "-q", TAGS, "extra", "-nosuch").startswith("unknown option: -nosuch")
    assert _error("-best", "-q", TAGS, "-esa", idx) == "option -best requires option -e"
    for bad in ("-1", "-7"):               # no way of leaving -e out: the answer names -e, not -maxocc
        assert _error("-e", bad, "-esa", idx, "-q", TAGS) == 'argument to option "-e" must be a non-negative integer'
    msg = _error("-q", TAGS, "-esa", idx)
    assert '"-e"' in msg and "-maxocc" in msg            # the matching statistics belong to -maxocc
    for option in REFUSED:
        extra = [index["dna"]] if option == "-pck" else ["4"] if option in ("-maxocc", "-maxdepth") else []
        assert _error("-e", "1", "-esa", idx, "-q", TAGS, option, *extra) == \
            'option "%s" is not supported by the MI355X engine' % option
    assert _error("-e", "1", "-esa", idx, "-q", TAGS, "-output", "tagnum", "nosuch").startswith(
        'illegal argument "nosuch" to option -output')
    assert "tagstartpos" in _error("-e", "1", "-esa", idx, "-q", TAGS, "-output", "tagstartpos")


def test_file_errors_end_before_the_device(index, tmp_path):
    """as in the reference, the three lines of gt_tagerator_runner come before the
    index is read"""
    def first_lines(K, idx):
        return "# computing complete matches %s\n# indexname(esa)=%s\n# queryfile=%s\n" % (
            "with up to %d differences" % K if K else "without differences (exact matches)", idx, TAGS)
    idx = index["dna"]
    missing = str(tmp_path / "nosuch")
    assert _error("-e", "1", "-esa", missing, "-q", TAGS, stdout=first_lines(1, missing)) == \
        "cannot open file '%s.prj'" % missing
    # the project has no tables
    assert _error("-e", "1", "-esa", idx, "-q", TAGS, stdout=first_lines(1, idx)) == \
        'cannot open file "%s.suf": No such file or directory' % idx
    assert '"-nop"' in _error("-e", "0", "-esa", index["protein"], "-q", TAGS, stdout=first_lines(0, index["protein"]))


def test_tag_errors_follow_the_blocks_before_them(index, tmp_path):
    """the errors of dotransformtag and of the length rule are worded by the host
    side, behind the `#` lines; those in the first tag need no device"""
    idx = index["dna"]
    n = int(dict(l.split("=") for l in open(idx + ".prj").read().splitlines())["totallength"])
    with open(idx + ".suf", "wb") as f:
        f.write(bytes(8 * (n + 1)))
    try:
        def tags(*seqs):
            path = str(tmp_path / "t.fna")
            with open(path, "w") as f:
                f.write("".join(">\n%s\n" % s for s in seqs))
            return path
        pre = "# computing complete matches with up to 2 differences\n# indexname(esa)=%s\n# queryfile=%s\n" \
              "# for each match show: tagnum tagseq dblength dbstartpos strand \n" % (idx, str(tmp_path / "t.fna"))
        long = "acgt" * 16 + "a"
        assert _error("-e", "2", "-esa", idx, "-q", tags(long), stdout=pre) == \
            'tag "%s" of length 65; tags must not be longer than 64' % long
        assert _error("-e", "2", "-esa", idx, "-q", tags("ac"), stdout=pre + "#\t0\tac\n") == \
            'tag "ac" of length 2; tags must be longer than the allowed number of errors (which is 2)'
        assert _error("-e", "2", "-esa", idx, "-q", tags("acgnt"), stdout=pre) == "wildcard in tag number 0"
        assert _error("-e", "2", "-esa", idx, "-q", tags("ac.gt"), stdout=pre) == \
            "undefined character '.' in tag number 0"
    finally:
        os.remove(idx + ".suf")
