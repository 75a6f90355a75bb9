"""The numpy restatement of the INDEX.esq sections and the sequence statistics
(tests/esq_sections_reference.py) against the host writer, which
test_forced_access_type_matches_reference pins to the reference's files, on
every case of tests/esq_edge_cases.py; and the host writer against what the
reference itself wrote for a dozen of the cases
(tests/golden/golden_esq_edges.json).  No GPU: this shows the restatement right
before tests/test_esq_sections_gpu.py holds the device to it."""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest

import esq_edge_cases as ec
import esq_sections_reference as ref
import oracle_util as ou
from test_host import EncInfo, SeqStats, _write_esq_forced, host  # noqa: F401  (fixture)

with open(os.path.join(ou.GOLDEN_DIR, "golden_esq_edges.json")) as _f:
    GOLDEN = json.load(_f)
STANDARD_CASES = [c for c in ec.cases() if c.alphabet in ec.STANDARD]
SHARED = ("totallength", "specialcharacters", "realspecialranges", "lengthofspecialprefix",
          "lengthofspecialsuffix", "wildcards", "realwildcardranges", "lengthofwildcardprefix",
          "lengthofwildcardsuffix", "numofsequences")


def memory_info(n):
    """a gtamd_encinfo for symbols that come from memory: one input of n bytes, no
    original characters (the arrays it points to live as long as the second value)"""
    tab = (ctypes.c_uint64 * 2)(n, n)
    info = EncInfo()
    info.filelengthtab = ctypes.cast(tab, ctypes.c_void_p)
    info.numfiles = 1
    return info, tab


def write_from_memory(host, enc, protein, idx, sat):
    """gtamd_write_esq_sat on symbols in memory, arguments as _write_esq_forced
    (tests/test_host.py) makes them; the statistics it returns"""
    names = (ctypes.c_char_p * 1)(b"symbols")
    info, keep = memory_info(enc.size)
    ss = SeqStats()
    err = ctypes.create_string_buffer(2048)
    rc = host.gtamd_write_esq_sat(idx.encode(), names, 1, enc.ctypes.data, enc.size, int(protein),
                                  ctypes.byref(info), 1, sat.encode(), ctypes.byref(ss), err, 2048)
    assert rc == 0, err.value
    del keep
    return ss


def padded(raw):
    """a section as `put` of esq_host.c leaves it: filled up to 8 bytes"""
    return raw + b"\0" * (-len(raw) % 8)


def expected_tail(case, sat):
    """the sections gtamd_write_esq_sections writes last, for three access types"""
    enc = case.enc
    if sat == "direct":
        return padded(enc.tobytes())
    if sat == "bytecompress":
        return padded(ref.bytecompress(enc, case.sigma, case.bits).tobytes())
    assert sat == "bit"
    tail = ref.twobit(enc, 1, 0).astype("<u8").tobytes()
    if (enc >= 254).any():       # no special bits without a special
        tail += ref.specialbits(enc).astype("<u8").tobytes()
    return tail


@pytest.mark.parametrize("case", STANDARD_CASES, ids=lambda c: c.name)
def test_sections_in_the_host_writers_files(host, case, tmp_path):
    protein = case.alphabet == "protein"
    idx = str(tmp_path / "idx")
    for sat in ("direct", "bytecompress") if protein else ("direct", "bit"):
        write_from_memory(host, case.enc, protein, idx, sat)
        with open(idx + ".esq", "rb") as f:
            raw = f.read()
        want = expected_tail(case, sat)
        assert len(raw) > len(want) and raw[len(raw) - len(want):] == want, sat
    sep = ref.separators(case.enc)
    if sep.size and case.enc.size < 255:
        # one page of 8-bit entries and its count (src/core/encseq.c:1714-1910)
        with open(idx + ".ssp", "rb") as f:
            assert f.read() == padded(sep.astype(np.uint8).tobytes()) + \
                np.array([sep.size], dtype="<u8").tobytes()


@pytest.mark.parametrize("case", ec.cases(), ids=lambda c: c.name)
def test_summary_against_the_host_statistics(host, case):
    exp = ref._expected_summary(case.enc, case.sigma)
    ss = SeqStats()
    host.gtamd_sequence_stats(case.enc.ctypes.data, case.enc.size, case.sigma, ctypes.byref(ss))
    for k in SHARED:
        assert getattr(ss, k) == exp[k], k
    # the stored-range counts are those of one of the three table widths
    assert (ss.specialranges, ss.wildcardranges) in list(zip(exp["specialrangestab"],
                                                             exp["wildcardrangestab"]))
    assert ss.numofchars == case.sigma
    # and the lists agree with the counts
    start, length = ref.wildcard_runs(case.enc)
    assert start.size == exp["realwildcardranges"] and int(length.sum()) == exp["wildcards"]
    assert ref.separators(case.enc).size == exp["numofsequences"] - 1
    assert ref.first_empty_sequence(case.enc) is None


@pytest.mark.parametrize("case", [c for c in STANDARD_CASES if c.alphabet == "dna"],
                         ids=lambda c: c.name)
def test_range_counts_per_table_width(host, case, tmp_path):
    """with a table type forced the host reports that type's stored ranges"""
    exp = ref._expected_summary(case.enc, case.sigma)
    for k, sat in enumerate(("uchar", "ushort", "uint32")):
        ss = write_from_memory(host, case.enc, False, str(tmp_path / "idx"), sat)
        assert (ss.specialranges, ss.wildcardranges) == (exp["specialrangestab"][k],
                                                         exp["wildcardrangestab"][k]), sat


def test_restatement_on_a_hand_made_sequence():
    enc = np.array([0, 1, 254, 255, 3], dtype=np.uint8)
    assert ref.twobit(enc, 1, 0).tolist() == [0x11C0000000000000, 0]
    assert ref.twobit(enc, 0, 2).tolist() == [0x1AC0000000000000, 0]
    assert ref.specialbits(enc).tolist() == [0x37FFFFFFFFFFFFFF, 0xF800000000000000]
    assert ref.bytecompress(enc, 4, 3).tolist() == [0b00000110, 0b01010110]
    assert [a.tolist() for a in ref.wildcard_runs(enc)] == [[2], [1]]
    assert ref.separators(enc).tolist() == [3]
    assert ref.first_empty_sequence(enc) is None
    for bad, at in (([255, 0], 0), ([0, 255], 1), ([0, 255, 255, 0], 2)):
        assert ref.first_empty_sequence(np.array(bad, dtype=np.uint8)) == at


def test_the_case_list_is_what_it_says():
    cases = ec.cases()
    assert len(cases) == 384 and max(c.enc.size for c in cases) == ec.BIG < 200_000
    assert all(c.enc.size > 0 and (c.enc[c.enc < 254] < c.sigma).all() for c in cases)
    assert set(GOLDEN) == set(ec.GOLDEN_CASES)


# ---- what the reference wrote ---------------------------------------------------
def write_fasta(case, tmp_path):
    path = tmp_path / ec.fasta_name(case)
    path.write_bytes(ec.fasta_bytes(case))
    return str(path)


def md5_of(path):
    with open(path, "rb") as f:
        return hashlib.md5(f.read()).hexdigest()


def check_against_golden(entry, sat, idx, ss):
    """INDEX.esq / INDEX.ssp at idx against the recorded md5s, and the statistics
    against the reference's INDEX.prj"""
    rec = entry["sat"][sat]
    for ext in ("esq", "ssp"):
        assert os.path.exists(idx + "." + ext) == (ext in rec), (sat, ext)
        if ext in rec:
            assert os.path.getsize(idx + "." + ext) == rec[ext]["bytes"], (sat, ext)
            assert md5_of(idx + "." + ext) == rec[ext]["md5"], (sat, ext)
    prj = dict(l.split("=") for l in rec["prj"].splitlines())
    for k in SHARED + ("specialranges", "wildcardranges"):
        assert getattr(ss, k) == int(prj[k]), (sat, k)


@pytest.mark.parametrize("name", ec.GOLDEN_CASES)
def test_host_writer_reproduces_the_reference(host, name, tmp_path):
    case, entry = ec.by_name(name), GOLDEN[name]
    path = write_fasta(case, tmp_path)
    assert md5_of(path) == entry["input_md5"]
    equal = ref._expected_summary(case.enc, case.sigma)["equallength"]
    assert sorted(entry["sat"]) == sorted(ec.legal_access_types(case, equal))
    for sat in entry["sat"]:
        idx = str(tmp_path / ("idx-" + sat))
        rc, msg, ss = _write_esq_forced(host, path, case.alphabet == "protein", idx, sat)
        assert rc == 0, msg
        check_against_golden(entry, sat, idx, ss)
