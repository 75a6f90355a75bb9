"""The device encoder's statistics and INDEX.esq sections (k_run_summary and the
host merge, k_empty_sequence, k_esq_twobit / _specialbits / _bitpack, k_positions
of genometools_amd/csrc/esa_encode.hip), fed through gtamd_encoder_set_symbols,
against the numpy restatement of tests/esq_sections_reference.py on every case of
tests/esq_edge_cases.py: runs and ends of input on word, thread and tile borders.
tests/test_esq_sections_reference.py shows the restatement right, without a GPU.
The two-bit words are compared for the alphabets whose codes fit two bits (DNA and
the 2-letter one), the files for the alphabets gtamd_write_esq_sat takes (DNA and
protein); everything else for all four."""
import ctypes
import os

import numpy as np
import pytest

import esq_edge_cases as ec
import esq_sections_reference as ref
from genometools_amd import _lib, encode
from genometools_amd._lib import EncodeSummary, EsaError
from test_esq_sections_reference import (GOLDEN, check_against_golden, memory_info, write_fasta,
                                         write_from_memory)
from test_host import EncInfo, SeqStats, _read_esq, host  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
GUARD = 0xA5A5A5A5A5A5A5A5
NOT_FINISHED = b"gtamd_encoder_finish has not completed"
EMPTY_SEQUENCE = b"the sequence contains an empty sequence"
CASES = ec.cases()
STANDARD_CASES = [c for c in CASES if c.alphabet in ec.STANDARD]


class Alphabet(ctypes.Structure):          # gtamd_alphabet, include/gtamd_host.h
    _fields_ = [("symbolmap", ctypes.c_uint8 * 256), ("numofchars", ctypes.c_uint32),
                ("characters", ctypes.c_char * 64), ("wildcardshow", ctypes.c_char),
                ("alphatype", ctypes.c_int), ("bitspersymbol", ctypes.c_uint),
                ("alphadef", ctypes.c_void_p), ("lengthofalphadef", ctypes.c_uint64)]


def _symbolmap(sigma):
    """sigma letters from 'a' on ('0', '1' behind 'z'), '*' the wildcard"""
    m = np.full(256, 253, dtype=np.uint8)
    for code, ch in enumerate("abcdefghijklmnopqrstuvwxyz01"[:sigma]):
        m[ord(ch)] = code
    m[ord("*")] = 254
    return m


@pytest.fixture(scope="module")
def encoders(gpu):
    """one encoder per alphabet: the built-in ones, and two made from a symbol map"""
    lib = _lib.load()
    made = {"dna": lib.gtamd_encoder_create(0, 0), "protein": lib.gtamd_encoder_create(0, 1)}
    for name in ("ab", "l28"):
        sigma, bits = ec.ALPHABETS[name]
        m = _symbolmap(sigma)
        made[name] = lib.gtamd_encoder_create_map(0, m.ctypes.data, sigma, bits)
    assert all(made.values()), lib.gtamd_esa_last_error()
    yield made
    for e in made.values():
        lib.gtamd_encoder_destroy(e)


def _set(lib, e, enc):
    return lib.gtamd_encoder_set_symbols(e, enc.ctypes.data if enc.size else None, enc.size)


def _summary(lib, e):
    s = EncodeSummary()
    assert lib.gtamd_encoder_get_summary(e, ctypes.byref(s)) == 0, lib.gtamd_esa_last_error()
    return {name: list(getattr(s, name)) if hasattr(getattr(s, name), "__len__") else getattr(s, name)
            for name, _ in s._fields_}


def _guarded(count, dtype=np.uint64):
    """the caller's array, one entry longer than the section"""
    return np.full(count + 1, GUARD if dtype == np.uint64 else 0xA5, dtype=dtype)


def _intact(a, count):
    return a[count] == (GUARD if a.dtype == np.uint64 else 0xA5)


def check_summary(lib, e, case):
    got = _summary(lib, e)
    exp = ref._expected_summary(case.enc, case.sigma)
    for k, v in exp.items():
        assert got[k] == v, k
    assert set(got) == set(exp) | {"originaldistribution"}
    assert got["characterdistribution"][case.sigma:] == [0] * (32 - case.sigma)
    assert got["originaldistribution"] == [0] * 256
    return got


def check_sections(lib, e, case):
    """every section equal to the restatement, every word, byte and entry, and the
    entry behind each section untouched"""
    enc, n = case.enc, int(case.enc.size)
    err = lib.gtamd_esa_last_error
    assert lib.gtamd_encoder_length(e) == n
    if case.sigma <= 4:            # two bits hold no more
        units = ref.twobit_units(n)
        for bitaccess, fill in [(1, 0), (0, 0), (0, 1), (0, 2), (0, 3)]:
            w = _guarded(units)
            assert lib.gtamd_encoder_pack_twobit(e, bitaccess, fill, w.ctypes.data, units + 1) == 0, err()
            assert _intact(w, units), (bitaccess, fill)
            assert np.array_equal(w[:units], ref.twobit(enc, bitaccess, fill)), (bitaccess, fill)
    units = ref.specialbits_units(n)
    w = _guarded(units)
    assert lib.gtamd_encoder_pack_specialbits(e, w.ctypes.data, units + 1) == 0, err()
    assert _intact(w, units)
    assert np.array_equal(w[:units], ref.specialbits(enc))
    want = ref.bytecompress(enc, case.sigma, case.bits)
    b = _guarded(want.size, np.uint8)
    assert lib.gtamd_encoder_pack_bytecompress(e, b.ctypes.data, want.size + 1) == 0, err()
    assert _intact(b, want.size)
    assert np.array_equal(b[:want.size], want)
    start, length = ref.wildcard_runs(enc)
    s, ln = _guarded(start.size), _guarded(start.size)
    assert lib.gtamd_encoder_get_wildcard_runs(e, s.ctypes.data, ln.ctypes.data, start.size + 1) == 0, err()
    assert _intact(s, start.size) and _intact(ln, start.size)
    assert np.array_equal(s[:start.size], start) and np.array_equal(ln[:start.size], length)
    sep = ref.separators(enc)
    p = _guarded(sep.size)
    assert lib.gtamd_encoder_get_separators(e, p.ctypes.data, sep.size + 1) == 0, err()
    assert _intact(p, sep.size)
    assert np.array_equal(p[:sep.size], sep)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_summary_and_sections(encoders, case):
    lib, e = _lib.load(), encoders[case.alphabet]
    assert _set(lib, e, case.enc) == 0, lib.gtamd_esa_last_error()
    check_summary(lib, e, case)
    check_sections(lib, e, case)


def test_the_case_list_reaches_what_it_is_meant_to(encoders):
    """from the device's own summaries: a run that the 8-, 16- and 32-bit tables
    cut differently, an input of specials only, a sequence of one symbol"""
    lib = _lib.load()
    graded, all_special, single = [], [], []
    for case in CASES:
        assert _set(lib, encoders[case.alphabet], case.enc) == 0, case.name
        s = _summary(lib, encoders[case.alphabet])
        tab = s["specialrangestab"]
        if tab[0] > tab[1] > tab[2]:
            graded.append(case.name)
        if s["lengthofspecialprefix"] == s["totallength"]:
            all_special.append(case.name)
        if s["minseqlen"] == 1:
            single.append(case.name)
    assert graded and all_special and single


def test_symbols_come_back(encoders):
    lib, e = _lib.load(), encoders["dna"]
    for name in ("d-run-s4095-len257-dna", "a-letters-n4097-dna", "c-both-n8193-dna", "b-wildcards-n1-dna"):
        enc = ec.by_name(name).enc
        n = int(enc.size)
        assert _set(lib, e, enc) == 0
        windows = {(0, n), (n - 1, 1), (n, 0), (0, 0), (n // 2, 0)}
        for edge in (4096, 8192):
            if edge < n:
                windows |= {(edge - 1, 1), (edge - 1, 2), (edge, 1), (edge, n - edge), (edge - 7, 7),
                            (edge, 0), (0, edge), (0, edge + 1)}
        for first, count in sorted(windows):
            dst = _guarded(count, np.uint8)
            assert lib.gtamd_encoder_copy_symbols(e, dst.ctypes.data, first, count) == 0, (first, count)
            assert _intact(dst, count) and np.array_equal(dst[:count], enc[first:first + count]), (first, count)
        for first, count in ((n, 1), (n + 1, 0), (0, n + 1), (n - 1, 2), (1 << 63, 1 << 63), (1, (1 << 64) - 1)):
            dst = _guarded(8, np.uint8)
            assert lib.gtamd_encoder_copy_symbols(e, dst.ctypes.data, first, count) == -1, (first, count)
            assert lib.gtamd_esa_last_error() == b"range [%d, +%d) exceeds the %d encoded symbols" % (
                first, count, n)
            assert (dst == 0xA5).all()


# ---- files -----------------------------------------------------------------------
@pytest.fixture(scope="module")
def device_writer(host):
    host.gtamd_alphabet_standard.restype = None
    host.gtamd_alphabet_standard.argtypes = [ctypes.POINTER(Alphabet), ctypes.c_int]
    host.gtamd_write_esq_device_alpha.restype = ctypes.c_int
    host.gtamd_write_esq_device_alpha.argtypes = [
        ctypes.c_char_p, ctypes.POINTER(ctypes.c_char_p), ctypes.c_size_t, ctypes.c_void_p,
        ctypes.POINTER(Alphabet), ctypes.POINTER(EncInfo), ctypes.c_int, ctypes.c_char_p,
        ctypes.POINTER(SeqStats), ctypes.c_char_p, ctypes.c_size_t]

    def write(e, protein, idx, sat, name, info):
        a = Alphabet()
        host.gtamd_alphabet_standard(ctypes.byref(a), int(protein))
        names = (ctypes.c_char_p * 1)(name)
        ss = SeqStats()
        err = ctypes.create_string_buffer(2048)
        rc = host.gtamd_write_esq_device_alpha(idx.encode(), names, 1, e, ctypes.byref(a),
                                               ctypes.byref(info), 1, sat.encode(), ctypes.byref(ss),
                                               err, 2048)
        assert rc == 0, (sat, err.value)
        return ss
    return write


def _fields(ss):
    return [getattr(ss, k) for k, _ in ss._fields_]


@pytest.mark.parametrize("case", STANDARD_CASES, ids=lambda c: c.name)
def test_device_written_files(encoders, host, device_writer, case, tmp_path):
    """gtamd_write_esq_device_alpha after set_symbols against gtamd_write_esq_sat
    from the same symbols, with every access type legal for the case"""
    lib, e, protein = _lib.load(), encoders[case.alphabet], case.alphabet == "protein"
    assert _set(lib, e, case.enc) == 0, lib.gtamd_esa_last_error()
    equal = ref._expected_summary(case.enc, case.sigma)["equallength"]
    for sat in ec.legal_access_types(case, equal):
        dev, hst = str(tmp_path / ("dev-" + sat)), str(tmp_path / ("host-" + sat))
        info, keep = memory_info(case.enc.size)
        ss_dev = device_writer(e, protein, dev, sat, b"symbols", info)
        ss_host = write_from_memory(host, case.enc, protein, hst, sat)
        del keep
        assert _fields(ss_dev) == _fields(ss_host), sat
        for ext in ("esq", "ssp"):
            assert os.path.exists(dev + "." + ext) == os.path.exists(hst + "." + ext), (sat, ext)
            if os.path.exists(hst + "." + ext):
                with open(dev + "." + ext, "rb") as f, open(hst + "." + ext, "rb") as g:
                    assert f.read() == g.read(), (sat, ext)
        back, was_protein, _ = _read_esq(host, dev)
        assert was_protein == protein and np.array_equal(back, case.enc), sat


@pytest.mark.parametrize("name", ec.GOLDEN_CASES)
def test_device_written_files_are_the_references(encoders, host, device_writer, name, tmp_path):
    """the cases the reference encoded: its md5s from the device's sections"""
    case, entry = ec.by_name(name), GOLDEN[name]
    lib, e, protein = _lib.load(), encoders[case.alphabet], case.alphabet == "protein"
    path = write_fasta(case, tmp_path)
    # file lengths and original characters as the host reader books them
    arr = (ctypes.c_char_p * 1)(path.encode())
    ptr, n = ctypes.c_void_p(), ctypes.c_uint64()
    dptr, dlen = ctypes.c_void_p(), ctypes.c_uint64()
    info = EncInfo()
    err = ctypes.create_string_buffer(2048)
    assert host.gtamd_encode_files_info(arr, 1, int(protein), ctypes.byref(ptr), ctypes.byref(n),
                                        ctypes.byref(dptr), ctypes.byref(dlen), ctypes.byref(info),
                                        err, 2048) == 0, err.value
    try:
        read = np.ctypeslib.as_array(ctypes.cast(ptr, ctypes.POINTER(ctypes.c_uint8)), shape=(n.value,))
        assert np.array_equal(read, case.enc)
        assert _set(lib, e, case.enc) == 0, lib.gtamd_esa_last_error()
        for sat in entry["sat"]:
            idx = str(tmp_path / ("idx-" + sat))
            ss = device_writer(e, protein, idx, sat, os.path.basename(path).encode(), info)
            check_against_golden(entry, sat, idx, ss)
    finally:
        host.gtamd_encinfo_free(ctypes.byref(info))
        libc = ctypes.CDLL(None)
        libc.free(ptr)
        libc.free(dptr)


# ---- refusals and reuse ------------------------------------------------------------
def _refused_everywhere(lib, e):
    """what a failed set_symbols leaves: no length, no section"""
    assert lib.gtamd_encoder_length(e) == 0
    assert not lib.gtamd_encoder_device_symbols(e)
    a, b = _guarded(64), _guarded(64)
    calls = [lambda: lib.gtamd_encoder_pack_twobit(e, 1, 0, a.ctypes.data, 65),
             lambda: lib.gtamd_encoder_pack_specialbits(e, a.ctypes.data, 65),
             lambda: lib.gtamd_encoder_pack_bytecompress(e, a.ctypes.data, 65 * 8),
             lambda: lib.gtamd_encoder_get_wildcard_runs(e, a.ctypes.data, b.ctypes.data, 65),
             lambda: lib.gtamd_encoder_get_separators(e, a.ctypes.data, 65),
             lambda: lib.gtamd_encoder_copy_symbols(e, a.ctypes.data, 0, 0),
             lambda: lib.gtamd_encoder_get_summary(e, ctypes.byref(EncodeSummary()))]
    for call in calls:
        assert call() == -1
        assert lib.gtamd_esa_last_error() == NOT_FINISHED
    assert (a == GUARD).all() and (b == GUARD).all()


def test_empty_sequences_are_refused_and_the_encoder_lives_on(encoders):
    lib, e = _lib.load(), encoders["dna"]
    good = ec.by_name("h-three-ends-dna")
    bad = {"at 0": (40, (0,)), "at n-1": (40, (39,)), "doubled at (255, 256)": (600, (255, 256)),
           "doubled at (4095, 4096)": (8200, (4095, 4096)), "doubled inside a thread": (100, (5, 6)),
           "at n-1 of a full tile": (4096, (4095,)), "alone": (1, (0,))}
    for what, (n, sep) in bad.items():
        enc = ec.letters(n, 4)
        enc[list(sep)] = 255
        assert ref.first_empty_sequence(enc) is not None
        assert _set(lib, e, enc) == -1, what
        assert lib.gtamd_esa_last_error() == EMPTY_SEQUENCE, what
        _refused_everywhere(lib, e)
        # the next good input on the same object
        assert _set(lib, e, good.enc) == 0, what
        check_summary(lib, e, good)
        check_sections(lib, e, good)
    # no symbol at all, in the words of summarise()
    assert _set(lib, e, np.zeros(0, dtype=np.uint8)) == -1
    assert lib.gtamd_esa_last_error() == b"file '(symbols)' contains an empty sequence"
    _refused_everywhere(lib, e)
    assert lib.gtamd_encoder_set_symbols(e, None, 5) == -1
    assert lib.gtamd_esa_last_error() == b"invalid argument to gtamd_encoder_set_symbols"
    assert _set(lib, e, good.enc) == 0
    check_sections(lib, e, good)


def test_one_encoder_for_one_input_after_another(gpu, tmp_path):
    """a long input, a shorter one, a FASTA file through the reader, symbols again,
    a FASTQ file, symbols again: nothing of an earlier input shows in a later one"""
    lib = gpu
    long_, short = ec.by_name("d-run65536-dna"), ec.by_name("c-both-n33-dna")
    filed = ec.by_name("f-period3-n4097-dna")
    with encode.DeviceEncoder() as de:
        assert de.file_lengths() == [] and de.length == 0
        for case in (long_, short):
            assert _set(lib, de._enc, case.enc) == 0
            check_summary(lib, de._enc, case)
            check_sections(lib, de._enc, case)
            assert de.descriptions() == [] and de.file_lengths() == []
            assert np.array_equal(de.symbols(), case.enc)
        path = write_fasta(filed, tmp_path)
        de.encode([path])
        assert np.array_equal(de.symbols(), filed.enc)
        assert len(de.descriptions()) == de.summary()["numofsequences"] == 1366
        assert de.descriptions()[1] == b"seq1 of f-period3-n4097-dna"
        assert sum(de.summary()["originaldistribution"]) == 4097 - 1365
        assert de.file_lengths() == [(os.path.getsize(path), 4097)]
        for case in (short, long_):
            assert _set(lib, de._enc, case.enc) == 0
            check_summary(lib, de._enc, case)          # (no original character left over)
            check_sections(lib, de._enc, case)
            # no description is left; the input file is forgotten, and asking for
            # its lengths is refused
            assert lib.gtamd_encoder_num_descriptions(de._enc) == 0 and de.descriptions() == []
            with pytest.raises(EsaError, match="no input file 0"):
                de.file_lengths()
        # FASTQ records of an earlier input do not outlive it either
        fq = tmp_path / "two.fastq"
        fq.write_bytes(b"@a\nACGT\n+\nIIII\n@b\nNNA\n+\nIII\n")
        de.encode([str(fq)])
        assert de.fastq_records()[1].tolist() == [4, 3]
        assert _set(lib, de._enc, short.enc) == 0
        check_summary(lib, de._enc, short)
        assert lib.gtamd_encoder_num_fastq_records(de._enc) == 0
        assert all(a.size == 0 for a in de.fastq_records())
