"""`gt-suffixerator-amd readjoiner correct` without a device: the option parser,
its defaults and refusals, -help, the dispatcher's unchanged answers, the
refusal of a sequence file that is not of the equal-length access type, and the
in-place patch of an INDEX.esq from a list of (position, letter): only the 2-bit
words and the character distribution change, and the file decodes to the edited
reads."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import kcorrect_reference as kr
from genometools_amd import _lib
from test_esq_sections_reference import write_from_memory
from test_host import host  # noqa: F401  (fixture)

CLI = os.path.join(_lib.HERE, "gt-suffixerator-amd")
SENTENCE = "twobitencoding correction is currently only implemented if the sequence access type is EQUALLENGTH"


def _error(*args):
    p = subprocess.run([CLI, "readjoiner", "correct"] + list(args), capture_output=True, text=True)
    assert p.returncode == 1 and p.stdout == "" and p.stderr.startswith("gt readjoiner correct: error: ")
    return p.stderr[len("gt readjoiner correct: error: "):].rstrip("\n")


def test_help():
    p = subprocess.run([CLI, "readjoiner", "correct", "-help"], capture_output=True, text=True)
    assert p.returncode == 0 and p.stderr == ""
    assert p.stdout.startswith("Usage: gt-suffixerator-amd readjoiner correct -ii INDEX [-k K] [-c C]")
    for words in ("default: 31", "default: 3", "in place", "left alone"):
        assert words in p.stdout


def test_option_parser():
    assert _error("-k", "12") == 'option "-ii" is mandatory'
    assert _error("-ii") == 'missing argument to option "-ii"'
    assert _error("-ii", "x", "-k") == 'missing argument to option "-k"'
    assert _error("-ii", "x", "-k", "0") == 'argument to option "-k" must be an integer >= 1'
    assert _error("-ii", "x", "-c", "0") == 'argument to option "-c" must be an integer >= 1'
    assert _error("-ii", "x", "-c", "two") == 'argument to option "-c" is out of range'
    assert "255 at most" in _error("-ii", "x", "-k", "256")
    assert "255 at most" in _error("-ii", "x", "-k", "100000")
    assert _error("-ii", "nothere", "-k", "255") == "cannot open file 'nothere.prj'"
    assert _error("-ii", "nothere") == "cannot open file 'nothere.prj'"
    for name in ("-encseq", "-dbg"):
        assert name in _error("-ii", "x", name) and "not supported" in _error("-ii", "x", name)
    assert _error("-ii", "x", "-nosuch").startswith("unknown option: -nosuch")


def test_the_dispatcher_answers_as_before():
    for args in (["readjoiner"], ["readjoiner", "assembly"], ["readjoiner", "prefilter"], ["readjoiner", "correct"]):
        p = subprocess.run([CLI] + args, capture_output=True, text=True)
        assert (p.returncode, p.stdout, p.stderr) == (1, "", "gt readjoiner: error: tool overlap expected\n")


def _patch(host, idx, positions, letters):
    host.gtamd_correct_patch_esq.argtypes = [ctypes.c_char_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64,
                                             ctypes.c_char_p, ctypes.c_size_t]
    positions = np.ascontiguousarray(positions, dtype=np.uint64)
    letters = np.ascontiguousarray(letters, dtype=np.uint8)
    err = ctypes.create_string_buffer(2048)
    rc = host.gtamd_correct_patch_esq(idx.encode(), positions.ctypes.data, letters.ctypes.data, positions.size, err, 2048)
    return rc, err.value.decode()


def _sections(raw, n):
    """(offset of the character distribution, offset of the 2-bit words, their end): a header of memory symbols"""
    words = 2 if n < 32 else 2 + (n - 1) // 32
    end = len(raw)
    return end - 8 * words - 32, end - 8 * words, end


def test_patch_in_place(host, tmp_path):
    rng = np.random.default_rng(5)
    reads = [rng.integers(0, 4, 37, dtype=np.uint8) for _ in range(9)]
    enc = kr.joined(reads)
    idx = str(tmp_path / "reads")
    write_from_memory(host, enc, False, idx, "eqlen")
    with open(idx + ".esq", "rb") as f:
        before = f.read()
    # edits in every place of a 2-bit word, one position twice (the last wins), the first and the last symbol
    positions = [0, 5, 27, 28, 31, 32, 63, 64, 100, 5, enc.size - 1]
    positions = [p for p in positions if enc[p] < 4]
    letters = [int(enc[p] + 1 + i) % 4 for i, p in enumerate(positions)]
    rc, err = _patch(host, idx, positions, letters)
    assert rc == 0, err
    with open(idx + ".esq", "rb") as f:
        after = f.read()
    want = enc.copy()
    for p, x in zip(positions, letters):
        want[p] = x
    dist, twobit, end = _sections(before, enc.size)
    assert len(after) == len(before) and after[:dist] == before[:dist]
    changed = {twobit + 8 * (p // 32) + b for p in positions for b in range(8)}
    assert all(after[i] == before[i] for i in range(twobit, end) if i not in changed)
    # the distribution as the reference's editor keeps it
    count = np.frombuffer(before[dist:dist + 32], dtype=np.uint64).copy()
    assert count.tolist() == np.bincount(enc[enc < 4], minlength=4).tolist()
    cur = enc.copy()
    for p, x in zip(positions, letters):
        count[int(cur[p]) if p % 32 >= 28 else 0] -= 1
        count[x] += 1
        cur[p] = x
    assert np.frombuffer(after[dist:dist + 32], dtype=np.uint64).tolist() == count.tolist()
    # it decodes to the edited reads
    words = np.frombuffer(after[twobit:end], dtype=np.uint64)
    letters_at = np.flatnonzero(enc < 4)
    got = np.array([(int(words[p // 32]) >> (62 - 2 * (p % 32))) & 3 for p in letters_at.tolist()], dtype=np.uint8)
    assert np.array_equal(got, want[letters_at])
    # no edit: nothing is written; an edit beyond the symbols: refused, nothing is written
    assert _patch(host, idx, [], []) == (0, "")
    rc, err = _patch(host, idx, [3, enc.size], [1, 1])
    assert rc == -1 and "position" in err
    rc, err = _patch(host, idx, [3], [4])
    assert rc == -1
    with open(idx + ".esq", "rb") as f:
        assert f.read() == after


def test_another_access_type_is_refused_with_the_reference_s_sentence(host, tmp_path):
    rng = np.random.default_rng(6)
    reads = [rng.integers(0, 4, 30 if i % 2 else 36, dtype=np.uint8) for i in range(12)]
    idx = str(tmp_path / "two")
    write_from_memory(host, kr.joined(reads), False, idx, "uchar")
    with open(idx + ".esq", "rb") as f:
        before = f.read()
    assert _patch(host, idx, [1], [2]) == (-1, SENTENCE)
    with open(idx + ".esq", "rb") as f:
        assert f.read() == before
    with open(idx + ".prj", "w") as f:
        f.write("totallength=%d\nreadmode=0\n" % kr.joined(reads).size)
    assert _error("-ii", idx, "-k", "8", "-c", "2") == SENTENCE


def test_truncated_files_are_refused(host, tmp_path):
    rng = np.random.default_rng(7)
    enc = kr.joined([rng.integers(0, 4, 40, dtype=np.uint8) for _ in range(5)])
    idx = str(tmp_path / "cut")
    write_from_memory(host, enc, False, idx, "eqlen")
    with open(idx + ".esq", "rb") as f:
        raw = f.read()
    for size in (0, 1, 9, 100, len(raw) - 8, len(raw) - 60):
        with open(idx + ".esq", "wb") as f:
            f.write(raw[:size])
        rc, err = _patch(host, idx, [1], [2])
        assert rc == -1 and "no encoded sequence" in err
    assert _patch(host, str(tmp_path / "nothere"), [1], [2])[0] == -1


# ---- the same code under the sanitizers, in a program of its own ----

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_DIR = os.path.join(_lib.HERE, "csrc", "host")
DRIVER_SRC = os.path.join(ROOT, "tests", "correct_san_driver.c")
STD_FLAGS = ["-Wall", "-Wextra", "-std=c99", "-D_POSIX_C_SOURCE=200809L", "-D_DEFAULT_SOURCE",
             "-I" + os.path.join(ROOT, "include"), "-I" + HOST_DIR]
SAN_FLAGS = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan"]
HOST_FILES = tuple(sorted(f for f in os.listdir(HOST_DIR) if f.endswith(".c") and f != "suffixerator_main.c"))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """tests/correct_san_driver.c with every file of the host layer, all under the sanitizers, linked against the
    ordinary libgtamd_esa.so, which is loaded and never asked for a device"""
    out = tmp_path_factory.mktemp("correctsan")
    probe = out / "probe.c"
    probe.write_text("int main(void) { return 0; }\n")
    p = subprocess.run(["gcc"] + SAN_FLAGS + ["-o", str(out / "probe"), str(probe)], capture_output=True, text=True)
    if p.returncode != 0:
        pytest.skip("gcc cannot build a program with -fsanitize=address,undefined -static-libasan here: " + p.stderr[-300:])
    jobs = []
    for src in [os.path.join(HOST_DIR, f) for f in HOST_FILES] + [DRIVER_SRC]:
        obj = str(out / (os.path.basename(src) + ".o"))
        jobs.append((obj, subprocess.Popen(["gcc"] + SAN_FLAGS + STD_FLAGS + ["-c", "-o", obj, src],
                                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
    logs = [(proc.communicate()[0], proc.returncode) for _, proc in jobs]
    assert all(rc == 0 for _, rc in logs), "".join(text for text, _ in logs)
    exe = str(out / "correct_san_driver")
    subprocess.run(["gcc"] + SAN_FLAGS + ["-o", exe] + [obj for obj, _ in jobs] +
                   ["-L" + _lib.HERE, "-lgtamd_esa", "-lpthread", "-lz", "-ldl", "-Wl,-rpath," + _lib.HERE], check=True)
    return exe


def _san_env():
    env = dict(os.environ)
    env["ASAN_OPTIONS"] = "allocator_may_return_null=1:detect_leaks=1"
    env["UBSAN_OPTIONS"] = "print_stacktrace=1"
    return env


def _driven(driver, *args):
    """(rc, message) of the sanitized program; no report, no leak"""
    p = subprocess.run([driver] + [str(a) for a in args], capture_output=True, text=True, env=_san_env())
    assert p.returncode == 0 and "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-4000:]
    rc, _, message = p.stdout.splitlines()[-1].partition("\t")
    return int(rc), message


def test_the_sanitizers_are_awake(driver):
    p = subprocess.run([driver, "canary"], capture_output=True, text=True, env=_san_env())
    assert p.returncode != 0 and "heap-buffer-overflow" in p.stderr


def test_parser_and_patcher_under_the_sanitizers(driver, host, tmp_path):
    assert _driven(driver, "tool", "-k", "12") == (-1, 'option "-ii" is mandatory')
    assert _driven(driver, "tool", "-ii") == (-1, 'missing argument to option "-ii"')
    assert "255 at most" in _driven(driver, "tool", "-ii", "x", "-k", "300")[1]
    assert _driven(driver, "tool", "-ii", str(tmp_path / "nothere"))[0] == -1
    for name in ("-encseq", "-dbg"):
        assert name in _driven(driver, "tool", "-ii", "x", name)[1]
    rng = np.random.default_rng(9)
    enc = kr.joined([rng.integers(0, 4, 37, dtype=np.uint8) for _ in range(9)])
    idx = str(tmp_path / "reads")
    write_from_memory(host, enc, False, idx, "eqlen")
    with open(idx + ".esq", "rb") as f:
        raw = f.read()
    edits = ["%d:%d" % (p, (int(enc[p]) + 1) % 4) for p in (0, 28, 31, 32, 100, 100, enc.size - 1) if enc[p] < 4]
    # the same edits by the sanitized program and by the library give the same file
    assert _driven(driver, "patch", idx, *edits) == (0, "")
    with open(idx + ".esq", "rb") as f:
        sanitized = f.read()
    with open(idx + ".esq", "wb") as f:
        f.write(raw)
    assert _patch(host, idx, [int(e.split(":")[0]) for e in edits], [int(e.split(":")[1]) for e in edits]) == (0, "")
    with open(idx + ".esq", "rb") as f:
        assert f.read() == sanitized and sanitized != raw
    assert _driven(driver, "patch", idx, "%d:1" % enc.size)[0] == -1
    assert _driven(driver, "patch", idx, "3:7")[0] == -1
    for size in sorted({0, 1, 8, 9, 17, 100, 160, len(raw) - 64, len(raw) - 9, len(raw) - 8, len(raw) - 1}):
        with open(idx + ".esq", "wb") as f:
            f.write(raw[:size])
        rc, message = _driven(driver, "patch", idx, "1:2", "%d:3" % (enc.size - 1))
        assert rc == -1 and "no encoded sequence" in message, size
        with open(idx + ".prj", "w") as f:
            f.write("totallength=%d\nreadmode=0\n" % enc.size)
        assert _driven(driver, "tool", "-ii", idx, "-k", "8")[0] == -1
    two = str(tmp_path / "two")
    write_from_memory(host, kr.joined([rng.integers(0, 4, 30 if i % 2 else 36, dtype=np.uint8) for i in range(12)]), False,
                      two, "uchar")
    assert _driven(driver, "patch", two, "1:2") == (-1, SENTENCE)
    with open(two + ".prj", "w") as f:
        f.write("readmode=0\n")
    assert _driven(driver, "tool", "-ii", two) == (-1, SENTENCE)
