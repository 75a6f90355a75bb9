"""Level A of the MSD first sort as one u64 per entry, K1 << 32 | X << 24 | the low
24 bits of the position, and level B bringing the upper bits back from the block
boundaries (genometools_amd/csrc/esa_msd.h, esa_msd_blocks.h).  GTAMD_MSD=1 takes
the MSD sort at every size; every table is checked against the oracle at sizes
around the switch points of the block size L = clamp(ceil(log2 N) - 8, 12, 24),
on texts whose level-B tiles span many blocks, with a digit that only the last
block holds, and for the 5-bit alphabet."""
import numpy as np
import pytest

import engine_paths
import oracle_util as ou
from genometools_amd import esa, synth

pytestmark = pytest.mark.gpu
WILD, SEP = 254, 255


def _assert_same_as_oracle(enc, sigma, res):
    ora = ou.esa(enc, sigma)
    assert np.array_equal(res.suf, ora["suf"]), "suf"
    assert np.array_equal(res.bwt, ora["bwt"]), "bwt"
    assert np.array_equal(res.lcp, ora["lcp"]), "lcp"
    assert np.array_equal(res.llv, ora["llv"]), "llv"
    st = ora["stats"]
    for k in ("longest", "largelcpvalues", "maxbranchdepth", "prefixlength"):
        assert res.stats[k] == st[k], k
    assert res.stats["lcptabsum"] == int(st["lcptabsum"])


def _block_bits(n):
    c = int(n - 1).bit_length()
    return min(24, max(12, c - 8))


@pytest.fixture
def msd(monkeypatch, capfd):
    """GTAMD_MSD=1, and at the end of the test: the MSD sort ran"""
    monkeypatch.setenv("GTAMD_MSD", "1")
    monkeypatch.setenv("GTAMD_DEBUG", "1")
    capfd.readouterr()
    yield monkeypatch
    parts = engine_paths.parse(capfd.readouterr().err)
    assert sorted(parts) == [0] and parts[0]["switches"]["msd"] == 1
    assert parts[0]["run"]["first_sort"] == "msd" and parts[0]["msd"] is not None


# L = 12 (one block up to 4096, then 2..256), 13 at 2^20 + 1, 14 at 2^21 + 1, 15 at 3 * 2^20
@pytest.mark.parametrize("n", [5000, 3 * 4096 + 1, 1 << 20, (1 << 20) + 1, 1 << 21, (1 << 21) + 1,
                               3 << 20])
def test_uniform_dna_at_block_switch_points(gpu, msd, n):
    enc = synth.generate(synth.MODEL_UNIFORM_DNA, 17, n)
    _assert_same_as_oracle(enc, 4, esa.suffixerator_tables(enc, 4))


def _sparse_dna(n, seed):
    """A, C and G only, except: the 4-mer TTTT at a few far-apart places (one
    level-B tile of its parent spans nearly all blocks, most of them empty of it),
    tandem copies of TACG in two far-apart blocks (parents of three tiles, with
    a run of equal boundaries between the two copies), TGTG only in the last
    block, wildcards and separators"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 3, n).astype(np.uint8)
    L = _block_bits(n)
    for p in [100, n // 5, n // 2, n // 2 + 9, (4 * n) // 5, n - (1 << L) - 40]:
        a[p:p + 4] = 3
    tacg = np.tile(np.array([3, 0, 1, 2], dtype=np.uint8), 1500)
    for p in [3000, (3 * n) // 4]:
        a[p:p + tacg.size] = tacg
    a[n - 30:n - 26] = [3, 2, 3, 2]
    a[rng.integers(0, n, n // 4000)] = WILD
    a[rng.integers(0, n, n // 20000)] = SEP
    return a


@pytest.mark.parametrize("n", [(1 << 20) + 1, (1 << 21) + 3])
def test_sparse_digits_span_blocks(gpu, msd, n):
    enc = _sparse_dna(n, n)
    _assert_same_as_oracle(enc, 4, esa.suffixerator_tables(enc, 4))


def test_digit_only_in_last_block(gpu, msd):
    """G only in the last 2000 symbols: the parents that start with it have every
    boundary but the ones behind the text at their start"""
    n = (1 << 20) + 777
    rng = np.random.default_rng(5)
    a = rng.integers(0, 4, n).astype(np.uint8)
    a[:n - 2000][a[:n - 2000] == 2] = 1
    _assert_same_as_oracle(a, 4, esa.suffixerator_tables(a, 4))


@pytest.mark.parametrize("n", [70001, (1 << 20) + 1])
def test_protein(gpu, msd, n):
    """the 5-bit alphabet (X: 6 bits); letter 19 in a few far-apart blocks only"""
    enc = synth.generate(synth.MODEL_PROTEIN, 9, n).copy()
    enc[enc == 19] = 18
    for p in [10, n // 3, n // 3 + 2, n - 100]:
        enc[p] = 19
    _assert_same_as_oracle(enc, 20, esa.suffixerator_tables(enc, 20))
