"""The position bits level A of the MSD first sort leaves out, brought back at
level B (genometools_amd/csrc/esa_msd_blocks.h) -- on the CPU: the header's
functions compiled with g++ and run over a level A restated in numpy (stable
partition of text order by an 8-bit digit, per-tile histograms of 4096 entries,
their column scan), every level-B tile of every parent, against the positions
the partition put there and against the definition  block = max{k: bnd[k] <= i}."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import oracle_util as ou

ROOT = ou.ROOT
SHIM_SRC = os.path.join(ROOT, "tests", "msd_blocks_shim.cpp")
HEADER = os.path.join(ROOT, "genometools_amd", "csrc", "esa_msd_blocks.h")
SHIM = os.path.join(ROOT, "oracle", "_build", "libmsd_blocks_shim.so")
TILE = 4096
P_U32 = ctypes.POINTER(ctypes.c_uint32)


@pytest.fixture(scope="module")
def shim():
    os.makedirs(os.path.dirname(SHIM), exist_ok=True)
    if (not os.path.exists(SHIM) or
            max(os.path.getmtime(SHIM_SRC), os.path.getmtime(HEADER)) > os.path.getmtime(SHIM)):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-shared", "-fPIC", "-o", SHIM,
                        SHIM_SRC], check=True)
    lib = ctypes.CDLL(SHIM)
    lib.msd_shim_block_bits.argtypes = [ctypes.c_uint64]
    lib.msd_shim_block_bits.restype = ctypes.c_int
    lib.msd_shim_recover.argtypes = [P_U32, ctypes.c_uint32, ctypes.c_uint32, P_U32, ctypes.c_int,
                                     P_U32]
    lib.msd_shim_recover.restype = ctypes.c_uint32
    return lib


def _ptr(a):
    return a.ctypes.data_as(P_U32)


def _block_bits(n):
    c = max(0, int(n - 1).bit_length()) if n > 1 else 0     # ceil(log2 n)
    return min(24, max(12, c - 8))


def _level_a(digits, L):
    """level-A order (positions), parent starts and the boundary table"""
    n = digits.size
    nt = -(-n // TILE)
    tile_of = np.arange(n) // TILE
    hist = np.zeros((nt, 256), dtype=np.int64)
    np.add.at(hist, (tile_of, digits), 1)
    starts = np.concatenate([[0], np.cumsum(hist.sum(axis=0))])
    scanned = starts[:256][None, :] + np.cumsum(hist, axis=0) - hist
    order = np.argsort(digits, kind="stable").astype(np.uint32)
    bnd = np.empty((256, 256), dtype=np.uint32)
    for k in range(256):
        t = k << (L - 12)
        bnd[:, k] = scanned[t] if t < nt else starts[1:]
    return order, starts, bnd


def _check(shim, digits):
    n = digits.size
    L = _block_bits(n)
    assert shim.msd_shim_block_bits(n) == L
    assert -(-n // (1 << L)) <= 256
    order, starts, bnd = _level_a(digits, L)
    low = order & np.uint32(0xFFFFFF)
    out = np.empty(TILE, dtype=np.uint32)
    spans = 0
    for d in range(256):
        row = np.ascontiguousarray(bnd[d])
        b, e = int(starts[d]), int(starts[d + 1])
        # the definition, for every entry of the parent
        idx = np.arange(b, e, dtype=np.uint64)
        blk = np.searchsorted(row.astype(np.uint64), idx, side="right") - 1
        assert np.array_equal(blk, order[b:e] >> L), d
        for s in range(b, e, TILE):
            v = min(TILE, e - s)
            lo = np.ascontiguousarray(low[s:s + v])
            kb0 = shim.msd_shim_recover(_ptr(row), s, v, _ptr(lo), L, _ptr(out))
            assert kb0 == int(order[s]) >> L
            assert np.array_equal(out[:v], order[s:s + v]), (d, s)
            spans += (int(order[s + v - 1]) >> L) - kb0
    return spans


@pytest.mark.parametrize("n", [64, 4095, 4096, 4097, 5000, 7 * TILE, 1 << 20, (1 << 20) + 1,
                               (1 << 21) + 1, 3 << 20])
def test_uniform_digits(shim, n):
    rng = np.random.default_rng(n)
    _check(shim, rng.integers(0, 256, n).astype(np.int64))


@pytest.mark.parametrize("n", [(1 << 20) + 1, (1 << 21) + 7])
def test_sparse_and_skewed_digits(shim, n):
    """digit 7 in a few far-apart blocks only (tiles that span many blocks, most of
    them empty of it), digit 9 in the last block only, digit 11 in two clusters of
    two tiles each, digit 0 most of the text; the rest absent or rare"""
    rng = np.random.default_rng(n + 3)
    dg = np.where(rng.random(n) < 0.7, 0, rng.integers(12, 200, n)).astype(np.int64)
    L = _block_bits(n)
    far = [1000, n // 3, n // 3 + 5, (2 * n) // 3, n - (1 << L) - 3]
    dg[far] = 7
    dg[n - 20:n - 2] = 9
    dg[5000:5000 + 2 * TILE:2] = 11
    dg[n - (1 << L) - 4 * TILE:n - (1 << L)] = 11
    spans = _check(shim, dg)
    assert spans >= 4                # some tile did cross blocks


def test_one_digit(shim):
    """every entry in one parent: its tiles are the text's tiles"""
    _check(shim, np.full((1 << 20) + 5, 200, dtype=np.int64))


def test_block_bits(shim):
    for n in [1, 2, 64, 4096, (1 << 20) - 1, 1 << 20, (1 << 20) + 1, 1 << 25, (1 << 25) + 1,
              3 * 10 ** 9, (1 << 32) - 1, 1 << 32]:
        L = shim.msd_shim_block_bits(n)
        assert L == _block_bits(n), n
        assert -(-n // (1 << L)) <= 256 and (1 << L) % TILE == 0
