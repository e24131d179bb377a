"""The digit helper of the leveled CMux replayed on the host (no GPU): diff_digits_z (torus-fhe_amd/csrc/thfhe_lane.h)
runs lane by lane over a wavefront (tests/emu/lhe_emu.cpp, compiled here) against oracle_decompose32 of the difference -- random words and the
extreme words -2^31 and 2^31 - 1, for l = 1 .. 4 at the Bgbit values of test_gpu_lut_shapes.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import lhe_reference as LR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 1024
i32p = C.POINTER(C.c_int32)
SHAPES = [(1, 8), (2, 10), (3, 7), (4, 8), (3, 6), (2, 7), (4, 4)]   # (l, Bgbit) of support.SHAPES


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("lhe_emu") / "liblhe_emu.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, os.path.join(ROOT, "tests", "emu", "lhe_emu.cpp")], check=True)
    L = C.CDLL(so)
    L.lhe_emu_diff_digits.argtypes = [i32p, i32p, C.c_int, C.c_int, i32p]
    return L


@pytest.mark.parametrize("l,Bgbit", SHAPES)
def test_digits_of_a_difference_equal_the_oracle_decomposition(emu, O, l, Bgbit):
    rng = np.random.default_rng(100 * l + Bgbit)
    p = O.make_params(n=1, N=N, k=1, l=l, Bgbit=Bgbit, ks_t=8, ks_basebit=2, torus_bits=32, parties=1)
    lo, hi = -2**31, 2**31 - 1
    p1 = rng.integers(lo, hi + 1, N, dtype=np.int64)
    p0 = rng.integers(lo, hi + 1, N, dtype=np.int64)
    # the extreme words, as operands and as differences: -2^31 - (2^31 - 1) wraps to 1, (2^31 - 1) - (-2^31) to -1, x - x = 0, and the
    # differences -2^31 and 2^31 - 1 themselves
    edge = [(lo, hi), (hi, lo), (lo, lo), (hi, hi), (lo, 0), (hi, 0), (0, lo), (0, hi), (0, 0), (-1, 0), (0, 1)]
    for q, (x, y) in enumerate(edge):
        for base in (0, 63, 64, 511, 512, 960):   # every lane role: first / last lane, both halves of the fold
            p1[(base + q) % N], p0[(base + q) % N] = x, y
    p1, p0 = p1.astype(np.int32), p0.astype(np.int32)
    got = np.zeros((l, N), np.int32)
    emu.lhe_emu_diff_digits(p1.ctypes.data_as(i32p), p0.ctypes.data_as(i32p), l, Bgbit, got.ctypes.data_as(i32p))
    diff = (p1.astype(np.int64) - p0.astype(np.int64)).astype(np.uint32).view(np.int32)
    want = LR.decompose(diff, p)
    assert np.array_equal(got, want), np.argwhere(got != want)[:6].tolist()
    assert np.abs(got).max() <= 1 << (Bgbit - 1)
