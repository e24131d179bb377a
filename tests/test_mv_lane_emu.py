"""The multi-value epilogue of the blind-rotate kernels replayed on the host (no GPU): extract_mv16 and its start
acc_init_tv16 (torus-fhe_amd/csrc/thfhe_lane.h) run lane by lane over a wavefront (tests/emu/mv_emu.cpp, compiled here) against the model's
combination of extractions -- the index and sign maps of every tap at every p, on random words."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import lut_reference as R
import mv_lut_reference as MV
from support import words

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 1024
i32p = C.POINTER(C.c_int32)


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("mv_emu") / "libmv_emu.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, os.path.join(ROOT, "tests", "emu", "mv_emu.cpp")], check=True)
    L = C.CDLL(so)
    L.mv_emu_init.argtypes = [i32p, C.c_int, i32p]
    L.mv_emu_extract.argtypes = [i32p, i32p, C.c_int, C.c_int, i32p]
    return L


@pytest.mark.parametrize("p", [2, 4, 8, 16, 32, 64])
def test_epilogue_equals_the_combination_of_extractions(emu, p):
    rng = np.random.default_rng(p)
    q = {2: 1, 4: 3, 8: 64, 16: 9, 32: 2, 64: 17}[p]
    acc, c = words(rng, 2 * N), words(rng, q, p)
    out = np.zeros((q, N + 1), np.int32)
    emu.mv_emu_extract(acc.ctypes.data_as(i32p), c.ctypes.data_as(i32p), p, q, out.ctypes.data_as(i32p))
    assert np.array_equal(out, MV.combine(acc, c, N))


def test_start_and_epilogue_give_the_product_test_vector_values(emu):
    # (0, X^{-barb} mv_base) through the epilogue with helper-built factors: the body of output j is f_j(m) * step for every amount inside m's box
    from thfhe import lut
    rng = np.random.default_rng(1)
    p, step = 8, 1 << 28
    f = rng.integers(-9, 10, (5, p))
    c, tv0 = lut.mv_factors(f, p), lut.mv_base(step)
    acc, out = np.zeros(2 * N, np.int32), np.zeros((5, N + 1), np.int32)
    for barb in list(range(0, 2 * N, 37)) + [N - 1, N, N + 1, 2 * N - 1, 63, 64, 65]:
        emu.mv_emu_init(acc.ctypes.data_as(i32p), barb, tv0.ctypes.data_as(i32p))
        assert not acc[:N].any() and np.array_equal(acc[N:], R.monomial(tv0, -barb, N))
        emu.mv_emu_extract(acc.ctypes.data_as(i32p), c.ctypes.data_as(i32p), p, 5, out.ctypes.data_as(i32p))
        assert not out[:, :N].any()
        for j in range(5):
            want = R.monomial(lut.test_vector(R.to_i32(f[j] * step), p), -barb, N)[0]
            assert out[j, N] == want, (barb, j)
