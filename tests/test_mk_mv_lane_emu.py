"""The multi-value epilogue of the 3-gen multi-key engine replayed on the host (no GPU): extract_mv64
(torus-fhe_amd/csrc/thfhe_lane.h), the body of mk_extract_mv_kernel, run thread by thread over its 256-thread workgroup (tests/emu/mk_mv_emu.cpp,
compiled here) against the model's combination of unconverted extractions -- the index and sign maps of every tap, the sign-extended taps, the bias
on the body word and the one conversion per word, on random int64 words at every ring degree."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mk_mv_lut_reference as MV

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
i32p, i64p = C.POINTER(C.c_int32), C.POINTER(C.c_int64)


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("mk_mv_emu") / "libmk_mv_emu.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, os.path.join(ROOT, "tests", "emu", "mk_mv_emu.cpp")], check=True)
    L = C.CDLL(so)
    L.mk_mv_emu_extract.argtypes = [C.c_int, i64p, i32p, C.c_int, C.c_int, C.c_int64, i32p]
    L.mk_mv_emu_extract.restype = C.c_int
    return L


def _run(emu, N, acc, c, out_bias):
    q, p = c.shape
    out = np.zeros((q, N + 1), np.int32)
    assert emu.mk_mv_emu_extract(N, acc.ctypes.data_as(i64p), c.ctypes.data_as(i32p), p, q, out_bias, out.ctypes.data_as(i32p)) == 1
    return out


@pytest.mark.parametrize("N", [1024, 2048, 4096])
@pytest.mark.parametrize("p,q", [(2, 1), (64, 9), (8, 64)])
def test_epilogue_equals_the_combination_in_torus64(emu, N, p, q):
    rng = np.random.default_rng(1000 * p + q + N)
    acc = rng.integers(-2**63, 2**63, 2 * N, dtype=np.int64)
    c = rng.integers(-2**31, 2**31, (q, p)).astype(np.int32)
    out_bias = int(rng.integers(-2**63, 2**63, dtype=np.int64))
    out = _run(emu, N, acc, c, out_bias)
    assert np.array_equal(out, MV.combine64(acc, c, p, N, out_bias))
    assert not np.array_equal(out, MV.convert_then_combine(acc, c, p, N, out_bias))   # the order is visible on these words


def test_single_tap_is_a_negated_extraction(emu):
    # tap k alone with weight -1: the record is mk_lut_reference.extract_at(acc, J_k) -- the sign map against the older model, tap by tap
    import mk_lut_reference as R
    N, p = 1024, 8
    rng = np.random.default_rng(5)
    acc = rng.integers(-2**63, 2**63, 2 * N, dtype=np.int64)
    c = (-np.eye(p)).astype(np.int32)
    out = _run(emu, N, acc, c, 0)
    for k, J in enumerate(MV.tap_positions(p, N)):
        assert np.array_equal(out[k], R.extract_at(acc, J, N)), k
