"""The multi-key packing key switch replayed on the host (no GPU): the digit with its rounding offset, the box source index
and sign and the prefix rule of the negacyclic extension (torus-fhe_amd/csrc/thfhe_mk_pack.h) -- what mk_pack_rows_kernel and mk_pack_boxes_kernel
call -- run thread by thread (tests/emu/mk_pack_emu.cpp, compiled here) against the numpy model of tests/mk_pack_reference.py, which sums explicit
monomial products."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mk_pack_reference as MP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
i32p, i64p = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
EXTREME = np.array([0x7FFFFFFF, -0x80000000, -1, 0, 1, 0x7FFFFFFE, -0x7FFFFFFF], np.int64).astype(np.int32)   # 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF, ...


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("mk_pack_emu") / "libmk_pack_emu.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, os.path.join(ROOT, "tests", "emu", "mk_pack_emu.cpp")], check=True)
    L = C.CDLL(so)
    L.mk_pack_emu_digits.argtypes = [i32p, C.c_long, C.c_int, C.c_int, i32p]
    L.mk_pack_emu_digits.restype = None
    L.mk_pack_emu_rows.argtypes = [i32p, C.c_long, i64p, C.c_int, C.c_int, C.c_int, C.c_int, i64p]
    L.mk_pack_emu_rows.restype = None
    L.mk_pack_emu_boxes.argtypes = [C.c_int, i64p, C.c_int, i64p, i64p]
    L.mk_pack_emu_boxes.restype = C.c_int
    return L


def _digits(emu, a, t, basebit):
    a = np.ascontiguousarray(a, np.int32)
    d = np.zeros((a.shape[0], t), np.int32)
    emu.mk_pack_emu_digits(a.ctypes.data_as(i32p), a.shape[0], t, basebit, d.ctypes.data_as(i32p))
    return d


@pytest.mark.parametrize("t,basebit", [(8, 2), (4, 3), (16, 2), (5, 1), (32, 1), (8, 4), (1, 1), (12, 1)])
def test_digits_with_the_rounding_offset(emu, t, basebit):
    # t basebit = 32 has no offset; 0x7FFFFFFF / 0xFFFFFFFF carry into (and out of) the top digit, the sum wrapping mod 2^32
    rng = np.random.default_rng(100 * t + basebit)
    a = np.concatenate([EXTREME, rng.integers(-2**31, 2**31, 4000, dtype=np.int64).astype(np.int32)])
    d = _digits(emu, a, t, basebit)
    assert np.array_equal(d, MP.digits(a, t, basebit))
    # the digits are those of the nearest multiple of 2^(32 - t basebit), ties upward, mod 2^32 -- written out independently of the model
    bt = t * basebit
    near = ((a.astype(np.int64) & 0xFFFFFFFF) + (0 if bt >= 32 else 1 << (31 - bt))) >> (32 - bt) & ((1 << bt) - 1)
    assert np.array_equal(sum(d[:, p].astype(np.int64) << (bt - (p + 1) * basebit) for p in range(t)), near)
    if bt < 32:
        assert not d[3].any() and not d[2].any()     # 0 and 0xFFFFFFFF (which rounds up and wraps): no key row at all
        assert d[0, 0] == (1 << basebit) >> 1        # 0x7FFFFFFF rounds up to 0x80000000: the top bit alone
        assert not d[0, 1:].any()


@pytest.mark.parametrize("N,D,t,basebit,count", [(1024, 9, 8, 2, 6), (1024, 5, 5, 1, 4), (2048, 4, 2, 2, 5), (4096, 3, 1, 2, 1), (1024, 7, 4, 3, 9)])
def test_row_sums_equal_the_model(emu, N, D, t, basebit, count):
    rng = np.random.default_rng(N + D + count)
    R = (1 << basebit) - 1
    pk = rng.integers(-2**63, 2**63, (D, t, R, 2, N), dtype=np.int64)
    recs = rng.integers(-2**31, 2**31, (count, D + 1), dtype=np.int64).astype(np.int32)
    recs[0, :D] = 0                                   # every digit zero: T = (0, b 2^32)
    if count > 1:
        recs[1, :min(D, len(EXTREME))] = EXTREME[:min(D, len(EXTREME))]
    T = np.zeros((count, 2, N), np.int64)
    emu.mk_pack_emu_rows(recs.ctypes.data_as(i32p), count, pk.ctypes.data_as(i64p), D, t, basebit, N, T.ctypes.data_as(i64p))
    assert np.array_equal(T, MP.pack_rows(recs, pk, t, basebit))
    if t * basebit < 32:
        assert not T[0, 0].any() and not T[0, 1, 1:].any() and T[0, 1, 0] == int(recs[0, D]) << 32


@pytest.mark.parametrize("N", [1024, 2048, 4096])
@pytest.mark.parametrize("p", [2, 8, 64])
def test_boxes_equal_the_sum_of_monomial_products(emu, N, p):
    rng = np.random.default_rng(N + p)
    T = rng.integers(-2**63, 2**63, (p, 2, N), dtype=np.int64)
    a, b = np.zeros(N, np.int64), np.zeros(N, np.int64)
    assert emu.mk_pack_emu_boxes(N, T.ctypes.data_as(i64p), p, a.ctypes.data_as(i64p), b.ctypes.data_as(i64p)) == 1
    ra, rb = MP.pack_boxes(T, p)
    assert np.array_equal(a, ra[0]) and np.array_equal(b, rb[0])


@pytest.mark.parametrize("N,p", [(1024, 2), (1024, 64), (2048, 4), (4096, 2), (4096, 64)])
def test_trivial_records_give_the_plain_test_vector(emu, N, p):
    from thfhe import lut
    rng = np.random.default_rng(7 * N + p)
    v = rng.integers(-2**31, 2**31, p, dtype=np.int64)
    T = np.zeros((p, 2, N), np.int64)
    T[:, 1, 0] = v << 32
    a, b = np.ones(N, np.int64), np.zeros(N, np.int64)
    assert emu.mk_pack_emu_boxes(N, T.ctypes.data_as(i64p), p, a.ctypes.data_as(i64p), b.ctypes.data_as(i64p)) == 1
    assert not a.any() and np.array_equal(b, lut.test_vector(v << 32, p, N=N, torus_bits=64))
