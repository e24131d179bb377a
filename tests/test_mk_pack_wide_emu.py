"""The wide packing-rows kernel replayed on the host (no GPU): mk_pack_rows_wide_kernel's walk over (j, p, digit value)
with its 32-record membership masks (tests/emu/mk_pack_wide_emu.cpp, compiled here, on the helpers of torus-fhe_amd/csrc/thfhe_mk_pack.h) against
the numpy model of tests/mk_pack_reference.py, and the row tiles it fetches against the count the digits predict: one per (group, j, p, value) that
some record of the group has, none where none has."""
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
    so = str(tmp_path_factory.mktemp("mk_pack_wide_emu") / "libmk_pack_wide_emu.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, os.path.join(ROOT, "tests", "emu", "mk_pack_wide_emu.cpp")], check=True)
    L = C.CDLL(so)
    L.mk_pack_wide_emu_rows.argtypes = [i32p, C.c_long, i64p, C.c_int, C.c_int, C.c_int, C.c_int, i64p, C.POINTER(C.c_long)]
    L.mk_pack_wide_emu_rows.restype = None
    return L


def _run(emu, recs, pk, t, basebit):
    recs = np.ascontiguousarray(recs, np.int32)
    count, D, N = recs.shape[0], pk.shape[0], pk.shape[-1]
    T = np.zeros((count, 2, N), np.int64)
    loads = C.c_long(-1)
    emu.mk_pack_wide_emu_rows(recs.ctypes.data_as(i32p), count, pk.ctypes.data_as(i64p), D, t, basebit, N, T.ctypes.data_as(i64p), C.byref(loads))
    return T, loads.value


def _expected_loads(emu, recs, D, t, basebit, N):
    """tiles x the number of (group, j, p, value) with at least one record of the group holding that value"""
    G, tile = emu.mk_pack_wide_emu_group(), emu.mk_pack_wide_emu_tile()
    d = MP.digits(np.asarray(recs)[:, :D], t, basebit)          # [count][D][t]
    n = 0
    for g0 in range(0, d.shape[0], G):
        grp = d[g0:g0 + G]
        n += sum(int(np.any(grp == v, axis=0).sum()) for v in range(1, 1 << basebit))
    return n * (2 * N // tile)


def _key(rng, D, t, basebit, N):
    return rng.integers(-2**63, 2**63, (D, t, (1 << basebit) - 1, 2, N), dtype=np.int64)


def test_group_and_tile_are_the_headers(emu):
    assert emu.mk_pack_wide_emu_group() == 32 and emu.mk_pack_wide_emu_tile() == 256


@pytest.mark.parametrize("N,D,t,basebit,count", [
    (1024, 9, 8, 2, 33),      # a last group with a single record
    (1024, 5, 5, 1, 31),      # one group, not full
    (1024, 3, 32, 1, 32),     # t basebit = 32: no rounding offset
    (1024, 3, 16, 2, 35),     # ... at two-bit digits
    (1024, 3, 8, 4, 64),      # ... at four-bit digits, two full groups
    (2048, 4, 2, 2, 40),
    (4096, 3, 1, 2, 1),
    (1024, 7, 4, 3, 65),
    (1024, 260, 2, 1, 3),     # two chunks of mask words
])
def test_row_sums_equal_the_model(emu, N, D, t, basebit, count):
    rng = np.random.default_rng(N + D + count)
    pk = _key(rng, D, t, basebit, N)
    recs = rng.integers(-2**31, 2**31, (count, D + 1), dtype=np.int64).astype(np.int32)
    if count > 1:
        recs[0, :D] = 0                               # every digit zero: T = (0, b 2^32); a lone record keeps its random words
        recs[1, :min(D, len(EXTREME))] = EXTREME[:min(D, len(EXTREME))]
    if count > 2:
        recs[count - 1, :min(D, len(EXTREME))] = EXTREME[::-1][:min(D, len(EXTREME))]   # the highest record of the last group
    T, loads = _run(emu, recs, pk, t, basebit)
    assert np.array_equal(T, MP.pack_rows(recs, pk, t, basebit))
    assert loads == _expected_loads(emu, recs, D, t, basebit, N)
    if t * basebit < 32 and count > 1:
        assert not T[0, 0].any() and not T[0, 1, 1:].any() and T[0, 1, 0] == int(recs[0, D]) << 32


@pytest.mark.parametrize("basebit", [1, 2, 4])
def test_one_record_or_none_with_a_digit_value(emu, basebit):
    # word j = 0: only record `lone` has a non-zero digit (the top value at p = 0); word j = 1: no record has any; word j = 2: every record has
    # digit 1 at p = 1.  The tiles fetched are exactly those, and only `lone` carries row (0, 0, R - 1).
    N, D, t, G = 1024, 3, 32 // basebit - 1, 32
    R = (1 << basebit) - 1
    rng = np.random.default_rng(basebit)
    pk = _key(rng, D, t, basebit, N)
    for count, lone in ((G, 0), (G, G - 1), (G + 1, G), (2 * G, G + 5)):
        recs = np.zeros((count, D + 1), np.int32)
        recs[:, D] = rng.integers(-2**31, 2**31, count)
        recs[lone, 0] = np.int64(R << (32 - basebit)).astype(np.int32)
        recs[:, 2] = 1 << (32 - 2 * basebit)
        T, loads = _run(emu, recs, pk, t, basebit)
        assert np.array_equal(T, MP.pack_rows(recs, pk, t, basebit)), (count, lone)
        groups = (count + G - 1) // G
        assert loads == (1 + groups) * (2 * N // 256), (count, lone)
        others = np.delete(np.arange(count), lone)
        body = (recs[:, D].astype(np.int64) << 32)
        base = T.copy()
        base[:, 1, 0] -= body
        assert all(np.array_equal(base[i], base[others[0]]) for i in others)                      # the shared row only
        diff = (base[lone].view(np.uint64) - base[others[0]].view(np.uint64)).view(np.int64)
        assert np.array_equal(diff, (np.uint64(0) - pk[0, 0, R - 1].view(np.uint64)).view(np.int64))
