"""Variant "x" of the lane code (torus-fhe_amd/csrc/thfhe_lane.h: the ring kernel's folded transforms around the exchange of register bits (2, 1, 0)
with lane bits (3, 5, 4), unmasked in the inverse) replayed on the host by tests/emu/exchange_emu.cpp, compiled here -- no GPU.  The exchange is
modelled move by move (DPP row_ror:8 with its bank mask, the two lane swaps).  Forward and inverse against the table form within the derived error
(the exchange moves signs and the order of a butterfly's two outputs, so the sums of "f" hold unchanged), forward -> product
with a key in ITS order -> inverse -> rounded limbs word for word against the exact negacyclic product, on random inputs and on the crafted CMux of
tests/bound_inputs.py with every limb sum at the bound, and the same replay as a stand-alone program under ASan + UBSan."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bound_inputs as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "emu", "exchange_emu.cpp")
U = 2.0**-53
# forward "f" / "x" 55u, inverse 54u, table form 25.5u (its inverse is the mirror of its forward: three plain passes and the
# same two table products); a CMux's inverse outputs are within CMUX_ERR * u * (rows N 2^(Bgbit-1) 2^15) of the integer limb sums
ETA_FWD_X, ETA_INV_X, ETA_TABLE, CMUX_ERR = 55.0, 54.0, 25.5, 4104.0
MOVES_FWD, MOVES_INV = 72, 48   # vector instructions of one exchange: 8 kept copies + 32 masked moves + 32 swaps | 16 unmasked moves + 32 swaps


@pytest.fixture(scope="module")
def E(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("exchange_emu") / "libexchange_emu.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, SRC], check=True)
    L = C.CDLL(so)
    L.exch_polymul.restype = C.c_double
    L.exch_mux_rotate.restype = C.c_double
    return L


def dptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def spectrum(z):
    """P_k = sum_j z_j zeta^(j(4k+1)) at the natural positions: [nu = k1 + 8 k0][register k2] holds k = k0 + 8 k1 + 64 k2."""
    k = np.arange(512)
    P = (np.exp(1j * (np.outer(4 * k + 1, np.arange(512)) % 2048) * (np.pi / 1024)) * z[None, :]).sum(axis=1)
    nu, k2 = np.meshgrid(np.arange(64), np.arange(8), indexing="ij")
    return P[(nu >> 3) + 8 * (nu & 7) + 64 * k2]


def test_lane_map_is_a_bijection_that_keeps_read_groups_on_one_row():
    lane = np.arange(64)
    nu = (lane & 7) | ((lane & 8) << 2) | ((lane & 0x30) >> 1)
    assert sorted(nu) == list(range(64))
    # a 16-byte LDS read serves these four 16-lane groups one 256-byte row (64 banks) each: the key read B[m * 64 + nu] must cover every 16-byte
    # column of the row exactly once per group
    groups = [list(range(0, 4)) + list(range(12, 16)) + list(range(20, 28)), list(range(4, 12)) + list(range(16, 20)) + list(range(28, 32))]
    groups += [[l + 32 for l in g] for g in groups]
    for g in groups:
        assert sorted(nu[g] % 16) == list(range(16))


@pytest.mark.parametrize("case", ["gauss", "digits10", "coherent"])
def test_forward_and_inverse_match_the_table_form_and_the_definition(E, case):
    rng = np.random.default_rng(60)
    if case == "gauss":
        z = rng.standard_normal(512) + 1j * rng.standard_normal(512)
    elif case == "digits10":
        z = rng.integers(-512, 512, 512) + 1j * rng.integers(-512, 512, 512)
    else:
        z = np.full(512, -512 - 512j)
    zin = np.ascontiguousarray(np.stack([z.real, z.imag], -1)).ravel()
    out, back, norms = np.zeros(64 * 8 * 2), np.zeros(1024), np.zeros(4)
    E.exch_fwd_raw(dptr(zin), dptr(out), dptr(back), dptr(norms))
    got = out.reshape(64, 8, 2)
    got = got[..., 0] + 1j * got[..., 1]
    nz = np.sqrt(512.0) * np.linalg.norm(z)            # ||Z||_2 = sqrt(512) ||z||_2
    assert abs(norms[1] - nz) <= 1e-12 * nz
    print("forward x - table, 2-norm:", norms[0], "bound:", (ETA_FWD_X + ETA_TABLE) * U * nz)
    assert norms[0] <= (ETA_FWD_X + ETA_TABLE) * U * nz
    assert np.abs(got - spectrum(z)).max() <= 1e-12 * nz
    assert (norms[2], norms[3]) == (MOVES_FWD, MOVES_INV)
    zb = back.reshape(512, 2)
    assert np.abs((zb[:, 0] + 1j * zb[:, 1]) / 512 - z).max() <= 1e-13 * max(1.0, np.abs(z).max())
    # the inverse alone, on these spectra, against the table form's inverse
    inorms = np.zeros(2)
    E.exch_inv_raw(dptr(out), dptr(inorms))
    print("inverse x - table, 2-norm:", inorms[0], "bound:", (ETA_INV_X + ETA_TABLE) * U * inorms[1])
    assert abs(inorms[1] - 512 * np.linalg.norm(z)) <= 1e-11 * inorms[1]
    assert inorms[0] <= (ETA_INV_X + ETA_TABLE) * U * inorms[1]


@pytest.mark.parametrize("case", ["random7", "random10", "worst_neg", "worst_alt"])
def test_polymul_exact_within_the_derived_error(E, O, case):
    N = 1024
    rng = np.random.default_rng(61)
    if case == "random7":
        a = rng.integers(-64, 64, N); b = rng.integers(-2**31, 2**31, N); bg = 7
    elif case == "random10":
        a = rng.integers(-512, 512, N); b = rng.integers(-2**31, 2**31, N); bg = 10
    elif case == "worst_neg":   # coherent: both limbs of every key word at magnitude 2^15, every digit at -2^9
        a = np.full(N, -512); b = np.full(N, B.extreme_key_word(32)); bg = 10
    else:
        a = 511 * (-1) ** np.arange(N); b = np.full(N, 2**31 - 1); bg = 10
    a = a.astype(np.int32); b = b.astype(np.int32)
    ref, got = np.zeros(N, np.int32), np.zeros(N, np.int32)
    O.lib().oracle_polymul_schoolbook32(O.p32(a), O.p32(b), N, O.p32(ref))
    off = E.exch_polymul(O.p32(a), O.p32(b), O.p32(got))
    print(case, "worst distance from an integer:", off, "bound:", CMUX_ERR * U * B.bound(1, N, bg))
    assert np.array_equal(ref, got)
    assert off <= CMUX_ERR * U * B.bound(1, N, bg)


def test_cmux_bit_exact_on_random_inputs(E, O, sk_small):
    p, K, orc = sk_small
    npolys = K.bk.size // 1024
    spec = np.zeros(npolys * 2 * 512 * 2, np.float64)
    E.exch_transform_key_polys(O.p32(K.bk), C.c_int64(npolys), dptr(spec))
    acc = np.random.default_rng(62).integers(-2**31, 2**31, (2, 1024)).astype(np.int32)
    for i, a in [(0, 1), (3, -1000), (7, 1023), (2, 1024), (15, 2047), (9, 777)]:
        ref = orc.mux_rotate(i, a, acc, schoolbook=True)
        got = acc.copy()
        off = E.exch_mux_rotate(dptr(spec), p.l, p.Bgbit, i, a, O.p32(got))
        assert np.array_equal(ref, got), (i, a)
        assert off <= CMUX_ERR * U * B.bound(2 * p.l, 1024, p.Bgbit)
        acc = ref


@pytest.mark.parametrize("l, Bgbit", [(2, 10), (3, 7), (3, 10)])
def test_cmux_at_the_full_bound(E, O, l, Bgbit):
    # all 2l digit rows at -2^(Bgbit-1) on every coefficient against a key whose every word is 0x7FFF8000: the limb sum at coefficient N - 1 is
    # exactly 2l N 2^(Bgbit-1) 2^15; every output word equals the oracle's (exact products) and every inverse output is within the derived error
    p = O.make_params("SK-128", n=2, l=l, Bgbit=Bgbit)
    K = O.SKKeys(p, 21, 2.0**-25, 2.0**-15)
    bk = K.bk.copy()
    bk[1] = B.extreme_key_word(32)
    orc = O.Oracle(p, bk, K.ksk)
    npolys = bk.size // 1024
    spec = np.zeros(npolys * 2 * 512 * 2, np.float64)
    E.exch_transform_key_polys(O.p32(bk), C.c_int64(npolys), dptr(spec))
    acc = np.full((2, 1024), B.crafted_mu(32, l, Bgbit), np.int32)
    rows = B.step_digit_rows(acc, 1024, 32, l, Bgbit)
    assert len(rows) == 2 * l and all(np.all(d == -2**(Bgbit - 1)) for _, _, d in rows)
    assert B.peak_limb_sum([(d, bk[1, r, 0]) for r, _, d in rows], 32) == B.bound(2 * l, 1024, Bgbit)
    ref = orc.mux_rotate(1, 1024, acc, schoolbook=True)
    got = acc.copy()
    off = E.exch_mux_rotate(dptr(spec), l, Bgbit, 1, 1024, O.p32(got))
    err = CMUX_ERR * U * B.bound(2 * l, 1024, Bgbit)
    print((l, Bgbit), "worst distance from an integer:", off, "bound:", err)
    assert np.array_equal(ref, got)
    assert off <= err < 0.5


def test_replay_is_clean_under_asan_and_ubsan(tmp_path):
    # the replay as a stand-alone host program: forward against the table form, round trip, inverse, the move counts, one product against the
    # schoolbook product; any out-of-bounds access or undefined operation in the lane code aborts it
    exe = str(tmp_path / "exchange_emu_san")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DEXCHANGE_EMU_MAIN", "-o", exe, SRC],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "status 0" in r.stdout
