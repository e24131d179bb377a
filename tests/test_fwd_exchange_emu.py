"""Variant "p" of the lane code (torus-fhe_amd/csrc/thfhe_lane.h: the ring kernel's forward transform with the UNMASKED lane-bit-3 exchange stage, over
a key copy whose spectra at the points with bit 5 of nu set are those of X^32 b) replayed on the host by tests/emu/fwd_exchange_emu.cpp, compiled
here -- no GPU.  The exchange is modelled move by move (16 unmasked DPP row_ror:8 moves, the two lane swaps).  Forward against the table form of p
at the plain points and of X^(-32) p at the phased ones within the derived error (signs, a conjugate of unit modulus and the
order of a butterfly's two outputs, so the sums of "f" hold), the phased key against rho^32 B, products and whole CMuxes word for word against the
form it replaces and against the exact oracle, the crafted CMux with every limb sum at the bound, the negative control (limbs split AFTER rotating
the words), and the same replay as a stand-alone program under ASan + UBSan."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bound_inputs as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "emu", "fwd_exchange_emu.cpp")
U = 2.0**-53
# forward "f" / "x" / "p" 55u, table form 25.5u, the key transform ("s") 37u; a CMux's inverse outputs are within
# CMUX_ERR * u * (rows N 2^(Bgbit-1) 2^15) of the integer limb sums
ETA_FWD_P, ETA_TABLE, ETA_KEY, CMUX_ERR = 55.0, 25.5, 37.0, 4104.0
MOVES_FWD = 48   # vector instructions of the exchange: 16 unmasked moves + 32 swaps
PHASE = 32


@pytest.fixture(scope="module")
def E(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("fwd_exchange_emu") / "libfwd_exchange_emu.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, SRC], check=True)
    L = C.CDLL(so)
    for f in ("exch_polymul", "exch_mux_rotate", "fxe_polymul", "fxe_mux_rotate"):
        getattr(L, f).restype = C.c_double
    return L


def dptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def spectrum(z):
    """P_k = sum_j z_j zeta^(j(4k+1)) at the natural positions: [nu = k1 + 8 k0][register k2] holds k = k0 + 8 k1 + 64 k2."""
    k = np.arange(512)
    P = (np.exp(1j * (np.outer(4 * k + 1, np.arange(512)) % 2048) * (np.pi / 1024)) * z[None, :]).sum(axis=1)
    nu, k2 = np.meshgrid(np.arange(64), np.arange(8), indexing="ij")
    return P[(nu >> 3) + 8 * (nu & 7) + 64 * k2]


def rho_pow(e):
    """rho^e at [nu][k2], rho = zeta^(4k+1)"""
    nu, k2 = np.meshgrid(np.arange(64), np.arange(8), indexing="ij")
    k = (nu >> 3) + 8 * (nu & 7) + 64 * k2
    return np.exp(1j * ((e * (4 * k + 1)) % 2048) * (np.pi / 1024))


def key_spectra(E, O, bk, split_after_rotate=0):
    npolys = bk.size // 1024
    plain, ring = np.zeros(npolys * 2 * 512 * 2), np.zeros(npolys * 2 * 512 * 2)
    E.fxe_transform_key_polys(O.p32(bk), C.c_int64(npolys), dptr(plain), dptr(ring), split_after_rotate)
    return plain, ring


@pytest.mark.parametrize("case", ["gauss", "digits10", "coherent"])
def test_forward_matches_the_table_form_of_p_and_of_the_rotated_p(E, case):
    rng = np.random.default_rng(70)
    if case == "gauss":
        z = rng.standard_normal(512) + 1j * rng.standard_normal(512)
    elif case == "digits10":
        z = rng.integers(-512, 512, 512) + 1j * rng.integers(-512, 512, 512)
    else:
        z = np.full(512, -512 - 512j)
    zin = np.ascontiguousarray(np.stack([z.real, z.imag], -1)).ravel()
    out, norms = np.zeros(64 * 8 * 2), np.zeros(6)
    E.fxe_fwd_raw(dptr(zin), dptr(out), dptr(norms))
    got = out.reshape(64, 8, 2)
    got = got[..., 0] + 1j * got[..., 1]
    nz = np.sqrt(512.0) * np.linalg.norm(z)            # ||Z||_2 = sqrt(512) ||z||_2 over all 512 points; the rotation is unitary
    print("forward p - table, plain points:", norms[0], "phased points:", norms[2], "bound:", (ETA_FWD_P + ETA_TABLE) * U * nz)
    assert np.hypot(norms[1], norms[3]) == pytest.approx(nz, rel=1e-12)
    assert np.hypot(norms[0], norms[2]) <= (ETA_FWD_P + ETA_TABLE) * U * nz
    # against the definition: P at the points with bit 5 of nu clear, rho^(-32) P at the others
    phased = (np.arange(64) & 32) != 0
    want = spectrum(z)
    want[phased] *= rho_pow(-PHASE)[phased]
    assert np.abs(got - want).max() <= 1e-12 * nz
    if case != "coherent":   # the control: the phased points do NOT hold the plain spectrum (the coherent input's spectrum has one large point only)
        assert norms[5] > 0.1 * norms[3]
    assert norms[4] == MOVES_FWD


@pytest.mark.parametrize("case", ["random", "worst_pos", "worst_neg", "worst_alt"])
def test_phased_key_is_rho32_times_the_plain_key(E, O, case):
    rng = np.random.default_rng(71)
    if case == "random":
        b = rng.integers(-2**31, 2**31, 1024)
    elif case == "worst_pos":          # both limbs of every word at magnitude 2^15: (-2^15, +2^15)
        b = np.full(1024, B.extreme_key_word(32))
    elif case == "worst_neg":          # (-2^15, -2^15 + 1): the most negative word with lo = -2^15
        b = np.full(1024, -2**31 - 2**15 + 2**16)
    else:
        b = np.where(np.arange(1024) % 2 == 0, B.extreme_key_word(32), -2**31 - 2**15 + 2**16)
    b = b.astype(np.int64).astype(np.int32)
    norms = np.zeros(3)
    E.fxe_key_phase_check(O.p32(b), dptr(norms))
    # the key bound: a key transform's spectra are within 37u ||B|| of the exact ones.  Here two of them meet, the transform of the rotated limb
    # polynomial and rho^32 times the transform of the plain one, both of 2-norm ||B|| (the rotation is unitary, the 1/512 exact)
    print(case, "phased key - rho^32 B, 2-norm:", norms[0], "bound:", 2 * ETA_KEY * U * norms[1])
    lo = ((b.astype(np.int64) + 2**15) % 2**16) - 2**15
    hi = (b.astype(np.int64) - lo) >> 16
    assert np.abs(lo).max() <= 2**15 and np.abs(hi).max() <= 2**15
    assert norms[1] == pytest.approx(np.sqrt((lo.astype(float)**2).sum() + (hi.astype(float)**2).sum()) / np.sqrt(512.0), rel=1e-12)
    assert norms[0] <= 2 * ETA_KEY * U * norms[1]
    assert norms[2] == 0.0


@pytest.mark.parametrize("case", ["random7", "random10", "worst_neg", "worst_alt"])
def test_polymul_word_for_word_with_the_current_form_and_the_oracle(E, O, case):
    N = 1024
    rng = np.random.default_rng(72)
    if case == "random7":
        a = rng.integers(-64, 64, N); b = rng.integers(-2**31, 2**31, N); bg = 7
    elif case == "random10":
        a = rng.integers(-512, 512, N); b = rng.integers(-2**31, 2**31, N); bg = 10
    elif case == "worst_neg":
        a = np.full(N, -512); b = np.full(N, B.extreme_key_word(32)); bg = 10
    else:
        a = 511 * (-1) ** np.arange(N); b = np.full(N, 2**31 - 1); bg = 10
    a = a.astype(np.int32); b = b.astype(np.int32)
    ref, got, cur = np.zeros(N, np.int32), np.zeros(N, np.int32), np.zeros(N, np.int32)
    O.lib().oracle_polymul_schoolbook32(O.p32(a), O.p32(b), N, O.p32(ref))
    off = E.fxe_polymul(O.p32(a), O.p32(b), O.p32(got), 0)
    E.exch_polymul(O.p32(a), O.p32(b), O.p32(cur))
    print(case, "worst distance from an integer:", off, "bound:", CMUX_ERR * U * B.bound(1, N, bg))
    assert np.array_equal(got, cur)
    assert np.array_equal(got, ref)
    assert off <= CMUX_ERR * U * B.bound(1, N, bg)


def test_split_after_rotate_fails_where_rotate_after_split_holds(E, O):
    # the negative control: words whose low limb is -2^15 at coefficients the rotation by 32 wraps (negates).  -(-2^15 + 2^16 h) splits into
    # (-2^15, 1 - h), the rotated limbs are (2^15, -h): a phased copy made from the limbs of the rotated WORDS belongs to another pair of limb
    # polynomials than the plain half of the spectrum, and the product is wrong
    N = 1024
    rng = np.random.default_rng(73)
    b = rng.integers(-2**31, 2**31, N)
    b[N - 32:] = (b[N - 32:] & ~0xFFFF) | 0x8000          # X^32 b brings these to coefficients 0 .. 31, negated
    b[5] = -2**31
    a = rng.integers(-512, 512, N)
    a = a.astype(np.int32); b = b.astype(np.int32)
    ref, good, bad = np.zeros(N, np.int32), np.zeros(N, np.int32), np.zeros(N, np.int32)
    O.lib().oracle_polymul_schoolbook32(O.p32(a), O.p32(b), N, O.p32(ref))
    E.fxe_polymul(O.p32(a), O.p32(b), O.p32(good), 0)
    E.fxe_polymul(O.p32(a), O.p32(b), O.p32(bad), 1)
    assert np.array_equal(good, ref)
    assert not np.array_equal(bad, ref)


@pytest.mark.parametrize("l, Bgbit", [(1, 8), (2, 10), (3, 7), (4, 8)], ids=["l1", "l2", "l3", "l4"])
def test_cmux_word_for_word_with_the_current_form_and_the_oracle(E, O, l, Bgbit):
    p = O.make_params("SK-128", n=16, l=l, Bgbit=Bgbit)
    K = O.SKKeys(p, 74 + l, 2.0**-25, 2.0**-15)
    orc = O.Oracle(p, K.bk, K.ksk)
    plain, ring = key_spectra(E, O, K.bk)
    acc = np.random.default_rng(75).integers(-2**31, 2**31, (2, 1024)).astype(np.int32)
    # rotation amounts below, at and above the phase and at the sign wraps of X^a
    for i, a in [(0, 1), (1, 31), (2, 32), (3, 33), (4, 1023), (5, 1024), (6, 2047), (7, -1000), (8, 777), (9, 1056), (10, 992)]:
        ref = orc.mux_rotate(i, a, acc, schoolbook=True)
        got, cur = acc.copy(), acc.copy()
        off = E.fxe_mux_rotate(dptr(ring), p.l, p.Bgbit, i, a, O.p32(got))
        E.exch_mux_rotate(dptr(plain), p.l, p.Bgbit, i, a, O.p32(cur))
        assert np.array_equal(got, cur), (i, a)
        assert np.array_equal(got, ref), (i, a)
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
    _, ring = key_spectra(E, O, bk)
    acc = np.full((2, 1024), B.crafted_mu(32, l, Bgbit), np.int32)
    rows = B.step_digit_rows(acc, 1024, 32, l, Bgbit)
    assert len(rows) == 2 * l and all(np.all(d == -2**(Bgbit - 1)) for _, _, d in rows)
    assert B.peak_limb_sum([(d, bk[1, r, 0]) for r, _, d in rows], 32) == B.bound(2 * l, 1024, Bgbit)
    ref = orc.mux_rotate(1, 1024, acc, schoolbook=True)
    got = acc.copy()
    off = E.fxe_mux_rotate(dptr(ring), l, Bgbit, 1, 1024, O.p32(got))
    err = CMUX_ERR * U * B.bound(2 * l, 1024, Bgbit)
    print((l, Bgbit), "worst distance from an integer:", off, "bound:", err)
    assert np.array_equal(ref, got)
    assert off <= err < 0.5


def test_fused_rounding_at_the_edge_of_the_bound(E):
    # acc_update16_ring rounds outputs m + 4 as round(R x) = low word of fma(R, x, 1.5 * 2^52).  Values R x at +-(1/2 - bound) around integers k,
    # bound = 4 104 u M at the largest admitted shape (l = 3, Bgbit = 10): the fused form must give k (mod 2^32) for every k up to the limb-sum
    # bound M, as close to the rounding edge as the exactness bound lets a value come
    M = B.bound(6, 1024, 10)
    eps = CMUX_ERR * U * M
    assert eps < 0.05
    rng = np.random.default_rng(76)
    k = np.concatenate([rng.integers(-M, M + 1, 4000), [0, 1, -1, M, -M, M - 1, 1 - M, 2**31, -2**31, 2**32 + 5, 2**31 - 1]]).astype(np.int64)
    R = np.longdouble(0.70710678118654752440)
    for delta in (0.5 - eps, -(0.5 - eps), 0.0, 0.25, -0.25):
        x = ((k.astype(np.longdouble) + np.longdouble(delta)) / R).astype(np.float64)
        fused, two = np.zeros(k.size, np.uint32), np.zeros(k.size, np.uint32)
        E.fxe_round_scaled(dptr(x), C.c_int64(k.size), fused.ctypes.data_as(C.POINTER(C.c_uint32)), two.ctypes.data_as(C.POINTER(C.c_uint32)))
        want = (k & 0xFFFFFFFF).astype(np.uint32)
        assert np.array_equal(fused, want), delta
        assert np.array_equal(two, want), delta          # the form it replaces agrees wherever the bound holds


def test_replay_is_clean_under_asan_and_ubsan(tmp_path):
    # the replay as a stand-alone host program: forward against both table forms, the phased key against rho^32 B, one product against the
    # schoolbook product and against the current form; any out-of-bounds access or undefined operation in the lane code aborts it
    exe = str(tmp_path / "fwd_exchange_emu_san")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DFWD_EXCHANGE_EMU_MAIN", "-o", exe, SRC],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "status 0" in r.stdout
