"""Circuit bootstrapping in one-rotation mode, host side (no GPU): the coefficient identity the mode rests on, the CPU
model (tests/cb_one_reference.py) on the real-key cases of tests/cb_cases.py, and the argument checks of the new C ABI entries that run before a
context is looked at.  tests/test_gpu_cb_one.py compares the device with the same model word for word."""
import ctypes as C

import numpy as np
import pytest

import cb_cases as CC
import cb_one_reference as R
import mk_lut_reference as ML
from support import N

D = 2048


@pytest.mark.parametrize("l,th,Bgbit", [(2, 2, 8), (3, 4, 7), (4, 4, 7)])
def test_coefficient_identity(l, th, Bgbit):
    """every barb that the theta-rounded mod-switch can give, every level: coefficient j of X^{-barb} tv is +mu_j for barb < D, else -mu_j -- the sign
    of coefficient 0, which is the bit.  The rotation is the oracle's (oracle_mul_by_monomial64) and, beside it, the start rule of the engine's
    accumulator in numpy: coefficient q is tv[(q + barb) mod D], negated when (q + barb) mod 2D >= D."""
    assert R.theta(l) == th
    tv = R.test_vector(l, Bgbit, D)
    assert tv.dtype == np.int64 and tv.shape == (D,)
    mu = np.array([1 << (63 - (j + 1) * Bgbit) for j in range(l)], np.int64)
    for j in range(th):
        assert np.all(tv[j::th] == (mu[j] if j < l else 0))
    if (l, th) == (3, 4):
        assert not tv[3::4].any()                                   # slot 3 is unused
    barb = np.arange(0, 2 * D, th)
    j = np.arange(l)
    e = (j[None, :] + barb[:, None]) % (2 * D)
    rule = np.where(e >= D, -tv[e % D], tv[e % D])
    want = np.where(barb[:, None] < D, mu[None, :], -mu[None, :])
    assert np.array_equal(rule, want)
    rotated = np.stack([ML.monomial64(tv, -int(b), D) for b in barb])
    assert np.array_equal(rotated[:, :l], want)
    assert np.array_equal(rotated[:, :th], np.where(e[:, :1] >= D, -1, 1) * tv[None, :th])      # an unused slot stays zero at every barb
    # a barb that is NOT a multiple of theta reads a neighbour's constant: the rounding is what the mode needs
    assert ML.monomial64(tv, -1, D)[0] == tv[1]


@pytest.mark.parametrize("name", ["SK-128", "SK-80"])
def test_model_decodes_under_the_real_keys(O, name):
    S, c, m = CC.keys(O, name), CC.case(O, name), R.models(O, name)      # models() asserts that the lookup and the comparison decode
    l, Bgbit = S.tp.l, S.tp.Bgbit
    pool = 48 if name == "SK-128" else 24
    assert m["lwe2_one"].shape == m["lwe2"].shape == (pool, l, D + 1) and m["rows"].shape == (pool, 2 * l, 2, N)
    assert not np.array_equal(m["lwe2_one"], m["lwe2"])                                       # another mod-switch: other words
    half_step = 1 << (31 - l * Bgbit)                                                         # of the finest level g_(l-1)
    assert half_step == (1024 if name == "SK-128" else 2048)
    for what, lwe2 in (("one rotation", m["lwe2_one"]), ("per level", m["lwe2"])):
        err = int(np.abs(R.lwe2_errors(S.z2, lwe2, c["bits"], l, Bgbit)).max())
        print(f"\nstage A {name}, {what}: worst |phase - m g_j| = {err} units of 2^-32, smallest half-step {half_step}")
        assert 4 * err < half_step, (what, err, half_step)
    std, pred = CC.row_noise(S, m["rows"], c["bits"]), S.sigma_row()
    print(f"cb row noise {name}, one rotation (CPU model): measured std {std:.3e}, predicted {pred:.3e}, ratio {std / pred:.2f}")
    assert 0.5 * pred <= std <= 2 * pred
    assert sorted(CC.ADDR.tolist()) == list(range(8))                                         # the 8 lookups models() decoded are all addresses
    assert len({r.tobytes() for r in m["rows"].reshape(pool, -1)}) == pool                    # a draw from the pool shows a misplaced bit


def test_stage_a_one_is_circuit_bootstrap_one_before_the_key_switch(O):
    import cb_reference as CB
    S, c, m = CC.keys(O, "SK-80"), CC.case(O, "SK-80"), R.models(O, "SK-80")
    pick = [3, 20]
    lwe2 = R.stage_a_one(S.orc2, c["recs"][pick], S.tp.l, S.tp.Bgbit)
    assert np.array_equal(lwe2, m["lwe2_one"][pick])
    rows = R.circuit_bootstrap_one(S.orc2, S.pks, c["recs"][pick], S.tp.l, S.tp.Bgbit, CC.T, CC.BASEBIT)
    assert np.array_equal(rows, m["rows"][pick])
    assert np.array_equal(rows, CB.private_keyswitch(S.pks, lwe2, S.tp.l, CC.T, CC.BASEBIT))


def test_new_abi_entries_refuse_bad_arguments_before_a_context_is_looked_at():
    import thfhe
    L = thfhe.lib()
    assert (thfhe.CB_PER_LEVEL, thfhe.CB_ONE_ROTATION) == (0, 1)
    buf = np.zeros(64, np.int32)
    p, h = thfhe._p32(buf), C.c_void_p()
    err = lambda: L.thfhe_last_error().decode()
    cb = L.thfhe_circuit_bootstrap_mode
    for mode in (2, -1, 7):
        assert cb(None, None, p, 1, 3, mode, None, C.byref(h)) != 0 and "mode must be" in err()
    for mode in (0, 1):
        assert cb(None, None, None, 1, 3, mode, None, C.byref(h)) != 0 and "null argument" in err()
        assert cb(None, None, p, 1, 3, mode, None, None) != 0 and "null argument" in err()
        assert cb(None, None, p, 1, 17, mode, None, C.byref(h)) != 0 and "d must be" in err()
        assert cb(None, None, p, 0, 3, mode, None, C.byref(h)) != 0 and "count must be" in err()
        assert cb(None, None, p, 1, 3, mode, None, C.byref(h)) != 0 and "null ctx" in err()   # valid arguments reach the context check
    assert not h.value
    sa = L.thfhe_cb_stage_a
    assert sa(None, None, p, 1, 2, p) != 0 and "mode must be" in err()
    for mode in (0, 1):
        assert sa(None, None, None, 1, mode, p) != 0 and "null argument" in err()
        assert sa(None, None, p, 1, mode, None) != 0 and "null argument" in err()
        assert sa(None, None, p, (1 << 24) + 1, mode, p) != 0 and "count must be" in err()
        assert sa(None, None, p, 1, mode, p) != 0 and "null ctx" in err()
        assert sa(None, None, p, 0, mode, p) != 0 and "null ctx" in err()                    # count 0 is fine; the context is still needed
    rot = L.thfhe_mk_lut_rotate_dev
    v = C.c_void_p(buf.ctypes.data)                                                           # never read: the context check comes first
    assert rot(None, None, 4, v, v, 1) != 0 and "null argument" in err()
    assert rot(None, v, 4, None, v, 1) != 0 and "null argument" in err()
    assert rot(None, v, 4, v, None, 1) != 0 and "null argument" in err()
    for th in (0, 3, 8):
        assert rot(None, v, th, v, v, 1) != 0 and "theta must be" in err()
    assert rot(None, v, 4, v, v, 1) != 0 and "null ctx" in err()
