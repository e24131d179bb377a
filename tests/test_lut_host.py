"""Programmable bootstrapping, host side (no GPU): the test-vector layout of thfhe.lut, the integer encoding, the composed oracle reference
the GPU tests compare against, and the argument checks of the C ABI that run before any device work."""
import ctypes as C

import numpy as np
import pytest

import lut_reference as R


@pytest.mark.parametrize("p", [2, 4, 8, 16, 32])
@pytest.mark.parametrize("theta", [1, 2, 4])
def test_test_vector_layout_noiseless(O, p, theta):
    # every phase inside m's box (multiples of theta, the wrapped lower half of m = 0 included) brings f_j(m) to coefficient j of X^{-phase} tv
    from thfhe import lut
    N = 1024
    rng = np.random.default_rng(1000 * p + theta)
    tables = rng.integers(-2**31, 2**31, (theta, p)).astype(np.int32)
    tv = lut.test_vector(tables, p, theta, N)
    assert tv.dtype == np.int32 and tv.shape == (N,)
    box = N // p
    for m in range(p):
        for phase in range(m * box - box // 2, m * box + box // 2, theta):
            rot = R.monomial(tv, -phase, N)
            assert np.array_equal(rot[:theta], tables[:, m]), (m, phase)


def test_test_vector_of_a_constant_table_is_the_gate_test_vector_inside_the_boxes():
    from thfhe import lut
    tv = lut.test_vector(np.full(4, lut.MU8, np.int32), 4)
    assert np.all(tv[:1024 - 128] == lut.MU8) and np.all(tv[1024 - 128:] == -lut.MU8)   # the wrapped half-box of m = 0 carries the sign


def test_encode_decode_round_trip():
    from thfhe import lut
    for p in (2, 4, 8, 16, 32, 64):
        m = np.arange(p)
        w = lut.encode(m, p)
        assert w.dtype == np.int32
        assert np.array_equal(lut.decode(w, p), m)
        step = (1 << 32) // (2 * p)
        for e in (-(step // 2) + 1, step // 2 - 1):   # noise below half a step decodes to the same message
            assert np.array_equal(lut.decode(R.to_i32(w.astype(np.int64) + e), p), m)
        assert np.all(lut.decode(R.to_i32(w.astype(np.int64) + (1 << 31)), p) >= p)   # a phase in [1/2, 1) is flagged, not folded
    assert np.array_equal(lut.int_outputs(lambda m: m + 1, 4), lut.encode([1, 2, 3, 0], 4))
    assert np.array_equal(lut.bool_outputs(lambda m: m >= 2, 4), [-lut.MU8, -lut.MU8, lut.MU8, lut.MU8])
    with pytest.raises(ValueError):
        lut.encode([4], 4)
    with pytest.raises(ValueError):
        lut.test_vector(np.zeros((2, 4)), 4, theta=1)


def _check_composed_reference(O, p, K, orc, x, mu):
    tv = np.full(p.N, mu, np.int32)
    for r in x:
        u = R.lut_bootstrap(orc, [r], (1,), 0, tv, 1, keyswitch=False)
        ref = orc.bootstrap_wo_keyswitch(r, mu)
        assert np.array_equal(u[0], ref)
        assert np.array_equal(R.lut_bootstrap(orc, [r], (1,), 0, tv, 1)[0], orc.keyswitch(ref))


def test_composed_reference_equals_the_oracle_bootstrap_small(O, sk_small):
    p, K, orc = sk_small
    x = K.encrypt_bits([0, 1, 1, 0], 2.0**-15, 5)
    for mu in (1 << 29, 1 << 28):
        _check_composed_reference(O, p, K, orc, x, mu)


def test_composed_reference_equals_the_oracle_bootstrap_sk128(O, sk128):
    p, K, orc = sk128
    _check_composed_reference(O, p, K, orc, K.encrypt_bits([1], O.SIGMAS["SK-128"]["lwe"], 6), 1 << 29)


def test_composed_reference_theta_rounds_to_multiples(O, sk_small):
    # the theta = 2 / 4 mod-switch is oracle_modswitch(x, N / theta) * theta: even resp. multiple-of-four exponents only
    p, K, orc = sk_small
    x = K.encrypt_bits([1, 0, 1], 2.0**-15, 8)
    for theta in (2, 4):
        bars = [O.lib().oracle_modswitch(int(w), p.N // theta) * theta for w in x.reshape(-1)]
        assert all(b % theta == 0 and -p.N <= b < p.N for b in bars)
        tv = np.arange(p.N, dtype=np.int32) << 20
        u = R.lut_bootstrap(orc, [x[0]], (1,), 0, tv, theta, keyswitch=False)
        assert u.shape == (theta, p.N + 1)


def _spec(thfhe, n_inputs=1, weights=(1, 0, 0), bias=0, theta=1):
    return thfhe.LutSpec(n_inputs, (C.c_int32 * 3)(*weights), bias, theta)


def test_lut_entry_points_validate_arguments_without_a_device():
    import thfhe
    L = thfhe.lib()
    i32 = C.POINTER(C.c_int32)
    tv = np.zeros((2, 1024), np.int32)
    rec = np.zeros((4, 631), np.int32)
    out = np.zeros(4 * 4 * 1025, np.int32)
    ptv, prec, pout = tv.ctypes.data_as(i32), rec.ctypes.data_as(i32), out.ctypes.data_as(i32)
    for fn in (L.thfhe_lut_bootstrap, L.thfhe_lut_bootstrap_wo_keyswitch):
        # null pointers first
        assert fn(None, None, None, 1, None, None, None, None, None, 1) == -1
        assert fn(None, C.byref(_spec(thfhe)), None, 1, None, prec, None, None, pout, 4) == -1 and b"null" in L.thfhe_last_error()
        assert fn(None, C.byref(_spec(thfhe, n_inputs=2)), ptv, 2, None, prec, None, None, pout, 4) == -1 and b"null operand" in L.thfhe_last_error()
        # the spec, the table count and every lut_index entry, before the context is looked at
        assert fn(None, C.byref(_spec(thfhe, n_inputs=4)), ptv, 2, None, prec, prec, prec, pout, 4) == -1 and b"n_inputs" in L.thfhe_last_error()
        assert fn(None, C.byref(_spec(thfhe, n_inputs=0)), ptv, 2, None, prec, None, None, pout, 4) == -1 and b"n_inputs" in L.thfhe_last_error()
        assert fn(None, C.byref(_spec(thfhe, theta=3)), ptv, 2, None, prec, None, None, pout, 4) == -1 and b"theta" in L.thfhe_last_error()
        assert fn(None, C.byref(_spec(thfhe)), ptv, 0, None, prec, None, None, pout, 4) == -1 and b"n_luts" in L.thfhe_last_error()
        assert fn(None, C.byref(_spec(thfhe)), ptv, 1025, None, prec, None, None, pout, 4) == -1 and b"n_luts" in L.thfhe_last_error()
        for bad in ([0, 1, 2, 0], [0, -1, 0, 0]):
            idx = np.array(bad, np.int32)
            assert fn(None, C.byref(_spec(thfhe)), ptv, 2, idx.ctypes.data_as(i32), prec, None, None, pout, 4) == -1
            assert b"lut_index" in L.thfhe_last_error()
        # a valid call without a context
        idx = np.array([0, 1, 1, 0], np.int32)
        assert fn(None, C.byref(_spec(thfhe, theta=4)), ptv, 2, idx.ctypes.data_as(i32), prec, None, None, pout, 4) == -1
        assert b"null ctx" in L.thfhe_last_error()


def test_cloudkey_lut_arguments_are_checked_in_python():
    # the Python layer refuses inputs out of order or a weight count that does not match, before calling the library
    import thfhe
    ck = thfhe.CloudKey.__new__(thfhe.CloudKey)
    ck.params, ck.words, ck.h = thfhe.make_params("SK-128"), 631, None
    x = np.zeros((2, 631), np.int32)
    tv = np.zeros(1024, np.int32)
    with pytest.raises(ValueError):
        ck.lut_bootstrap(tv, x, None, x, weights=(1, 1))
    with pytest.raises(ValueError):
        ck.lut_bootstrap(tv, x, x, weights=(1,))
    with pytest.raises(ValueError):
        ck.lut_bootstrap(tv, x, x[:1], weights=(1, 1))
    with pytest.raises(ValueError):
        ck.lut_bootstrap(tv, x, lut_index=[0])
