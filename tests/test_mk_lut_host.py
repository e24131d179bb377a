"""Multi-key programmable bootstrapping, host side (no GPU): the Torus64 test-vector layout of thfhe.lut, the unchanged Torus32 defaults, the
composed oracle reference the GPU tests compare against, and the argument checks of the C ABI that run before any device work."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import mk_lut_reference as R


@pytest.mark.parametrize("N", [1024, 2048, 4096])
@pytest.mark.parametrize("p", [2, 4, 8])
@pytest.mark.parametrize("theta", [1, 2, 4])
def test_torus64_test_vector_layout_noiseless(O, N, p, theta):
    # every phase inside m's box (multiples of theta, the wrapped lower half of m = 0 included) brings f_j(m) to coefficient j of X^{-phase} tv
    from thfhe import lut
    rng = np.random.default_rng(10000 * p + 100 * theta + N // 1024)
    tables = rng.integers(-2**63, 2**63, (theta, p), dtype=np.int64)
    tv = lut.test_vector(tables, p, theta, N, torus_bits=64)
    assert tv.dtype == np.int64 and tv.shape == (N,)
    box = N // p
    for m in range(p):
        for phase in range(m * box - box // 2, m * box + box // 2, theta):
            rot = R.monomial64(tv, -phase, N)
            assert np.array_equal(rot[:theta], tables[:, m]), (m, phase)


def test_torus64_outputs():
    from thfhe import lut
    for p in (2, 4, 8):
        w = lut.int_outputs(lambda m: m, p, torus_bits=64)
        assert w.dtype == np.int64
        assert [int(v) % (1 << 64) for v in w] == [m * ((1 << 64) // (2 * p)) for m in range(p)]
    assert np.array_equal(lut.int_outputs(lambda m: m + 1, 4, torus_bits=64), R.to_i64([1 << 61, 2 << 61, 3 << 61, 0]))
    assert np.array_equal(lut.bool_outputs(lambda m: m >= 2, 4, torus_bits=64), [-(1 << 61), -(1 << 61), 1 << 61, 1 << 61])
    tv = lut.test_vector(lut.bool_outputs(lambda m: True, 4, torus_bits=64), 4, N=2048, torus_bits=64)
    assert np.all(tv[:2048 - 256] == 1 << 61) and np.all(tv[2048 - 256:] == -(1 << 61))   # the gate test vector inside the boxes
    with pytest.raises(ValueError):
        lut.test_vector(np.zeros(4, np.int64), 4, torus_bits=16)


def test_torus32_defaults_are_unchanged():
    # sha256 of the Torus32 helpers' output for a fixed set of calls, recorded before the torus_bits option existed
    from thfhe import lut
    h, h32 = hashlib.sha256(), hashlib.sha256()
    rng = np.random.default_rng(7)
    for p in (2, 4, 8, 16):
        for theta in (1, 2, 4):
            for N in (1024, 2048):
                T = rng.integers(-2**31, 2**31, (theta, p)).astype(np.int32)
                h.update(lut.test_vector(T, p, theta, N).tobytes())
                h32.update(lut.test_vector(T, p, theta, N, torus_bits=32).tobytes())
        for hh, kw in ((h, {}), (h32, dict(torus_bits=32))):
            hh.update(lut.int_outputs(lambda m: 3 * m + 1, p, **kw).tobytes())
            hh.update(lut.int_outputs(lambda m: m * m, 2 * p, p, **kw).tobytes())
            hh.update(lut.bool_outputs(lambda m: m % 3 == 1, p, **kw).tobytes())
    assert h.hexdigest() == "768bcbbed39ce958fa635b44ae6b70362c0a28034c4483bfa4be761824c66a89"
    assert h32.hexdigest() == h.hexdigest()


def _mk(O, name, seed, **over):
    p = O.make_params(name, **over)
    s = O.SIGMAS[name]
    K = O.MKKeys(p, seed, s["bk"], s["ks"])
    return p, K, O.MKOracle(p, K.bk, K.ksk)


@pytest.mark.parametrize("name,over", [("MK2", dict(n=24)), ("MK4-N2048", dict(n=6, parties=2)), ("MK64-fft", dict(n=3, parties=2))])
def test_composed_reference_equals_the_oracle_bootstrap(O, name, over):
    p, K, orc = _mk(O, name, 31, **over)
    x = K.encrypt_bits([0, 1, 1], O.SIGMAS[name]["lwe"], 5)
    x[2, 1] = 0   # a zero mask word: the skip
    for mu in (1 << 61, 1 << 60):
        tv = np.full(p.N, mu, np.int64)
        for r in x:
            u = R.lut_bootstrap(orc, [r], (1,), 0, tv, 1, keyswitch=False)
            ref = orc.bootstrap_wo_keyswitch(r, mu)
            assert np.array_equal(u[0], ref), (name, mu)
            assert np.array_equal(R.lut_bootstrap(orc, [r], (1,), 0, tv, 1)[0], orc.keyswitch(ref))


def test_composed_reference_theta_rounds_to_multiples(O):
    # the theta = 2 / 4 mod-switch is oracle_modswitch(x, N / theta) * theta: even resp. multiple-of-four exponents only
    p, K, orc = _mk(O, "MK2", 32, n=12)
    x = K.encrypt_bits([1, 0, 1], O.SIGMAS["MK2"]["lwe"], 8)
    for theta in (2, 4):
        bars = R.bars(x.reshape(-1), p.N, theta)
        assert all(b % theta == 0 and -p.N <= b < p.N for b in bars)
        assert any(b % (2 * theta) for b in bars)   # not merely a coarser grid
        tv = np.arange(p.N, dtype=np.int64) << 40
        u = R.lut_bootstrap(orc, [x[0]], (1,), 0, tv, theta, keyswitch=False)
        assert u.shape == (theta, p.N + 1)


def _spec(thfhe, n_inputs=1, weights=(1, 0, 0), bias=0, theta=1):
    return thfhe.LutSpec(n_inputs, (C.c_int32 * 3)(*weights), bias, theta)


def test_mk_lut_entry_points_validate_arguments_without_a_device():
    import thfhe
    L = thfhe.lib()
    i32, i64 = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    tv = np.zeros((2, 1024), np.int64)
    rec = np.zeros((4, 1041), np.int32)
    out = np.zeros(4 * 4 * 1041, np.int32)
    ptv, prec, pout = tv.ctypes.data_as(i64), rec.ctypes.data_as(i32), out.ctypes.data_as(i32)
    for fn in (L.thfhe_mk_lut_bootstrap, L.thfhe_mk_lut_bootstrap_wo_keyswitch):
        # null pointers first
        assert fn(None, None, None, 1, None, None, None, None, None, 1) == -1
        assert fn(None, C.byref(_spec(thfhe)), None, 1, None, prec, None, None, pout, 4) == -1 and b"null" in L.thfhe_last_error()
        assert fn(None, C.byref(_spec(thfhe)), ptv, 1, None, None, None, None, pout, 4) == -1 and b"null" in L.thfhe_last_error()
        assert fn(None, C.byref(_spec(thfhe)), ptv, 1, None, prec, None, None, None, 4) == -1 and b"null" in L.thfhe_last_error()
        assert fn(None, C.byref(_spec(thfhe, n_inputs=2)), ptv, 2, None, prec, None, None, pout, 4) == -1 and b"null operand" in L.thfhe_last_error()
        assert fn(None, C.byref(_spec(thfhe, n_inputs=3)), ptv, 2, None, prec, prec, None, pout, 4) == -1 and b"null operand" in L.thfhe_last_error()
        # the spec, the table count and every lut_index entry, before the context is looked at
        assert fn(None, C.byref(_spec(thfhe, n_inputs=4)), ptv, 2, None, prec, prec, prec, pout, 4) == -1 and b"n_inputs" in L.thfhe_last_error()
        assert fn(None, C.byref(_spec(thfhe, n_inputs=0)), ptv, 2, None, prec, None, None, pout, 4) == -1 and b"n_inputs" in L.thfhe_last_error()
        for theta in (0, 3, 8):
            assert fn(None, C.byref(_spec(thfhe, theta=theta)), ptv, 2, None, prec, None, None, pout, 4) == -1 and b"theta" in L.thfhe_last_error()
        for n_luts in (0, -1, 1025):
            assert fn(None, C.byref(_spec(thfhe)), ptv, n_luts, None, prec, None, None, pout, 4) == -1 and b"n_luts" in L.thfhe_last_error()
        for bad in ([0, 1, 2, 0], [0, -1, 0, 0], [0, 0, 0, 2]):
            idx = np.array(bad, np.int32)
            assert fn(None, C.byref(_spec(thfhe)), ptv, 2, idx.ctypes.data_as(i32), prec, None, None, pout, 4) == -1
            assert b"lut_index" in L.thfhe_last_error()
        # a valid call without a context
        idx = np.array([0, 1, 1, 0], np.int32)
        assert fn(None, C.byref(_spec(thfhe, n_inputs=3, theta=4)), ptv, 2, idx.ctypes.data_as(i32), prec, prec, prec, pout, 4) == -1
        assert b"null ctx" in L.thfhe_last_error()


def test_mkcloudkey_lut_arguments_are_checked_in_python():
    # the Python layer refuses inputs out of order, a weight count that does not match, a short lut_index or a test vector of the wrong
    # ring degree, before calling the library
    import thfhe
    ck = thfhe.MKCloudKey.__new__(thfhe.MKCloudKey)
    ck.params, ck.words, ck.h = thfhe.make_params("MK2"), 1041, None
    x = np.zeros((2, 1041), np.int32)
    tv = np.zeros(1024, np.int64)
    with pytest.raises(ValueError):
        ck.lut_bootstrap(tv, x, None, x, weights=(1, 1))
    with pytest.raises(ValueError):
        ck.lut_bootstrap(tv, x, x, weights=(1,))
    with pytest.raises(ValueError):
        ck.lut_bootstrap(tv, x, x[:1], weights=(1, 1))
    with pytest.raises(ValueError):
        ck.lut_bootstrap(tv, x, lut_index=[0])
    with pytest.raises(ValueError):
        ck.lut_bootstrap_wo_keyswitch(np.zeros(1000, np.int64), x)
