"""Multi-value bootstrapping with factored test vectors, host side (no GPU): the identity the construction rests on
(base vector times factor = the test vector of thfhe.lut.test_vector, word for word), thfhe.lut's helpers, the argument checks of the new
C entry points that run before any device work, and the model composed from the CPU oracle on reduced parameters."""
import ctypes as C

import numpy as np
import pytest

import lut_reference as R
import mv_lut_reference as MV

N = 1024


@pytest.mark.parametrize("p", [2, 4, 8, 16, 64, 512])
def test_base_times_factor_is_the_test_vector(p):
    # TV0 * F mod (X^N + 1, 2^32) = test_vector(f * step, p) for random signed tables and several steps (even Torus32 words)
    from thfhe import lut
    rng = np.random.default_rng(p)
    for step in (1 << 29, 1 << 27, 2, 0x12345678, -(1 << 20)):
        f = rng.integers(-40, 41, (3, p))
        c = lut.mv_factors(f, p)
        tv0 = lut.mv_base(step)
        for j in range(3):
            want = lut.test_vector(R.to_i32(f[j] * step), p)
            assert np.array_equal(MV.negacyclic_mul(tv0, MV.factor_poly(c[j], N), N), want), (step, j)


def test_combination_of_extractions_is_coefficient_zero_of_the_product():
    # the epilogue's form against the definition: record j = extraction at coefficient 0 of (mask * F_j, body * F_j), random words everywhere
    rng = np.random.default_rng(7)
    acc = rng.integers(-2**31, 2**31, 2 * N, dtype=np.int64).astype(np.int32)
    for p, q in ((2, 1), (16, 3), (64, 2)):
        w = rng.integers(-2**31, 2**31, (q, p), dtype=np.int64).astype(np.int32)
        got = MV.combine(acc, w, N)
        for j in range(q):
            F = MV.factor_poly(w[j], N)
            prod = np.concatenate([MV.negacyclic_mul(acc[:N], F, N), MV.negacyclic_mul(acc[N:], F, N)])
            assert np.array_equal(got[j], R.extract_at(prod, 0, N)), (p, j)


def test_mv_helpers_shapes_and_values():
    from thfhe import lut
    c = lut.mv_factors([[0, 1, 2, 3], [3, 0, 3, 0]], 4)
    assert c.shape == (2, 4) and c.dtype == np.int32
    assert c.tolist() == [[1, 1, 1, -3], [-3, 3, -3, -3]]
    assert lut.mv_factors([5, 7], 2).shape == (1, 2)
    assert lut.mv_factors([4, 1, 2, 3], 4).tolist() == [[-3, 1, 1, -7]]           # integers as given: 4 is not reduced to 0
    with pytest.raises(ValueError):
        lut.mv_factors([[0, 1, 2]], 4)
    with pytest.raises(ValueError):
        lut.mv_factors([0, 1, 2], 3)
    tv0 = lut.mv_base(1 << 29)
    assert tv0.shape == (N,) and tv0.dtype == np.int32 and (tv0 == 1 << 28).all()
    with pytest.raises(ValueError):
        lut.mv_base(3)
    f = lambda h, l: 3 * h + l * l + 1
    tv0, w = lut.tree_mv_factors(f, 8, 4, 8)
    assert (tv0 == 1 << 27).all() and w.shape == (8, 4)
    for h in range(8):
        assert np.array_equal(w[h], lut.mv_factors([f(h, l) % 8 for l in range(4)], 4)[0])
        tv = MV.negacyclic_mul(tv0, MV.factor_poly(w[h], N), N)
        assert np.array_equal(tv, lut.tree_test_vectors(f, 8, 4, 8)[h])              # the rows thfhe_tree_lut_bootstrap rotates one by one


def _spec(thfhe, n_inputs=1, weights=(1, 0, 0), bias=0, theta=1):
    return thfhe.LutSpec(n_inputs, (C.c_int32 * 3)(*weights), bias, theta)


def test_mv_entry_points_validate_arguments_without_a_device():
    import thfhe
    L = thfhe.lib()
    i32 = C.POINTER(C.c_int32)
    tv = np.zeros(N, np.int32)
    w = np.zeros((2, 64, 64), np.int32)
    rec = np.zeros((4, 631), np.int32)
    out = np.zeros(4 * 64 * 1025, np.int32)
    ptv, pw, prec, pout = tv.ctypes.data_as(i32), w.ctypes.data_as(i32), rec.ctypes.data_as(i32), out.ctypes.data_as(i32)
    err = L.thfhe_last_error
    ok = _spec(thfhe)
    for fn in (L.thfhe_mv_lut_bootstrap, L.thfhe_mv_lut_bootstrap_wo_keyswitch):
        call = lambda spec=ok, tv0=ptv, f=pw, p=4, q=4, n_tables=1, idx=None, in0=prec, in1=None, o=pout: fn(
            None, None if spec is None else C.byref(spec), tv0, f, p, q, n_tables, idx, in0, in1, None, o, 4)
        for kw in (dict(spec=None), dict(tv0=None), dict(f=None), dict(in0=None), dict(o=None)):
            assert call(**kw) == -1 and b"null" in err(), kw
        assert call(spec=_spec(thfhe, n_inputs=2)) == -1 and b"null operand" in err()
        assert call(spec=_spec(thfhe, n_inputs=4), in1=prec) == -1 and b"n_inputs" in err()
        assert call(spec=_spec(thfhe, theta=3)) == -1 and b"theta" in err()
        for theta in (2, 4):
            assert call(spec=_spec(thfhe, theta=theta)) == -1 and b"theta must be 1" in err()
        for bad in (0, 1, 3, 6, 128, -4):
            assert call(p=bad) == -1 and b"p must be" in err(), bad
        for bad in (0, 65, -1):
            assert call(q=bad) == -1 and b"q must be" in err(), bad
        for bad in (0, 1025, -1):
            assert call(n_tables=bad) == -1, bad
        for bad in ([0, 1, 2, 0], [0, -1, 0, 0]):
            idx = np.array(bad, np.int32)
            assert call(n_tables=2, idx=idx.ctypes.data_as(i32)) == -1 and b"out of range" in err()
        # a valid call gets as far as the missing context, at both limits of p and q
        idx = np.array([0, 1, 1, 0], np.int32)
        assert call(p=64, q=64, n_tables=2, idx=idx.ctypes.data_as(i32)) == -1 and b"null ctx" in err()
        assert call(p=2, q=1) == -1 and b"null ctx" in err()

    tree = L.thfhe_tree_lut_bootstrap_mv
    call = lambda lo=ok, hi=ok, p_hi=4, p_lo=4, tv0=ptv, f=pw, n_tables=1, idx=None, lo1=None, hi1=None: tree(
        None, None, C.byref(lo), C.byref(hi), p_hi, p_lo, tv0, f, n_tables, idx, prec, lo1, None, prec, hi1, None, pout, 4)
    assert tree(None, None, None, None, 4, 4, None, None, 1, None, None, None, None, None, None, None, None, 4) == -1 and b"null" in err()
    assert call(tv0=None) == -1 and b"null" in err()
    assert call(f=None) == -1 and b"null" in err()
    assert call(lo=_spec(thfhe, n_inputs=2)) == -1 and b"null operand" in err()
    assert call(hi=_spec(thfhe, n_inputs=2)) == -1 and b"null operand" in err()
    assert call(lo=_spec(thfhe, theta=3)) == -1 and b"theta" in err()
    assert call(lo=_spec(thfhe, theta=2)) == -1 and b"theta must be 1" in err()
    assert call(hi=_spec(thfhe, theta=2)) == -1 and b"spec_hi theta" in err()
    for bad in (0, 1, 3, 6, 1024):
        assert call(p_hi=bad) == -1 and b"p_hi" in err()
    assert call(p_hi=128) == -1 and b"q must be" in err()                          # a valid tree modulus, beyond a multi-value rotation's 64 outputs
    for bad in (0, 1, 3, 128):
        assert call(p_lo=bad) == -1 and b"p must be" in err()
    assert call(n_tables=0) == -1 and b"n_tables" in err()
    assert call(n_tables=1025) == -1 and b"n_tables" in err()
    idx = np.array([0, 1, 2, 0], np.int32)
    assert call(n_tables=2, idx=idx.ctypes.data_as(i32)) == -1 and b"table_index" in err()
    assert call(p_hi=64, p_lo=64, n_tables=2, idx=np.array([0, 1, 1, 0], np.int32).ctypes.data_as(i32)) == -1 and b"null ctx" in err()
    # a null context is refused before the count is looked at, as in thfhe_lut_bootstrap
    assert L.thfhe_mv_lut_bootstrap(None, C.byref(ok), ptv, pw, 4, 4, 1, None, prec, None, None, pout, 0) == -1 and b"null ctx" in err()


def test_python_layer_checks_shapes_before_the_library():
    import thfhe
    ck = thfhe.CloudKey.__new__(thfhe.CloudKey)
    ck.params, ck.words, ck.h = thfhe.make_params("SK-128"), 631, None
    x = np.zeros((2, 631), np.int32)
    tv0, w = np.zeros(N, np.int32), np.zeros((4, 4), np.int32)
    with pytest.raises(ValueError):
        ck.mv_lut_bootstrap(w, x, tv0=np.zeros(N - 1, np.int32))
    with pytest.raises(ValueError):
        ck.mv_lut_bootstrap(np.zeros(4, np.int32), x, tv0=tv0)
    with pytest.raises(ValueError):
        ck.mv_lut_bootstrap(w, x, x, tv0=tv0, weights=(1,))
    with pytest.raises(ValueError):
        ck.mv_lut_bootstrap_wo_keyswitch(w, x, tv0=tv0, table_index=[0])
    pc = type("P", (), {"h": None})()
    with pytest.raises(ValueError):
        ck.tree_lut_bootstrap_mv(pc, w, x, x[:1], tv0=tv0)
    with pytest.raises(ValueError):
        ck.tree_lut_bootstrap_mv(pc, w, x, x, tv0=tv0, table_index=[0, 0, 0])


def test_model_decrypts_every_message_at_p4_q4(sk_small):
    # SK-128's ring, gadget and key-switch shape at n = 16: four functions of every digit from one rotation, with and without the key switch
    from thfhe import lut
    p, K, orc = sk_small
    f = np.array([[0, 1, 2, 3], [3, 2, 1, 0], [1, 1, 2, 2], [0, 3, 0, 3]])
    tv0, w = lut.mv_base((1 << 32) // 8), lut.mv_factors(f, 4)
    x = R.encrypt_words(K, lut.encode(np.arange(4), 4), 2.0**-15, 41)
    for m in range(4):
        u = MV.mv_lut(orc, [x[m]], (1,), 0, tv0, w, keyswitch=False)
        got = MV.mv_lut(orc, [x[m]], (1,), 0, tv0, w)
        assert u.shape == (4, N + 1) and got.shape == (4, p.n + 1)
        assert np.array_equal(got, np.stack([orc.keyswitch(r) for r in u]))
        assert np.array_equal(lut.decode(K.phases(got), 4), f[:, m]), m
        # one rotation of the product test vector gives the same message: the factored form changes the noise, not the value
        one = R.lut_bootstrap(orc, [x[m]], (1,), 0, lut.test_vector(lut.int_outputs(lambda k: f[1][k], 4), 4), 1)
        assert lut.decode(K.phases(one), 4)[0] == f[1, m]
