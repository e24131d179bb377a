"""Multi-value bootstrapping on the 3-gen multi-key engine, host side (no GPU): the factored test vector over Torus64, the
model's combination (tests/mk_mv_lut_reference.py) against explicit negacyclic products, the order "combine, then convert", the helpers of
thfhe.lut, every host check of the flat entries (they run before the context is looked at) and the model on reduced MK2 keys."""
import ctypes as C

import numpy as np
import pytest

import mk_lut_reference as R
import mk_mv_lut_reference as MV

I32, I64 = C.POINTER(C.c_int32), C.POINTER(C.c_int64)


def negacyclic_mul64(a, F, N):
    """a * F mod (X^N + 1, 2^64), exact, term by term of the sparse integer polynomial F."""
    a = np.ascontiguousarray(a, np.int64).view(np.uint64)
    out = np.zeros(N, np.uint64)
    for k in np.flatnonzero(np.asarray(F)):
        r = np.roll(a, k)
        r[:k] = np.uint64(0) - r[:k]
        out += r * R.to_i64([F[k]]).view(np.uint64)[0]
    return out.view(np.int64)


def factor_poly(c, N):
    """F(X) = sum_k c[k] X^(box/2 + k box), box = N / p."""
    p = len(c)
    box = N // p
    F = np.zeros(N, np.int64)
    F[box // 2 + box * np.arange(p)] = np.asarray(c, np.int64)
    return F


def test_vectorised_conversion_is_the_oracles(O):
    rng = np.random.default_rng(3)
    w = np.concatenate([rng.integers(-2**63, 2**63, 4000, dtype=np.int64),
                        R.to_i64([0, 1, -1, 2**32 - 1, 2**32, -2**32, -2**32 + 1, -2**32 - 1, 2**63 - 1, 2**63 - 512, 2**63 - 513, -2**63, -2**63 + 1])])
    assert np.array_equal(MV.t64tot32(w), [O.lib().oracle_t64tot32(int(v)) for v in w])


@pytest.mark.parametrize("N", [1024, 2048, 4096])
def test_base_times_factor_is_the_test_vector(N):
    # (a) TV0 * F = test_vector(f * step) mod (X^N + 1, 2^64) for every p and signed tables
    from thfhe import lut
    rng = np.random.default_rng(N)
    for p in (2, 4, 8, 16, 32, 64):
        step = 1 << int(rng.integers(40, 62))
        f = rng.integers(-9, 10, (3, p))
        c, tv0 = lut.mv_factors(f, p), lut.mv_base(step, N, torus_bits=64)
        for j in range(3):
            want = lut.test_vector(R.to_i64(f[j].astype(object) * step), p, N=N, torus_bits=64)
            assert np.array_equal(negacyclic_mul64(tv0, factor_poly(c[j], N), N), want), (p, j)


@pytest.mark.parametrize("N,p,q", [(1024, 2, 1), (1024, 64, 3), (2048, 8, 4), (4096, 16, 2)])
def test_combination_is_coefficient_zero_of_the_products(N, p, q):
    # (b) on random accumulators: output j = the extraction at coefficient 0 of ACC * F_j over Torus64, bias on the body, converted once
    rng = np.random.default_rng(p + N)
    acc = rng.integers(-2**63, 2**63, 2 * N, dtype=np.int64)
    c = rng.integers(-2**31, 2**31, (q, p))
    bias = int(rng.integers(-2**63, 2**63, dtype=np.int64))
    got = MV.combine64(acc, c, p, N, bias)
    for j in range(q):
        F = factor_poly(c[j], N)
        prod = np.concatenate([negacyclic_mul64(acc[:N], F, N), negacyclic_mul64(acc[N:], F, N)])
        prod[N] = R.to_i64([int(prod[N]) + bias])[0]
        assert np.array_equal(got[j], R.extract_at(prod, 0, N)), j


@pytest.mark.parametrize("N,p", [(1024, 2), (1024, 64), (2048, 8), (4096, 4)])
def test_converting_first_gives_other_words(N, p):
    # (c) t64tot32 truncates toward zero and is not linear: the model must combine in Torus64 and convert once
    rng = np.random.default_rng(7 * p)
    acc = rng.integers(-2**63, 2**63, 2 * N, dtype=np.int64)
    c = rng.integers(-2**31, 2**31, (2, p))
    a, b = MV.combine64(acc, c, p, N, 12345), MV.convert_then_combine(acc, c, p, N, 12345)
    assert a.shape == b.shape == (2, N + 1) and np.any(a != b)
    # with small taps the two orders differ by the truncation carries only: at most p + 1 units per word, and not everywhere
    c = rng.integers(-1, 2, (2, p))
    d = (MV.combine64(acc, c, p, N).astype(np.int64) - MV.convert_then_combine(acc, c, p, N)).astype(np.int32)
    assert np.any(d != 0) and np.abs(d).max() <= p + 1


def test_helpers_shapes_and_values():
    # (d)
    from thfhe import lut
    b = lut.mv_base(1 << 62, 2048, torus_bits=64)
    assert b.dtype == np.int64 and b.shape == (2048,) and np.all(b == 1 << 61)
    assert lut.mv_base(1 << 30).dtype == np.int32 and lut.mv_base(1 << 30).shape == (1024,)          # the Torus32 default is unchanged
    assert np.array_equal(lut.mv_base(1 << 30, 1024, torus_bits=32), lut.mv_base(1 << 30))
    with pytest.raises(ValueError):
        lut.mv_base(3, 1024, torus_bits=64)
    with pytest.raises(ValueError):
        lut.mv_base(2, 1024, torus_bits=16)
    tabs = [[int(m >= t) for m in range(4)] for t in (1, 2, 3)]
    tv0, c, ob = lut.mv_bool_factors(tabs, 4, 64, 1024)
    assert tv0.dtype == np.int64 and np.all(tv0 == 1 << 61) and ob == -(1 << 61)
    assert c.dtype == np.int32 and c.tolist() == [[1, 0, 0, -1], [0, 1, 0, -1], [0, 0, 1, -1]]       # step functions: two taps, norm sqrt 2
    # noiseless: X^{-phase} tv0 through the combination leaves +-2^61 on the body, nothing on the mask
    for m in range(4):
        acc = np.zeros(2048, np.int64)
        acc[1024:] = R.monomial64(tv0, -(m * 256 + 17), 1024)
        out = MV.combine64(acc, c, 4, 1024, ob)
        assert not out[:, :1024].any() and out[:, 1024].tolist() == [(1 << 29) if m >= t else -(1 << 29) for t in (1, 2, 3)], m
    tv32, c32, ob32 = lut.mv_bool_factors(tabs, 4)
    assert tv32.dtype == np.int32 and np.all(tv32 == 1 << 29) and ob32 == -(1 << 29) and np.array_equal(c32, c)
    with pytest.raises(ValueError):
        lut.mv_bool_factors([[0, 2, 0, 1]], 4, 64)


def _spec(thfhe, n_inputs=1, weights=(1, 0, 0), bias=0, theta=1):
    return thfhe.LutSpec(n_inputs, (C.c_int32 * 3)(*weights), bias, theta)


def test_flat_entries_validate_arguments_without_a_device():
    # (e) every check of lut_validate and mv_validate, then "null ctx"
    import thfhe
    L = thfhe.lib()
    tv0 = np.zeros(1024, np.int64)
    fac = np.zeros((2, 3, 8), np.int32)
    rec = np.zeros((4, 1041), np.int32)
    out = np.zeros(4 * 3 * 1041, np.int32)
    ptv, pf, prec, pout = tv0.ctypes.data_as(I64), fac.ctypes.data_as(I32), rec.ctypes.data_as(I32), out.ctypes.data_as(I32)
    sp = lambda **kw: C.byref(_spec(thfhe, **kw))
    for fn in (L.thfhe_mk_mv_lut_bootstrap, L.thfhe_mk_mv_lut_bootstrap_wo_keyswitch):
        err = lambda *a: (fn(*a), L.thfhe_last_error())
        rc, msg = err(None, sp(), ptv, None, 8, 3, 2, None, 0, prec, None, None, pout, 4)
        assert rc == -1 and b"null" in msg
        for args in ((None, ptv, pf, prec, pout), (sp(), None, pf, prec, pout), (sp(), ptv, pf, None, pout), (sp(), ptv, pf, prec, None)):
            rc, msg = err(None, args[0], args[1], args[2], 8, 3, 2, None, 0, args[3], None, None, args[4], 4)
            assert rc == -1 and b"null" in msg
        rc, msg = err(None, sp(n_inputs=2), ptv, pf, 8, 3, 2, None, 0, prec, None, None, pout, 4)
        assert rc == -1 and b"null operand" in msg
        rc, msg = err(None, sp(n_inputs=3), ptv, pf, 8, 3, 2, None, 0, prec, prec, None, pout, 4)
        assert rc == -1 and b"null operand" in msg
        for n_in in (0, 4):
            rc, msg = err(None, sp(n_inputs=n_in), ptv, pf, 8, 3, 2, None, 0, prec, prec, prec, pout, 4)
            assert rc == -1 and b"n_inputs" in msg
        for theta in (0, 2, 3, 4):
            rc, msg = err(None, sp(theta=theta), ptv, pf, 8, 3, 2, None, 0, prec, None, None, pout, 4)
            assert rc == -1 and b"theta" in msg, theta
        for n_tables in (0, -1, 1025):
            rc, msg = err(None, sp(), ptv, pf, 8, 3, n_tables, None, 0, prec, None, None, pout, 4)
            assert rc == -1 and b"n_luts" in msg
        for p in (0, 1, 3, 12, 128, -8):
            rc, msg = err(None, sp(), ptv, pf, p, 3, 2, None, 0, prec, None, None, pout, 4)
            assert rc == -1 and b"p must be a power of two" in msg, p
        for q in (0, -1, 65):
            rc, msg = err(None, sp(), ptv, pf, 8, q, 2, None, 0, prec, None, None, pout, 4)
            assert rc == -1 and b"q must be" in msg, q
        for bad in ([0, 1, 2, 0], [0, -1, 0, 0]):
            idx = np.array(bad, np.int32)
            rc, msg = err(None, sp(), ptv, pf, 8, 3, 2, idx.ctypes.data_as(I32), 0, prec, None, None, pout, 4)
            assert rc == -1 and b"lut_index" in msg
        rc, msg = err(None, sp(), ptv, pf, 8, 3, 2, None, 0, prec, None, None, pout, (1 << 31) // 16 + 1)
        assert rc == -1 and b"count too large" in msg
        # a valid call, and the empty batch, without a context
        idx = np.array([0, 1, 1, 0], np.int32)
        for count in (4, 0):
            rc, msg = err(None, sp(n_inputs=3), ptv, pf, 8, 3, 2, idx.ctypes.data_as(I32), -(1 << 61), prec, prec, prec, pout, count)
            assert rc == -1 and b"null ctx" in msg
    assert L.thfhe_mk_set_mv_slice(None, 64) == -1 and b"slice" in L.thfhe_last_error()


def test_python_layer_checks_its_arguments():
    import thfhe
    ck = thfhe.MKCloudKey.__new__(thfhe.MKCloudKey)
    ck.params, ck.words, ck.h = thfhe.make_params("MK2"), 1041, None
    x = np.zeros((2, 1041), np.int32)
    tv0, fac = np.zeros(1024, np.int64), np.zeros((3, 4), np.int32)
    with pytest.raises(ValueError):
        ck.mv_lut_bootstrap(fac, x, None, x, tv0=tv0, weights=(1, 1))
    with pytest.raises(ValueError):
        ck.mv_lut_bootstrap(fac, x, tv0=np.zeros(2048, np.int64))
    with pytest.raises(ValueError):
        ck.mv_lut_bootstrap(fac, x, tv0=tv0, table_index=[0])
    with pytest.raises(ValueError):
        ck.mv_lut_bootstrap_wo_keyswitch(np.zeros(4, np.int32), x, tv0=tv0)
    with pytest.raises(thfhe.ThfheError):   # the library's own checks follow: a p that is no power of two
        ck.mv_lut_bootstrap(np.zeros((3, 6), np.int32), x, tv0=tv0)


def test_model_decrypts_three_step_functions_of_a_digit(O):
    # (f) MK2 at reduced n: [m >= t], t = 1, 2, 3, of a p = 4 digit in the gate encoding from ONE rotation, every message
    from thfhe import lut
    p = O.make_params("MK2", n=24)
    s = O.SIGMAS["MK2"]
    K = O.MKKeys(p, 77, s["bk"], s["ks"])
    orc = O.MKOracle(p, K.bk, K.ksk)
    tabs = [[int(m >= t) for m in range(4)] for t in (1, 2, 3)]
    tv0, c, ob = lut.mv_bool_factors(tabs, 4, 64, p.N)
    x = R.encrypt_words(K, lut.encode(np.arange(4), 4), s["lwe"], 9)
    for m in range(4):
        out = MV.mv_lut(orc, [x[m]], (1,), 0, tv0, c, ob)
        assert out.shape == (3, p.parties * p.n + 1)
        assert K.decrypt_bits(out).tolist() == [m >= t for t in (1, 2, 3)], m
        wo = MV.mv_lut(orc, [x[m]], (1,), 0, tv0, c, ob, keyswitch=False)
        assert np.array_equal(out, np.stack([orc.keyswitch(u) for u in wo]))
