"""The multi-value two-digit tree on the 3-gen multi-key engine, host side (no GPU): every host check of
thfhe_mk_tree_lut_bootstrap_mvk, of the packing-kernel switches and (the ends of) thfhe_mk_dag_run_tree_batch (they run before the context is looked at), the Torus64 case of
thfhe.lut.tree_mv(k)_factors against the many-LUT tree's rows, tree_mvk_bool_factors, the Python layer's own checks, and the model
(tests/mk_tree_mv_reference.py) decrypting every (hi, lo) of two bit functions on reduced MK2 keys."""
import ctypes as C

import numpy as np
import pytest

import mk_lut_reference as R
import mk_tree_mv_reference as TM

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


def _spec(thfhe, n_inputs=1, weights=(1, 0, 0), bias=0, theta=1):
    return thfhe.LutSpec(n_inputs, (C.c_int32 * 3)(*weights), bias, theta)


def test_flat_entry_validates_arguments_without_a_device():
    import thfhe
    L = thfhe.lib()
    fn = L.thfhe_mk_tree_lut_bootstrap_mvk
    tv0 = np.zeros(1024, np.int64)
    fac = np.zeros((2, 2, 4, 8), np.int32)      # n_tables 2, k 2, p_hi 4, p_lo 8
    rec = np.zeros((4, 1041), np.int32)
    out = np.zeros((4, 2, 1041), np.int32)
    ptv, pf, prec, pout = tv0.ctypes.data_as(I64), fac.ctypes.data_as(I32), rec.ctypes.data_as(I32), out.ctypes.data_as(I32)
    sp = lambda **kw: C.byref(_spec(thfhe, **kw))

    def err(lo=None, hi=None, p_hi=4, p_lo=8, k=2, tv=ptv, f=pf, n_tables=2, idx=None, lo_in=(prec, None, None), hi_in=(prec, None, None), o=pout, count=4):
        rc = fn(None, sp() if lo is None else lo, sp() if hi is None else hi, p_hi, p_lo, k, tv, f, n_tables, idx, 0, *lo_in, *hi_in, o, count)
        return rc, L.thfhe_last_error()

    # null pointers
    for kw in (dict(tv=None), dict(f=None), dict(lo_in=(None, None, None)), dict(hi_in=(None, None, None)), dict(o=None)):
        rc, msg = err(**kw)
        assert rc == -1 and b"null" in msg, kw
    rc, msg = fn(None, None, sp(), 4, 8, 2, ptv, pf, 2, None, 0, prec, None, None, prec, None, None, pout, 4), L.thfhe_last_error()
    assert rc == -1 and b"null" in msg
    rc, msg = fn(None, sp(), None, 4, 8, 2, ptv, pf, 2, None, 0, prec, None, None, prec, None, None, pout, 4), L.thfhe_last_error()
    assert rc == -1 and b"null" in msg
    # the specs
    for n_in in (0, 4):
        assert err(lo=sp(n_inputs=n_in))[0] == -1 and b"n_inputs" in L.thfhe_last_error()
        assert err(hi=sp(n_inputs=n_in))[0] == -1 and b"n_inputs" in L.thfhe_last_error()
    for kw in (dict(lo=sp(n_inputs=2)), dict(hi=sp(n_inputs=2)), dict(lo=sp(n_inputs=3), lo_in=(prec, prec, None)), dict(hi=sp(n_inputs=3), hi_in=(prec, prec, None))):
        rc, msg = err(**kw)
        assert rc == -1 and b"null operand" in msg
    for theta in (0, 3):
        assert err(lo=sp(theta=theta))[0] == -1 and b"theta" in L.thfhe_last_error()
    for theta in (2, 4):                           # valid specs, but both levels of this tree are theta = 1
        rc, msg = err(hi=sp(theta=theta))
        assert rc == -1 and b"spec_hi theta must be 1" in msg, theta
        rc, msg = err(lo=sp(theta=theta))
        assert rc == -1 and b"multi-value: the spec's theta must be 1" in msg, theta
    # the shapes
    for p_hi in (0, 1, 3, 12, 128, -4):
        rc, msg = err(p_hi=p_hi, k=1)
        assert rc == -1 and b"p_hi must be a power of two in 2 .. 64" in msg, p_hi
    for p_lo in (0, 1, 3, 12, 128, -8):
        rc, msg = err(p_lo=p_lo)
        assert rc == -1 and b"p must be a power of two in 2 .. 64" in msg, p_lo
    for n_tables in (0, -1, 1025):
        rc, msg = err(n_tables=n_tables)
        assert rc == -1 and b"n_tables must be 1 .. 1024" in msg, n_tables
    for k in (0, -1):
        rc, msg = err(k=k)
        assert rc == -1 and b"k must be at least 1" in msg, k
    for p_hi, k in ((4, 17), (64, 2), (2, 33), (32, 4)):   # k p_hi = 68, 128, 66, 128
        rc, msg = err(p_hi=p_hi, k=k)
        assert rc == -1 and b"k p_hi must be at most 64" in msg, (p_hi, k)
    # the table indices and the count
    for bad in ([0, 1, 2, 0], [0, -1, 0, 0]):
        idx = np.array(bad, np.int32)
        rc, msg = err(idx=idx.ctypes.data_as(I32))
        assert rc == -1 and b"table_index out of range" in msg
    rc, msg = err(count=(1 << 31) // 16 + 1)
    assert rc == -1 and b"count too large" in msg
    # out aliasing an input
    for kw in (dict(o=prec), dict(lo=sp(n_inputs=2), lo_in=(prec, pout, None)), dict(hi=sp(n_inputs=3), hi_in=(prec, prec, pout))):
        rc, msg = err(**kw)
        assert rc == -1 and b"must not alias" in msg
    assert err(hi_in=(prec, pout, None))[0] == -1 and b"null ctx" in L.thfhe_last_error()   # an operand the spec does not name is not read
    # valid calls, the largest shapes and the empty batch among them: only the context is missing
    idx = np.array([0, 1, 1, 0], np.int32)
    for kw in (dict(), dict(idx=idx.ctypes.data_as(I32)), dict(count=0), dict(p_hi=64, k=1, p_lo=64), dict(p_hi=2, k=32, p_lo=2), dict(n_tables=1024),
               dict(lo=sp(n_inputs=3), lo_in=(prec, prec, prec), hi=sp(n_inputs=2), hi_in=(prec, prec, None))):
        rc, msg = err(**kw)
        assert rc == -1 and b"null ctx" in msg, kw


def test_packing_kernel_switches_validate_arguments_without_a_device():
    import thfhe
    L = thfhe.lib()
    assert L.thfhe_mk_set_pack_wide_threshold(None, 64) == -1 and b"null ctx" in L.thfhe_last_error()
    buf = C.create_string_buffer(64)
    assert L.thfhe_mk_pack_kernel_name(None, 64, buf, 64) == -1 and b"null" in L.thfhe_last_error()


def test_dag_entry_validates_arguments_without_a_device():
    # thfhe_mk_dag_run_tree_batch: every refusal is in tests/test_mk_dag_tree_host.py; here the ends of the argument list with a NULL context
    import thfhe
    import test_mk_dag_tree_host as D
    L = thfhe.lib()
    rc, msg = D._call(L, D.CHAIN)
    assert rc == -1 and "null ctx" in msg
    rc, msg = L.thfhe_mk_dag_run_tree_batch(None, None, 2, None, 1, None, 0, None, 0, None, None, 0, None, 0, None, 0, None, 0, None, 0, None, 0, None, 1, None, 0,
                                            None, None), L.thfhe_last_error().decode()
    assert rc == -1 and "null argument" in msg
    for rows, kw, needle in (([[D.TREE_MV, 0, 1, -1, 1, 0]], {}, "missing LUT_OUT"), ([[D.SELECT, 0, -1, -1, 0, 0]], {}, D.SELECT_MSG),
                             ([[D.TREE, 0, 1, -1, 0, 3]], {}, "row0 + R"), ([[D.LUT_ENC, 0, -1, -1, 0, 0]], dict(enc=(False, False), n_enc=0), "null table family")):
        rc, msg = D._call(L, rows, **kw)
        assert rc == -1 and needle in msg and "null ctx" not in msg, msg


@pytest.mark.parametrize("N", [1024, 2048, 4096])
def test_factors_times_the_base_vector_are_the_trees_rows(N):
    from thfhe import lut
    rng = np.random.default_rng(N)
    for p_hi, p_lo, p_out, k in ((4, 4, 2, 2), (2, 8, 4, 3), (8, 2, 8, 1), (2, 64, 2, 1)):
        tabs = rng.integers(0, p_out, (k, p_hi, p_lo))
        fs = [lambda h, l, T=T: T[h, l] for T in tabs]
        tv0, w = lut.tree_mvk_factors(fs, p_hi, p_lo, p_out, N=N, torus_bits=64)
        assert tv0.dtype == np.int64 and tv0.shape == (N,) and w.dtype == np.int32 and w.shape == (k, p_hi, p_lo)
        for j in range(k):
            rows = lut.tree_test_vectors(fs[j], p_hi, p_lo, p_out, N=N, torus_bits=64)
            tv1, w1 = lut.tree_mv_factors(fs[j], p_hi, p_lo, p_out, N=N, torus_bits=64)
            assert np.array_equal(tv1, tv0) and np.array_equal(w1, w[j])
            for h in range(p_hi):
                assert np.array_equal(negacyclic_mul64(tv0, factor_poly(w[j, h], N), N), rows[h]), (p_hi, p_lo, j, h)


def test_helpers_defaults_and_the_bool_factors():
    from thfhe import lut
    f = lambda h, l: (h * 3 + l) % 4
    tv32, w32 = lut.tree_mvk_factors([f], 4, 4, 4)
    assert tv32.dtype == np.int32 and tv32.shape == (1024,) and np.all(tv32 == 1 << 28)     # the Torus32 default is unchanged
    assert np.array_equal(lut.tree_mv_factors(f, 4, 4, 4)[1], w32[0])
    tv64, w64 = lut.tree_mvk_factors([f], 4, 4, 4, N=2048, torus_bits=64)
    assert np.all(tv64 == 1 << 60) and np.array_equal(w64, w32)
    with pytest.raises(ValueError):
        lut.tree_mvk_factors([f], 4, 4, 4, torus_bits=16)
    fs = [lambda h, l: int(l > h), lambda h, l: (h ^ l) & 1]
    tv0, w, ob = lut.tree_mvk_bool_factors(fs, 4, 4, N=1024, torus_bits=64)
    assert tv0.dtype == np.int64 and np.all(tv0 == 1 << 61) and ob == -(1 << 61) and w.shape == (2, 4, 4) and w.dtype == np.int32
    for j, g in enumerate(fs):
        for h in range(4):
            assert np.array_equal(w[j, h], lut.mv_factors([[g(h, l) for l in range(4)]], 4)[0])
    assert np.abs(w).max() == 1 and float(np.sqrt((w.astype(float)**2).sum(axis=-1)).max()) <= 2.0
    t32, w32b, ob32 = lut.tree_mvk_bool_factors(fs, 4, 4)
    assert t32.dtype == np.int32 and ob32 == -(1 << 29) and np.array_equal(w32b, w)
    with pytest.raises(ValueError):
        lut.tree_mvk_bool_factors(fs * 9, 4, 4)          # k p_hi = 72
    with pytest.raises(ValueError):
        lut.tree_mvk_bool_factors([lambda h, l: 2], 4, 4)


def test_python_layer_checks_its_arguments():
    import thfhe
    ck = thfhe.MKCloudKey.__new__(thfhe.MKCloudKey)
    ck.params, ck.words, ck.h = thfhe.make_params("MK2"), 1041, None
    x = np.zeros((2, 1041), np.int32)
    tv0, fac = np.zeros(1024, np.int64), np.zeros((2, 4, 4), np.int32)
    with pytest.raises(ValueError):
        ck.tree_lut_bootstrap_mvk(fac, (x, x), x, tv0=tv0)                       # two inputs, one weight
    with pytest.raises(ValueError):
        ck.tree_lut_bootstrap_mvk(fac, x, x[:1], tv0=tv0)
    with pytest.raises(ValueError):
        ck.tree_lut_bootstrap_mvk(fac[0], x, x, tv0=tv0)                         # int32[p_hi][p_lo] is tree_lut_bootstrap_mv's
    with pytest.raises(ValueError):
        ck.tree_lut_bootstrap_mvk(fac, x, x, tv0=np.zeros(2048, np.int64))
    with pytest.raises(ValueError):
        ck.tree_lut_bootstrap_mvk(fac, x, x, tv0=tv0, table_index=[0])
    with pytest.raises(ValueError):
        ck.tree_lut_bootstrap_mv(fac[None], x, x, tv0=tv0)
    with pytest.raises(thfhe.ThfheError, match="k p_hi"):                        # the library's own checks follow
        ck.tree_lut_bootstrap_mvk(np.zeros((5, 16, 4), np.int32), x, x, tv0=tv0)
    with pytest.raises(thfhe.ThfheError, match="null ctx"):
        ck.tree_lut_bootstrap_mv(fac[0], x, x, tv0=tv0, out_bias=-(1 << 61))


def test_model_decrypts_every_pair_of_digits(O):
    # MK2 at n = 24 with real keys and a D = N packing key of 10 one-bit digits: two bit functions of two p = 4 digits in the gates' encoding from
    # 1 + 2 rotations, every (hi, lo), none left out; the candidates and the packed tables are what the contract names
    from thfhe import keygen, lut
    import mk_mv_lut_reference as MV
    import mk_pack_reference as MP
    import support
    p = O.make_params("MK2", n=24)
    s = O.SIGMAS["MK2"]
    K = O.MKKeys(p, 77, s["bk"], s["ks"])
    orc = O.MKOracle(p, K.bk, K.ksk)
    pk = keygen.gen_mk_pack_key(np.random.default_rng(11), K.rlwe_keys.sum(axis=0), K.rlwe_keys, 10, 1, s["bk"])
    fs = [lambda h, l: int(l > h), lambda h, l: (h ^ l) & 1]
    tv0, w, ob = lut.tree_mvk_bool_factors(fs, 4, 4, N=p.N, torus_bits=64)
    x = R.encrypt_words(K, lut.encode(np.arange(4), 4), s["lwe"], 21)
    pairs = [(h, l) for h in range(4) for l in range(4)]
    outs = support.pmap(lambda hl: TM.tree_mvk(orc, pk, 10, 1, tv0, w, [x[hl[1]]], [x[hl[0]]], out_bias=ob), pairs)
    got = np.stack([K.decrypt_bits(o) for o in outs])
    assert got.shape == (16, 2)
    assert got.tolist() == [[bool(f(h, l)) for f in fs] for h, l in pairs]
    # one sample in parts: the level-1 records are the flat multi-value call's, table j packs records j p_hi .. j p_hi + 3
    out, cand, ta, tb = TM.tree_mvk(orc, pk, 10, 1, tv0, w, [x[1]], [x[2]], out_bias=ob, parts=True)
    assert np.array_equal(out, outs[2 * 4 + 1])
    assert np.array_equal(cand, MV.mv_lut(orc, [x[1]], (1,), 0, tv0, w.reshape(8, 4), ob, keyswitch=False))
    for j in range(2):
        a, b = MP.pack(cand[4 * j:4 * j + 4], pk, 10, 1, 4)
        assert np.array_equal(a[0], ta[j]) and np.array_equal(b[0], tb[j])
