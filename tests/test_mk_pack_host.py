"""Multi-key packing key switch, encrypted tables and the two-digit tree of the 3-gen engine, host side (no GPU): the numpy
model (tests/mk_pack_reference.py) on trivial records, thfhe.keygen.gen_mk_pack_key against the summed ring key, the model's tree on reduced MK2
keys, the Torus64 cases of the thfhe.lut helpers and every host check of the new entries (they run before the context is looked at)."""
import ctypes as C

import numpy as np
import pytest

import mk_lut_reference as R
import mk_pack_reference as MP

I32, I64 = C.POINTER(C.c_int32), C.POINTER(C.c_int64)


@pytest.mark.parametrize("N", [1024, 2048, 4096])
@pytest.mark.parametrize("p", [2, 8, 64])
def test_trivial_records_give_the_plain_test_vector_whatever_the_key(N, p):
    from thfhe import lut
    rng = np.random.default_rng(N + p)
    D, t, basebit = 6, 3, 2
    pk = rng.integers(-2**63, 2**63, (D, t, 3, 2, N), dtype=np.int64)
    recs = np.zeros((2 * p, D + 1), np.int32)
    recs[:, D] = rng.integers(-2**31, 2**31, 2 * p, dtype=np.int64).astype(np.int32)
    ta, tb = MP.pack(recs, pk, t, basebit, p)
    assert ta.shape == tb.shape == (2, N) and not ta.any()
    for g in range(2):
        assert np.array_equal(tb[g], lut.test_vector(recs[g * p:(g + 1) * p, D].astype(np.int64) << 32, p, N=N, torus_bits=64))


def _phase64(alpha, beta, Z):
    from thfhe import keygen
    return (beta.view(np.uint64) - keygen.polymul_small64(alpha, Z).view(np.uint64)).view(np.int64)


@pytest.mark.parametrize("P,D,t,basebit", [(2, 10, 4, 2), (4, 6, 12, 1), (1, 5, 8, 4)])
def test_pack_key_rows_decrypt_under_the_summed_key(P, D, t, basebit):
    from thfhe import keygen
    N, sigma = 1024, 2.0**-30.7
    rng = np.random.default_rng(P * 1000 + D)
    zq = keygen.rand_ternary(rng, (P, N))
    in_key = rng.integers(-P, P + 1, D)       # as the coefficients of Z; binary LWE keys are a special case
    pk = keygen.gen_mk_pack_key(np.random.default_rng(5), in_key, zq, t, basebit, sigma, chunk=50)
    R_ = (1 << basebit) - 1
    assert pk.shape == (D, t, R_, 2, N) and pk.dtype == np.int64
    ph = _phase64(pk[..., 0, :].reshape(-1, N), pk[..., 1, :].reshape(-1, N), zq.sum(axis=0)).reshape(D, t, R_, N)
    j, p, v = np.meshgrid(np.arange(D), np.arange(t), np.arange(1, R_ + 1), indexing="ij")
    msg = R.to_i64((v * in_key[j]).astype(object) * (1 << 64) // (1 << ((p + 1) * basebit)).astype(object))
    noise = ph.copy()
    noise[..., 0] = (ph[..., 0].view(np.uint64) - msg.view(np.uint64)).view(np.int64)
    bound = 6 * sigma * np.sqrt(P) * 2.0**64
    assert np.abs(noise).max() <= bound
    assert 0.9 < noise.std() / (sigma * np.sqrt(P) * 2.0**64) < 1.1     # and it is noise of the stated size, not zero
    # another chunking draws another stream, the same chunking the same words
    assert np.array_equal(pk, keygen.gen_mk_pack_key(np.random.default_rng(5), in_key, zq, t, basebit, sigma, chunk=50))


def test_lut_helpers_gain_the_torus64_case():
    from thfhe import keygen, lut
    f = lambda hi, lo: (hi * 3 + lo) % 4
    t32 = lut.tree_test_vectors(f, 4, 4, 4, theta=2)
    assert t32.dtype == np.int32 and np.array_equal(t32, lut.tree_test_vectors(f, 4, 4, 4, 2, 1024, 32))     # the default is unchanged
    t64 = lut.tree_test_vectors(f, 4, 4, 4, theta=2, N=2048, torus_bits=64)
    assert t64.dtype == np.int64 and t64.shape == (2, 2048)
    assert np.array_equal(t64 >> 32, lut.tree_test_vectors(f, 4, 4, 4, theta=2, N=2048).astype(np.int64))   # the same words, 32 bits up
    rng = np.random.default_rng(1)
    Z = keygen.rand_ternary(rng, (3, 1024)).sum(axis=0)
    tv = lut.test_vector(lut.int_outputs(lambda m: m ^ 1, 4, torus_bits=64), 4, torus_bits=64)
    a, b = lut.encrypt_table(Z, tv, 2.0**-30, np.random.default_rng(2), torus_bits=64)
    assert a.dtype == b.dtype == np.int64 and a.shape == b.shape == (1024,)
    e = (_phase64(a[None], b[None], Z)[0].view(np.uint64) - tv.view(np.uint64)).view(np.int64)
    assert 0 < np.abs(e).max() <= 6 * 2.0**34
    z32 = rng.integers(0, 2, 1024).astype(np.int32)
    tv32 = lut.test_vector(lut.int_outputs(lambda m: m, 4), 4)
    a0, b0 = lut.encrypt_table(z32, tv32, 2.0**-25, np.random.default_rng(3))
    a1, b1 = lut.encrypt_table(z32, tv32, 2.0**-25, np.random.default_rng(3), torus_bits=32)
    assert a0.dtype == np.int32 and np.array_equal(a0, a1) and np.array_equal(b0, b1)
    with pytest.raises(ValueError):
        lut.tree_test_vectors(f, 4, 4, 4, torus_bits=16)


@pytest.fixture(scope="module")
def mk2_tree(O):
    """MK2 at n = 24 with real keys and a D = N packing key of 10 one-bit digits (rounding 2^-10 sqrt(sum Z^2 / 12), far inside the half step 1/8)."""
    from thfhe import keygen
    p = O.make_params("MK2", n=24)
    s = O.SIGMAS["MK2"]
    K = O.MKKeys(p, 77, s["bk"], s["ks"])
    Z = K.rlwe_keys.sum(axis=0)
    pk = keygen.gen_mk_pack_key(np.random.default_rng(11), Z, K.rlwe_keys, 10, 1, s["bk"])
    return p, s, K, O.MKOracle(p, K.bk, K.ksk), pk


def test_model_tree_decrypts_every_pair_of_digits(O, mk2_tree):
    from thfhe import lut
    import support
    p, s, K, orc, pk = mk2_tree
    f = lambda hi, lo: ((hi * 5 + lo * 3 + (hi & lo)) >> 1) & 1
    tv1 = lut.tree_test_vectors(f, 4, 4, 2, N=p.N, torus_bits=64)
    x = R.encrypt_words(K, lut.encode(np.arange(4), 4), s["lwe"], 21)
    pairs = [(h, l) for h in range(4) for l in range(4)]
    outs = support.pmap(lambda hl: MP.tree(orc, pk, 10, 1, tv1, [x[hl[1]]], [x[hl[0]]], 4), pairs)
    got = lut.decode(K.phases(np.stack(outs)), 2)
    assert got.tolist() == [f(h, l) for h, l in pairs]


def test_model_packed_table_decrypts_under_the_summed_key(O, mk2_tree):
    # the packed candidates ARE an encrypted test vector under Z: every box of the phase decodes to its candidate
    from thfhe import lut
    p, s, K, orc, pk = mk2_tree
    f = lambda hi, lo: (hi + lo) & 1
    tv1 = lut.tree_test_vectors(f, 4, 4, 2, N=p.N, torus_bits=64)
    x = R.encrypt_words(K, lut.encode([2], 4), s["lwe"], 22)
    out, cand, ta, tb = MP.tree(orc, pk, 10, 1, tv1, [x[0]], [x[0]], 4, parts=True)
    ph = _phase64(ta[None], tb[None], K.rlwe_keys.sum(axis=0))[0]
    want = lut.test_vector(lut.int_outputs(lambda hi: f(hi, 2), 2, 4, torus_bits=64), 4, N=p.N, torus_bits=64)
    err = (ph.view(np.uint64) - want.view(np.uint64)).view(np.int64) / 2.0**64
    assert np.abs(err).max() < 1 / 16       # half of the half step 1/8 of p_out = 2
    assert lut.decode(K.phases(out[None]), 2)[0] == f(2, 2)


def _spec(thfhe, n_inputs=1, weights=(1, 0, 0), bias=0, theta=1):
    return thfhe.LutSpec(n_inputs, (C.c_int32 * 3)(*weights), bias, theta)


def test_new_entries_validate_arguments_without_a_device():
    import thfhe
    L = thfhe.lib()
    last = L.thfhe_last_error
    sp = lambda **kw: C.byref(_spec(thfhe, **kw))
    tv = np.zeros((8, 1024), np.int64)
    rec = np.zeros((8, 1041), np.int32)
    out = np.zeros(8 * 4 * 1041, np.int32)
    ptv, prec, pout = tv.ctypes.data_as(I64), rec.ctypes.data_as(I32), out.ctypes.data_as(I32)
    # thfhe_mk_pack_key_set
    assert L.thfhe_mk_pack_key_set(None, None, 1024, 8, 2) == -1 and b"null" in last()
    for t, bb in ((0, 2), (8, 0), (8, 5), (17, 2), (9, 4), (-1, 1)):
        assert L.thfhe_mk_pack_key_set(None, ptv, 1024, t, bb) == -1 and b"basebit" in last(), (t, bb)
    assert L.thfhe_mk_pack_key_set(None, ptv, 1024, 16, 2) == -1 and b"null ctx" in last()
    # thfhe_mk_pack_boxes
    for args in ((None, ptv, ptv), (prec, None, ptv), (prec, ptv, None)):
        assert L.thfhe_mk_pack_boxes(None, args[0], 8, 4, args[1], args[2]) == -1 and b"null" in last()
    for p in (0, 1, 3, 6, 128, -4):
        assert L.thfhe_mk_pack_boxes(None, prec, 8, p, ptv, ptv) == -1 and b"p must be a power of two" in last(), p
    assert L.thfhe_mk_pack_boxes(None, prec, 6, 4, ptv, ptv) == -1 and b"multiple of p" in last()
    assert L.thfhe_mk_pack_boxes(None, prec, 1 << 28, 4, ptv, ptv) == -1 and b"count too large" in last()
    for count in (8, 0):
        assert L.thfhe_mk_pack_boxes(None, prec, count, 4, ptv, ptv) == -1 and b"null ctx" in last()
    # thfhe_mk_lut_bootstrap_enc(_wo_keyswitch): lut_validate with the raised table cap, and the mask pointer
    for fn in (L.thfhe_mk_lut_bootstrap_enc, L.thfhe_mk_lut_bootstrap_enc_wo_keyswitch):
        err = lambda *a: (fn(*a), last())
        for args in ((None, ptv, ptv, prec, pout), (sp(), None, ptv, prec, pout), (sp(), ptv, None, prec, pout), (sp(), ptv, ptv, None, pout),
                     (sp(), ptv, ptv, prec, None)):
            rc, msg = err(None, args[0], args[1], args[2], 8, None, args[3], None, None, args[4], 4)
            assert rc == -1 and b"null" in msg
        rc, msg = err(None, sp(n_inputs=2), ptv, ptv, 8, None, prec, None, None, pout, 4)
        assert rc == -1 and b"null operand" in msg
        for n_in in (0, 4):
            rc, msg = err(None, sp(n_inputs=n_in), ptv, ptv, 8, None, prec, prec, prec, pout, 4)
            assert rc == -1 and b"n_inputs" in msg
        for theta in (0, 3, 8):
            rc, msg = err(None, sp(theta=theta), ptv, ptv, 8, None, prec, None, None, pout, 4)
            assert rc == -1 and b"theta" in msg
        for n_luts in (0, -1, 262145):
            rc, msg = err(None, sp(), ptv, ptv, n_luts, None, prec, None, None, pout, 4)
            assert rc == -1 and b"n_luts must be 1 .. 262144" in msg
        for bad in ([0, 8, 0, 0], [0, 0, -1, 0]):
            idx = np.array(bad, np.int32)
            rc, msg = err(None, sp(), ptv, ptv, 8, idx.ctypes.data_as(I32), prec, None, None, pout, 4)
            assert rc == -1 and b"lut_index" in msg
        rc, msg = err(None, sp(), ptv, ptv, 8, None, prec, None, None, pout, (1 << 31) // 16 + 1)
        assert rc == -1 and b"count too large" in msg
        idx = np.array([0, 7, 3, 0], np.int32)
        for count in (4, 0):
            rc, msg = err(None, sp(n_inputs=3, theta=4), ptv, ptv, 8, idx.ctypes.data_as(I32), prec, prec, prec, pout, count)
            assert rc == -1 and b"null ctx" in msg
    # thfhe_mk_tree_lut_bootstrap
    fn = L.thfhe_mk_tree_lut_bootstrap
    call = lambda lo, hi, p_hi, tv1, n_tables, idx, lo0, lo1, lo2, hi0, hi1, hi2, o, count: (
        fn(None, lo, hi, p_hi, tv1, n_tables, idx, lo0, lo1, lo2, hi0, hi1, hi2, o, count), last())
    good = dict(lo=sp(), hi=sp(), p_hi=4, tv1=ptv, n_tables=2, idx=None, lo0=prec, lo1=None, lo2=None, hi0=prec, hi1=None, hi2=None, o=pout, count=4)
    bad = lambda **kw: call(**{**good, **kw})
    for k in ("lo", "hi", "tv1", "lo0", "hi0", "o"):
        rc, msg = bad(**{k: None})
        assert rc == -1 and b"null" in msg, k
    for kw in (dict(lo=sp(n_inputs=2)), dict(hi=sp(n_inputs=3), hi1=prec)):
        rc, msg = bad(**kw)
        assert rc == -1 and b"null operand" in msg
    rc, msg = bad(lo=sp(theta=3))
    assert rc == -1 and b"theta" in msg
    rc, msg = bad(hi=sp(theta=2))
    assert rc == -1 and b"spec_hi theta must be 1" in msg
    for p_hi in (0, 1, 3, 12, 128):
        rc, msg = bad(p_hi=p_hi)
        assert rc == -1 and b"p_hi must be a power of two" in msg, p_hi
    rc, msg = bad(lo=sp(theta=4), p_hi=2)
    assert rc == -1 and b"must divide p_hi" in msg
    for n_tables in (0, -3, 262144 // 4 + 1):
        rc, msg = bad(n_tables=n_tables)
        assert rc == -1 and b"n_tables" in msg
    for ix in ([0, 2, 0, 0], [-1, 0, 0, 0]):
        rc, msg = bad(idx=np.array(ix, np.int32).ctypes.data_as(I32))
        assert rc == -1 and b"table_index" in msg
    rc, msg = bad(count=(1 << 31) // 16 + 1)
    assert rc == -1 and b"count too large" in msg
    for count in (4, 0):
        rc, msg = bad(count=count, idx=np.array([0, 1, 1, 0], np.int32).ctypes.data_as(I32), lo=sp(theta=2))
        assert rc == -1 and b"null ctx" in msg
    for v in (64, 0):
        assert L.thfhe_mk_set_tree_slice(None, v) == -1 and b"slice" in last()


def test_python_layer_checks_its_arguments():
    import thfhe
    ck = thfhe.MKCloudKey.__new__(thfhe.MKCloudKey)
    ck.params, ck.words, ck.h = thfhe.make_params("MK2"), 1041, None
    x = np.zeros((2, 1041), np.int32)
    tv = np.zeros((2, 1024), np.int64)
    with pytest.raises(ValueError):
        ck.pack_key_set(np.zeros((4, 8, 3, 2, 512), np.int64), 8, 2)
    with pytest.raises(ValueError):
        ck.pack_boxes(np.zeros((4, 1025), np.int32), 4)                   # no key set
    with pytest.raises(ValueError):
        ck.lut_bootstrap_enc(tv, tv[:1], x)
    with pytest.raises(ValueError):
        ck.lut_bootstrap_enc(tv, tv, x, lut_index=[0])
    with pytest.raises(ValueError):
        ck.tree_lut_bootstrap(np.zeros((3, 1024), np.int64), x, x, p_hi=4)
    with pytest.raises(ValueError):
        ck.tree_lut_bootstrap(np.zeros((4, 1024), np.int64), x, x[:1], p_hi=4)
    with pytest.raises(thfhe.ThfheError):   # the library's own checks follow
        ck.tree_lut_bootstrap(np.zeros((3, 1024), np.int64), x, x, p_hi=3)
