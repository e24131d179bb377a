"""Encrypted lookup tables and the two-digit tree PBS, host side (no GPU): the box-packing model against the
test-vector layout, the encrypted-table reference against the plaintext one, the composed tree on reduced parameters, thfhe.lut's new
helpers, and the argument checks of the new C entry points that run before any device work."""
import ctypes as C

import numpy as np
import pytest

import lut_reference as R
import pack_reference as PR
import tree_lut_reference as TR

N = 1024


@pytest.mark.parametrize("p", [2, 4, 8, 16])
def test_model_pack_boxes_of_trivial_samples_is_the_test_vector(p):
    # noiseless trivial inputs (a = 0, b = v_i) and an all-zero packing key: exactly (0, test_vector(v, p)), two outputs
    from thfhe import lut
    rng = np.random.default_rng(p)
    n, t, basebit = 12, 8, 2
    pk = np.zeros((n, t, 3, 2, N), np.int32)
    v = rng.integers(-2**31, 2**31, (2, p)).astype(np.int32)
    lwe = np.zeros((2 * p, n + 1), np.int32)
    lwe[:, n] = v.reshape(-1)
    a, b = TR.pack_boxes(lwe, pk, t, basebit, p)
    assert a.shape == b.shape == (2, N) and not a.any()
    for g in range(2):
        assert np.array_equal(b[g], lut.test_vector(v[g], p))


def test_window_product_is_the_window_sum():
    # U(X) f against the definition: sum_k X^(k - B/2) f through the oracle's monomial product
    rng = np.random.default_rng(3)
    f = rng.integers(-2**31, 2**31, N).astype(np.int32)
    for p in (2, 64, 512):
        B = N // p
        want = np.zeros(N, np.int64)
        for k in range(B):
            want += R.monomial(f, k - B // 2, N)
        assert np.array_equal(PR.negacyclic_mul(f[None], TR.window(p, N))[0], PR.wrap32(want))


def test_lut_enc_with_a_zero_mask_is_the_plaintext_lut(sk_small):
    p, K, orc = sk_small
    rng = np.random.default_rng(5)
    x = R.encrypt_words(K, rng.integers(-2**31, 2**31, 3), 2.0**-15, 9)
    tv = rng.integers(-2**31, 2**31, N).astype(np.int32)
    for theta in (1, 2, 4):
        for r in x:
            for ks in (False, True):
                got = TR.lut_enc(orc, [r], (3,), 12345, np.zeros(N, np.int32), tv, theta, keyswitch=ks)
                assert np.array_equal(got, R.lut_bootstrap(orc, [r], (3,), 12345, tv, theta, keyswitch=ks))


def test_lut_enc_of_a_fresh_encrypted_table_decrypts(sk_small):
    from thfhe import lut
    p, K, orc = sk_small
    f = np.array([3, 1, 0, 2])
    tv = lut.test_vector(lut.int_outputs(lambda m: f[m], 4), 4)
    tv_a, tv_b = lut.encrypt_table(K.rlwe_key[0], tv, 2.0**-25, np.random.default_rng(1))
    assert np.abs(PR.torus(PR.wrap32(PR.tlwe_phase(tv_a[None], tv_b[None], K.rlwe_key[0])[0].astype(np.int64) - tv))).max() < 2.0**-20
    x = R.encrypt_words(K, lut.encode(np.arange(4), 4), 2.0**-15, 11)
    got = np.stack([TR.lut_enc(orc, [r], (1,), 0, tv_a, tv_b, 1)[0] for r in x])
    assert np.array_equal(lut.decode(K.phases(got), 4), f)


def _small_pack_key(K, p, seed):
    from thfhe import keygen
    return keygen.gen_pack_key(np.random.default_rng(seed), K.lwe_key, K.rlwe_key[0], p.ks_t, p.ks_basebit, 2.0**-25)


@pytest.mark.parametrize("theta1", [1, 2])
def test_model_tree_decrypts_every_pair_at_p4(sk_small, theta1):
    # SK-128's ring, gadget and key-switch shape at n = 16: f(hi, lo) for all 16 pairs, a table with no structure
    from thfhe import lut
    p, K, orc = sk_small
    pk = _small_pack_key(K, p, 21)
    F = np.random.default_rng(4).integers(0, 4, (4, 4))
    tv1 = lut.tree_test_vectors(lambda h, l: F[h, l], 4, 4, 4, theta=theta1)
    hi, lo = np.repeat(np.arange(4), 4), np.tile(np.arange(4), 4)
    xh = R.encrypt_words(K, lut.encode(hi, 4), 2.0**-15, 31)
    xl = R.encrypt_words(K, lut.encode(lo, 4), 2.0**-15, 32)
    for s in range(16):
        out, cands, (a, b) = TR.tree(orc, pk, p.ks_t, p.ks_basebit, [xl[s]], (1,), 0, theta1, [xh[s]], (1,), 0, tv1, 4)
        assert np.array_equal(lut.decode(K.phases(cands), 4), F[:, lo[s]])
        assert np.array_equal(lut.decode(PR.tlwe_phase(a[None], b[None], K.rlwe_key[0])[0][::256], 4), F[:, lo[s]])
        assert lut.decode(K.phases(out[None]), 4)[0] == F[hi[s], lo[s]], (hi[s], lo[s])


@pytest.mark.parametrize("theta", [1, 2, 4])
def test_tree_test_vectors_rows_equal_test_vector(theta):
    from thfhe import lut
    f = lambda h, l: (3 * h + l * l + 1) % 8
    p_hi, p_lo, p_out = 8, 4, 8
    rows = lut.tree_test_vectors(f, p_hi, p_lo, p_out, theta=theta)
    assert rows.shape == (p_hi // theta, N) and rows.dtype == np.int32
    for r in range(p_hi // theta):
        tables = [lut.encode(np.array([f(r * theta + j, l) % p_out for l in range(p_lo)]), p_out) for j in range(theta)]
        assert np.array_equal(rows[r], lut.test_vector(tables, p_lo, theta))
    with pytest.raises(ValueError):
        lut.tree_test_vectors(f, 2, 4, 8, theta=4)


def _spec(thfhe, n_inputs=1, weights=(1, 0, 0), bias=0, theta=1):
    return thfhe.LutSpec(n_inputs, (C.c_int32 * 3)(*weights), bias, theta)


def test_new_entry_points_validate_arguments_without_a_device():
    import thfhe
    L = thfhe.lib()
    i32 = C.POINTER(C.c_int32)
    tv = np.zeros((2, N), np.int32)
    rec = np.zeros((4, 631), np.int32)
    out = np.zeros(4 * 4 * 1025, np.int32)
    ptv, prec, pout = tv.ctypes.data_as(i32), rec.ctypes.data_as(i32), out.ctypes.data_as(i32)
    err = L.thfhe_last_error
    for fn in (L.thfhe_lut_bootstrap_enc, L.thfhe_lut_bootstrap_enc_wo_keyswitch):
        assert fn(None, None, None, None, 1, None, None, None, None, None, 1) == -1
        assert fn(None, C.byref(_spec(thfhe)), None, ptv, 1, None, prec, None, None, pout, 4) == -1 and b"null" in err()   # the mask is not optional
        assert fn(None, C.byref(_spec(thfhe)), ptv, None, 1, None, prec, None, None, pout, 4) == -1 and b"null" in err()
        assert fn(None, C.byref(_spec(thfhe, n_inputs=2)), ptv, ptv, 2, None, prec, None, None, pout, 4) == -1 and b"null operand" in err()
        assert fn(None, C.byref(_spec(thfhe, n_inputs=4)), ptv, ptv, 2, None, prec, prec, prec, pout, 4) == -1 and b"n_inputs" in err()
        assert fn(None, C.byref(_spec(thfhe, theta=3)), ptv, ptv, 2, None, prec, None, None, pout, 4) == -1 and b"theta" in err()
        assert fn(None, C.byref(_spec(thfhe)), ptv, ptv, 0, None, prec, None, None, pout, 4) == -1 and b"n_luts" in err()
        assert fn(None, C.byref(_spec(thfhe)), ptv, ptv, (1 << 18) + 1, None, prec, None, None, pout, 4) == -1 and b"n_luts" in err()
        for bad in ([0, 1, 2, 0], [0, -1, 0, 0]):
            idx = np.array(bad, np.int32)
            assert fn(None, C.byref(_spec(thfhe)), ptv, ptv, 2, idx.ctypes.data_as(i32), prec, None, None, pout, 4) == -1 and b"lut_index" in err()
        # more than 1 024 tables is a valid call: it gets as far as the missing context
        assert fn(None, C.byref(_spec(thfhe, theta=4)), ptv, ptv, 65536, None, prec, None, None, pout, 4) == -1 and b"null ctx" in err()
    # the plaintext entry keeps its cap
    assert L.thfhe_lut_bootstrap(None, C.byref(_spec(thfhe)), ptv, 1025, None, prec, None, None, pout, 4) == -1 and b"n_luts must be 1 .. 1024" in err()

    tree = L.thfhe_tree_lut_bootstrap
    ok, ok2 = _spec(thfhe), _spec(thfhe, theta=2)
    call = lambda lo, hi, p_hi, n_tables=1, idx=None, tv1=ptv, lo1=None, hi1=None: tree(None, None, C.byref(lo), C.byref(hi), p_hi, tv1, n_tables, idx, prec, lo1, None,
                                                                                        prec, hi1, None, pout, 4)
    assert tree(None, None, None, None, 4, None, 1, None, None, None, None, None, None, None, None, 4) == -1 and b"null" in err()
    assert call(ok, ok, 4, tv1=None) == -1 and b"null" in err()
    assert call(_spec(thfhe, n_inputs=2), ok, 4) == -1 and b"null operand" in err()
    assert call(ok, _spec(thfhe, n_inputs=2), 4) == -1 and b"null operand" in err()
    assert call(_spec(thfhe, theta=3), ok, 4) == -1 and b"theta" in err()
    assert call(ok, ok2, 4) == -1 and b"spec_hi theta" in err()
    for bad_p in (0, 1, 3, 6, 1024):
        assert call(ok, ok, bad_p) == -1 and b"p_hi" in err()
    assert call(_spec(thfhe, theta=4), ok, 2) == -1 and b"divide" in err()
    assert call(ok, ok, 4, n_tables=0) == -1 and b"n_tables" in err()
    assert call(ok, ok, 512, n_tables=513) == -1 and b"n_tables" in err()
    idx = np.array([0, 1, 2, 0], np.int32)
    assert call(ok, ok, 4, n_tables=2, idx=idx.ctypes.data_as(i32)) == -1 and b"table_index" in err()
    assert call(ok2, ok, 4, n_tables=2, idx=np.array([0, 1, 1, 0], np.int32).ctypes.data_as(i32)) == -1 and b"null ctx" in err()

    assert L.thfhe_pack_boxes(None, prec, 4, 4, ptv, ptv) == -1 and b"null" in err()
    assert L.thfhe_set_tree_slice(None, 4096) == -1


def test_python_layers_check_shapes_before_the_library():
    import thfhe
    from thfhe import threshold as T
    ck = thfhe.CloudKey.__new__(thfhe.CloudKey)
    ck.params, ck.words, ck.h = thfhe.make_params("SK-128"), 631, None
    x = np.zeros((2, 631), np.int32)
    tv = np.zeros((1, N), np.int32)
    with pytest.raises(ValueError):
        ck.lut_bootstrap_enc(tv, np.zeros((2, N), np.int32), x)
    with pytest.raises(ValueError):
        ck.lut_bootstrap_enc(tv, tv, x, x, weights=(1,))
    with pytest.raises(ValueError):
        ck.lut_bootstrap_enc(tv, tv, x, lut_index=[0])
    pc = T.PolyContext.__new__(T.PolyContext)
    pc.h, pc.N, pc.pack_n = None, N, None
    with pytest.raises(ValueError):
        ck.tree_lut_bootstrap(pc, np.zeros((3, N), np.int32), x, x, p_hi=4)          # tv1 is not a whole number of tables of 4 rows
    with pytest.raises(ValueError):
        ck.tree_lut_bootstrap(pc, np.zeros((4, N), np.int32), x, x[:1], p_hi=4)
    with pytest.raises(ValueError):
        ck.tree_lut_bootstrap(pc, np.zeros((4, N), np.int32), x, x, p_hi=4, table_index=[0])
    with pytest.raises(thfhe.ThfheError):
        T.PackBoxes(pc, x, 2)                                                        # no key set
