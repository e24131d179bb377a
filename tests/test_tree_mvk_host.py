"""The k-output two-digit tree with a multi-value level 1, host side (no GPU): lut.tree_mvk_factors against
lut.tree_mv_factors; every host check of thfhe_tree_lut_bootstrap_mvk, each reached with NULL contexts (they run before a context is looked at);
the Python layer's shape checks; and the model (tests/tree_mvk_reference.py) decrypting every (hi, lo) at p_hi = p_lo = 4, k = 3 on reduced keys."""
import ctypes as C

import numpy as np
import pytest

import lut_reference as R
import tree_mvk_reference as TK

N = 1024


def _spec(thfhe, n_inputs=1, weights=(1, 0, 0), bias=0, theta=1):
    return thfhe.LutSpec(n_inputs, (C.c_int32 * 3)(*weights), bias, theta)


def test_symbol_and_binding():
    import thfhe
    assert "thfhe_tree_lut_bootstrap_mvk" in thfhe.SIGNATURES and hasattr(thfhe.lib(), "thfhe_tree_lut_bootstrap_mvk")
    assert len(thfhe.SIGNATURES["thfhe_tree_lut_bootstrap_mvk"][1]) == len(thfhe.SIGNATURES["thfhe_tree_lut_bootstrap_mv"][1]) + 1


def test_tree_mvk_factors_are_the_stacked_tree_mv_factors():
    from thfhe import lut
    rng = np.random.default_rng(3)
    T = rng.integers(0, 2, (3, 4, 8))
    fs = [lambda h, l, j=j: T[j, h, l] for j in range(3)]
    tv0, w = lut.tree_mvk_factors(fs, 4, 8)
    assert w.shape == (3, 4, 8) and w.dtype == np.int32 and tv0.shape == (N,)
    for j in range(3):
        tv0_j, w_j = lut.tree_mv_factors(fs[j], 4, 8, 2)
        assert np.array_equal(tv0, tv0_j) and np.array_equal(w[j], w_j)
    assert np.array_equal(tv0, lut.mv_base(1 << 30))                       # p_out = 2 by default: step 2^32 / 4
    tv0_4, w_4 = lut.tree_mvk_factors([lambda h, l: h + l], 4, 4, p_out=4)
    assert np.array_equal(tv0_4, lut.mv_base(1 << 29)) and np.array_equal(w_4[0], lut.tree_mv_factors(lambda h, l: h + l, 4, 4, 4)[1])
    # the flattened table is what one multi-value rotation with q = k p_hi outputs takes: output j p_hi + h = candidate h of function j
    flat = w.reshape(12, 8)
    assert np.array_equal(flat[2 * 4 + 3], lut.mv_factors([T[2, 3]], 8)[0])
    for bad in (lambda: lut.tree_mvk_factors([], 4, 4), lambda: lut.tree_mvk_factors(fs * 6, 4, 8), lambda: lut.tree_mvk_factors(fs, 3, 8)):
        with pytest.raises(ValueError):
            bad()
    assert lut.tree_mvk_factors(fs * 5 + fs[:1], 4, 8)[1].shape == (16, 4, 8)                     # k p_hi = 64 is allowed


def test_entry_validates_arguments_before_a_context_is_touched():
    import thfhe
    L = thfhe.lib()
    i32 = C.POINTER(C.c_int32)
    tv = np.zeros(N, np.int32)
    w = np.zeros((2, 64, 64), np.int32)
    rec = np.zeros((4, 631), np.int32)
    out = np.zeros(4 * 32 * 631, np.int32)
    ptv, pw, prec, pout = tv.ctypes.data_as(i32), w.ctypes.data_as(i32), rec.ctypes.data_as(i32), out.ctypes.data_as(i32)
    err = L.thfhe_last_error
    ok = _spec(thfhe)
    tree = L.thfhe_tree_lut_bootstrap_mvk
    call = lambda lo=ok, hi=ok, p_hi=4, p_lo=4, k=2, tv0=ptv, f=pw, n_tables=1, idx=None, lo0=prec, lo1=None, hi0=prec, hi1=None, o=pout, count=4: tree(
        None, None, None if lo is None else C.byref(lo), None if hi is None else C.byref(hi), p_hi, p_lo, k, tv0, f, n_tables, idx, lo0, lo1, None, hi0, hi1,
        None, o, count)
    # those of thfhe_tree_lut_bootstrap_mv ...
    for kw in (dict(lo=None), dict(hi=None), dict(tv0=None), dict(f=None), dict(lo0=None), dict(hi0=None), dict(o=None)):
        assert call(**kw) == -1 and b"null" in err(), kw
    assert call(lo=_spec(thfhe, n_inputs=2)) == -1 and b"null operand" in err()
    assert call(hi=_spec(thfhe, n_inputs=3), hi1=prec) == -1 and b"null operand" in err()
    assert call(lo=_spec(thfhe, n_inputs=4), lo1=prec) == -1 and b"n_inputs" in err()
    assert call(lo=_spec(thfhe, theta=3)) == -1 and b"theta" in err()
    assert call(lo=_spec(thfhe, theta=2)) == -1 and b"theta must be 1" in err()
    assert call(hi=_spec(thfhe, theta=4)) == -1 and b"spec_hi theta" in err()
    for bad in (0, 1, 3, 6, 1024, -4):
        assert call(p_hi=bad) == -1 and b"p_hi" in err(), bad
    assert call(p_hi=128, k=1) == -1 and b"q must be" in err()
    for bad in (0, 1, 3, 128):
        assert call(p_lo=bad) == -1 and b"p must be" in err(), bad
    for bad in (0, 1025, -1):
        assert call(n_tables=bad) == -1 and b"n_tables" in err(), bad
    idx = np.array([0, 1, 2, 0], np.int32)
    assert call(n_tables=2, idx=idx.ctypes.data_as(i32)) == -1 and b"table_index" in err()
    # ... then k and k p_hi
    for bad in (0, -1, -(1 << 31)):
        assert call(k=bad) == -1 and b"k must be" in err(), bad
    for p_hi, k in ((4, 17), (64, 2), (2, 33), (8, 9), (32, 1 << 30)):
        assert call(p_hi=p_hi, k=k) == -1 and b"k p_hi must be at most 64" in err(), (p_hi, k)
    # every check comes before the contexts: valid calls get as far as the missing context, at the limits of k p_hi, and so does count 0
    idx = np.array([0, 1, 1, 0], np.int32)
    for p_hi, p_lo, k in ((2, 2, 1), (4, 8, 3), (8, 8, 4), (2, 64, 32), (64, 2, 1), (4, 4, 16)):
        assert call(p_hi=p_hi, p_lo=p_lo, k=k, n_tables=2, idx=idx.ctypes.data_as(i32)) == -1 and b"null ctx" in err(), (p_hi, p_lo, k)
    assert call(count=0) == -1 and b"null ctx" in err()
    # the k = 1 wrapper keeps its own checks
    assert L.thfhe_tree_lut_bootstrap_mv(None, None, C.byref(ok), C.byref(ok), 128, 4, ptv, pw, 1, None, prec, None, None, prec, None, None, pout, 4) == -1
    assert b"q must be" in err()


def test_python_layer_checks_shapes_before_the_library():
    import thfhe
    ck = thfhe.CloudKey.__new__(thfhe.CloudKey)
    ck.params, ck.words, ck.h = thfhe.make_params("SK-128"), 631, None
    x = np.zeros((3, 631), np.int32)
    tv0 = np.zeros(N, np.int32)

    class Pc:
        h = None
    for bad in (dict(factors=np.zeros((4, 4), np.int32)), dict(factors=np.zeros((2, 2, 2, 2, 2), np.int32)), dict(tv0=np.zeros(5, np.int32)),
                dict(table_index=[0, 0]), dict(hi=x[:2]), dict(weights_lo=(1, 2))):
        kw = dict(factors=np.zeros((2, 4, 4), np.int32), lo=x, hi=x, tv0=tv0)
        kw.update(bad)
        with pytest.raises(ValueError):
            ck.tree_lut_bootstrap_mvk(Pc, kw.pop("factors"), kw.pop("lo"), kw.pop("hi"), **kw)
    with pytest.raises(thfhe.ThfheError, match="null ctx"):      # a well-formed call reaches the library
        ck.tree_lut_bootstrap_mvk(Pc, np.zeros((2, 4, 4), np.int32), x, x, tv0=tv0)


def test_model_decrypts_every_pair_at_p4_k3(sk_small):
    # SK-128's ring, gadget and key-switch shape at n = 16: three bit-valued functions of two p = 4 digits in 1 + 3 rotations
    from thfhe import keygen, lut
    p, K, orc = sk_small
    pk = keygen.gen_pack_key(np.random.default_rng(11), K.lwe_key, K.rlwe_key[0], p.ks_t, p.ks_basebit, 2.0**-25)
    fs = [lambda h, l: (h + l) & 1, lambda h, l: int(h > l), lambda h, l: (h * l >> 1) & 1]
    tv0, w = lut.tree_mvk_factors(fs, 4, 4)
    hi, lo = np.repeat(np.arange(4), 4), np.tile(np.arange(4), 4)
    xh, xl = R.encrypt_words(K, lut.encode(hi, 4), 2.0**-15, 51), R.encrypt_words(K, lut.encode(lo, 4), 2.0**-15, 52)
    for g in range(16):
        out, cands = TK.tree_mvk(orc, pk, p.ks_t, p.ks_basebit, [xl[g]], (1,), 0, [xh[g]], (1,), 0, tv0, w)
        assert out.shape == (3, p.n + 1) and cands.shape == (12, p.n + 1)
        want = [f(int(hi[g]), int(lo[g])) for f in fs]
        assert lut.decode(K.phases(out), 2).tolist() == want, (g, want)
        # candidate j p_hi + h carries f_j(h, lo)
        assert lut.decode(K.phases(cands), 2).tolist() == [f(h, int(lo[g])) for f in fs for h in range(4)], g
