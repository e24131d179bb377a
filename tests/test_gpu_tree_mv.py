"""The two-digit tree with a multi-value level 1 on the MI355X (pytest -m gpu): thfhe_tree_lut_bootstrap_mv word for
word against the three public calls in a row (thfhe_mv_lut_bootstrap -> thfhe_pack_boxes -> thfhe_lut_bootstrap_enc) and against the model
composed from the CPU oracle (mv_lut_reference.tree_mv) on a sample of jobs.  SK-128; the packing key maps the gate key set's LWE key to its
bootstrapping ring key.

Noise: a candidate carries the rotation's noise times the 2-norm of its factor, and the selection adds a second rotation and key switch
(DESIGN 4.13).  Decrypt-exactness is asserted on tables inside that section's supported set, for which the model alone, run on the CPU on
the same seeds, decrypts every sample: the digit table of test_every_pair_at_p4 (p_out = 4, |c|_2 <= 3.5: std 8.4e-3, largest error 1.6e-2
of the half-step 6.3e-2) and a random 6-bit -> 1-bit table (p_out = 2, |c|_2 <= 3.2: largest error 1.6e-2 of 1.25e-1).  The random
6-bit -> 3-bit table (p_out = 8, |c|_2 up to 15.4) is outside it -- the model decrypts 54 of its 64 samples, std 2.4e-2 against the
half-step 3.1e-2 -- so it is checked word for word only, and its 1-bit companion is the one that must decrypt."""
import ctypes as C

import numpy as np
import pytest

import mv_lut_reference as MV
from support import N, SIGMA_BK, dec_int, enc_int, pmap, sk128_cloud_key, sk128_pack, words

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ck(sk128):
    yield from sk128_cloud_key(sk128)


@pytest.fixture(scope="module")
def pack(sk128):
    yield from sk128_pack(sk128)


def compose(ck, pc, tv0, w, lo, hi, w_lo=(1,), b_lo=0, w_hi=(1,), b_hi=0, table_index=None):
    """the three public calls in a row"""
    from thfhe import threshold as T
    w = w if w.ndim == 3 else w[None]
    cands = ck.mv_lut_bootstrap(w, *lo, tv0=tv0, weights=w_lo, bias=b_lo, table_index=table_index)
    a, b = T.PackBoxes(pc, cands.reshape(-1, cands.shape[-1]), w.shape[1])
    return ck.lut_bootstrap_enc(a, b, *hi, weights=w_hi, bias=b_hi, lut_index=np.arange(len(a)))[:, 0]


def model(orc, pk, p, tv0, w, lo, hi, g, **kw):
    return MV.tree_mv(orc, pk, p.ks_t, p.ks_basebit, [x[g] for x in lo], kw.get("w_lo", (1,)), kw.get("b_lo", 0), [x[g] for x in hi],
                      kw.get("w_hi", (1,)), kw.get("b_hi", 0), tv0, w)[0]


# f(hi, lo) at p = 4 -> p_out = 4 whose rows have |c|_2 <= 3.5: hi picks one of the digit tables lo -> lo, 3 - lo, (1, 1, 2, 2), (0, 1, 1, 0)
P4_TABLE = np.array([[0, 1, 2, 3], [3, 2, 1, 0], [1, 1, 2, 2], [0, 1, 1, 0]])


def test_every_pair_at_p4(sk128, ck, pack):
    from thfhe import lut
    p, K, orc = sk128
    pc, pk = pack
    F = P4_TABLE
    tv0, w = lut.tree_mv_factors(lambda h, l: F[h, l], 4, 4, 4)
    hi, lo = np.repeat(np.arange(4), 4), np.tile(np.arange(4), 4)
    xh, xl = enc_int(K, hi, 4, 4100), enc_int(K, lo, 4, 4101)
    got = ck.tree_lut_bootstrap_mv(pc, w, xl, xh, tv0=tv0)
    assert got.shape == (16, p.n + 1)
    assert np.array_equal(got, compose(ck, pc, tv0, w, [xl], [xh]))
    picks = [0, 5, 10, 15]
    ref = np.stack(pmap(lambda g: model(orc, pk, p, tv0, w, [xl], [xh], g), picks))
    assert np.array_equal(got[picks], ref)
    err = (K.phases(got).astype(np.int64) - lut.encode(F[hi, lo], 4).astype(np.int64) + 2**31) % 2**32 - 2**31
    print(f"\ntree_mv p = 4, p_out = 4: std of phase - encode {np.std(err / 2.0**32):.3e} (largest {np.abs(err).max() / 2.0**32:.3e}, half-step 6.25e-02)")
    assert np.array_equal(dec_int(K, got, 4), F[hi, lo])
    # the decoded outputs agree with the tree of one-row rotations on the same inputs (messages, not words: the noise differs)
    old = ck.tree_lut_bootstrap(pc, lut.tree_test_vectors(lambda h, l: F[h, l], 4, 4, 4), xl, xh, p_hi=4)
    assert np.array_equal(dec_int(K, old, 4), dec_int(K, got, 4))


def test_six_bits_to_three_and_to_one(sk128, ck, pack):
    # p = 8 digits, 1 + 1 rotations where thfhe_tree_lut_bootstrap spends 4 + 1: a random 6-bit -> 3-bit table, every word against the three
    # calls and the model (outside the supported noise set, see the module docstring), and a 6-bit -> 1-bit table that must decrypt
    from thfhe import lut
    p, K, orc = sk128
    pc, pk = pack
    rng = np.random.default_rng(4200)
    hi, lo = np.repeat(np.arange(8), 8), np.tile(np.arange(8), 8)
    xh, xl = enc_int(K, hi, 8, 4200), enc_int(K, lo, 8, 4201)
    for p_out in (8, 2):
        F = rng.integers(0, p_out, (8, 8))
        tv0, w = lut.tree_mv_factors(lambda h, l: F[h, l], 8, 8, p_out)
        got = ck.tree_lut_bootstrap_mv(pc, w, xl, xh, tv0=tv0)
        assert np.array_equal(got, compose(ck, pc, tv0, w, [xl], [xh]))
        picks = [0, 27, 63]
        assert np.array_equal(got[picks], np.stack(pmap(lambda g: model(orc, pk, p, tv0, w, [xl], [xh], g), picks)))
        dec = dec_int(K, got, p_out)
        print(f"\ntree_mv p = 8, p_out = {p_out}: {int((dec == F[hi, lo]).sum())} of 64 decrypt, |c|_2 up to {np.sqrt((w.astype(float) ** 2).sum(-1)).max():.1f}")
        if p_out == 2:
            assert np.array_equal(dec, F[hi, lo])
            old = ck.tree_lut_bootstrap(pc, lut.tree_test_vectors(lambda h, l: F[h, l], 8, 8, 2, theta=2), xl, xh, p_hi=8, theta=2)
            assert np.array_equal(dec_int(K, old, 2), dec)


def test_slices_table_index_and_weighted_operands(sk128, ck, pack):
    # 13 samples, three tables chosen per sample, two weighted `lo` and three weighted `hi` operands with both biases, random words everywhere:
    # whole, in slices of 3 samples (12 candidates) and one sample per slice, against the three calls
    p, K, orc = sk128
    pc, pk = pack
    rng = np.random.default_rng(4300)
    count = 13
    word = lambda *shape: words(rng, *shape)
    tv0, w = word(N), word(3, 4, 16)                              # p_hi = 4 candidates of p_lo = 16 taps
    lo, hi = [word(count, p.n + 1) for _ in range(2)], [word(count, p.n + 1) for _ in range(3)]
    tab = rng.integers(0, 3, count).astype(np.int32)
    kw = dict(tv0=tv0, weights_lo=(3, -5), bias_lo=0x12345678, weights_hi=(-2, 9, 1), bias_hi=-0x0abcdef1, table_index=tab)
    whole = ck.tree_lut_bootstrap_mv(pc, w, tuple(lo), tuple(hi), **kw)
    try:
        ck.set_tree_slice(12)
        sliced = ck.tree_lut_bootstrap_mv(pc, w, tuple(lo), tuple(hi), **kw)
        ck.set_tree_slice(1)     # below p_hi: one sample per slice
        single = ck.tree_lut_bootstrap_mv(pc, w, tuple(x[:3] for x in lo), tuple(x[:3] for x in hi), **dict(kw, table_index=tab[:3]))
    finally:
        ck.set_tree_slice(65536)
    assert np.array_equal(sliced, whole) and np.array_equal(single, whole[:3])
    assert np.array_equal(whole, compose(ck, pc, tv0, w, lo, hi, w_lo=(3, -5), b_lo=0x12345678, w_hi=(-2, 9, 1), b_hi=-0x0abcdef1, table_index=tab))
    g = 12
    ref = model(orc, pk, p, tv0, w[tab[g]], lo, hi, g, w_lo=(3, -5), b_lo=0x12345678, w_hi=(-2, 9, 1), b_hi=-0x0abcdef1)
    assert np.array_equal(whole[g], ref)


def test_error_paths_leave_both_contexts_usable(sk128, ck, pack):
    import thfhe
    from thfhe import keygen, lut
    from thfhe import threshold as T
    p, K, orc = sk128
    pc, pk = pack
    tv0, w = lut.tree_mv_factors(lambda h, l: P4_TABLE[h, l], 4, 4, 4)
    xh, xl = enc_int(K, [1, 2, 3], 4, 4400), enc_int(K, [3, 0, 2], 4, 4401)
    want = ck.tree_lut_bootstrap_mv(pc, w, xl, xh, tv0=tv0)
    assert np.array_equal(dec_int(K, want, 4), P4_TABLE[[1, 2, 3], [3, 0, 2]])
    bare = T.PolyContext(0)
    with pytest.raises(thfhe.ThfheError, match="error -1.*no packing key"):
        ck.tree_lut_bootstrap_mv(bare, w, xl, xh, tv0=tv0)
    bare.set_pack_key(keygen.gen_pack_key(np.random.default_rng(5), K.lwe_key[:10], K.rlwe_key[0], 8, 2, SIGMA_BK), 8, 2)
    with pytest.raises(thfhe.ThfheError, match="error -1.*dimension"):
        ck.tree_lut_bootstrap_mv(bare, w, xl, xh, tv0=tv0)
    bare.close()
    with pytest.raises(thfhe.ThfheError, match="error -1.*table_index"):
        ck.tree_lut_bootstrap_mv(pc, w, xl, xh, tv0=tv0, table_index=[0, 1, 0])
    with pytest.raises(thfhe.ThfheError, match="error -1.*p must be"):
        ck.tree_lut_bootstrap_mv(pc, np.zeros((4, 3), np.int32), xl, xh, tv0=tv0)
    with pytest.raises(thfhe.ThfheError, match="error -1.*p_hi"):
        ck.tree_lut_bootstrap_mv(pc, np.zeros((3, 4), np.int32), xl, xh, tv0=tv0)
    spec, spec2 = thfhe.LutSpec(1, (C.c_int32 * 3)(1, 0, 0), 0, 1), thfhe.LutSpec(1, (C.c_int32 * 3)(1, 0, 0), 0, 2)
    i32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    out = np.zeros((3, p.n + 1), np.int32)
    tree = thfhe.lib().thfhe_tree_lut_bootstrap_mv
    args = lambda lo, hi: (ck.h, pc.h, C.byref(lo), C.byref(hi), 4, 4, i32(tv0), i32(w), 1, None, i32(xl), None, None, i32(xh), None, None, i32(out), 3)
    assert tree(*args(spec2, spec)) == -1 and b"theta must be 1" in thfhe.lib().thfhe_last_error()
    assert tree(*args(spec, spec2)) == -1 and b"spec_hi theta" in thfhe.lib().thfhe_last_error()
    assert ck.tree_lut_bootstrap_mv(pc, w, xl[:0], xh[:0], tv0=tv0).shape == (0, p.n + 1)
    # both contexts still work, and give the same words
    assert np.array_equal(ck.tree_lut_bootstrap_mv(pc, w, xl, xh, tv0=tv0), want)
    assert np.array_equal(ck.tree_lut_bootstrap(pc, lut.tree_test_vectors(lambda h, l: P4_TABLE[h, l], 4, 4, 4), xl, xh, p_hi=4).shape, want.shape)
