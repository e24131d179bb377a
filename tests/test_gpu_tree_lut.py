"""Encrypted lookup tables and the two-digit tree PBS on the MI355X (pytest -m gpu): thfhe_lut_bootstrap_enc,
thfhe_pack_boxes and thfhe_tree_lut_bootstrap word for word against the model composed from the CPU oracle (tree_lut_reference.py) on a sample
of jobs, and decrypt-exact on all of them.  SK-128 throughout; the packing key maps the gate key set's LWE key to its bootstrapping ring key."""
import ctypes as C

import numpy as np
import pytest

import lut_reference as R
import pack_reference as PR
import tree_lut_reference as TR
from support import N, SIGMA, SIGMA_BK, dec_int, enc_int, pmap, sk128_cloud_key, sk128_pack, thresholds, words

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ck(sk128):
    yield from sk128_cloud_key(sk128)


@pytest.fixture(scope="module")
def pack(sk128):
    yield from sk128_pack(sk128)


def ring_phase_at0(K, u):
    """phase of LWE(N) records under the ring key (the _wo_keyswitch outputs)."""
    u = np.asarray(u, np.int64).reshape(-1, N + 1)
    return PR.wrap32(u[:, N] - (u[:, :N] * K.rlwe_key[0].astype(np.int64)).sum(axis=1))


# ---- (a) rotation of an encrypted test vector -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("theta", [1, 2, 4])
def test_enc_fresh_tables_equal_the_model_and_decrypt(sk128, ck, theta):
    # three fresh encrypted tables of theta functions each, random per-sample index: word for word with and without the key switch
    from thfhe import lut
    p, K, orc = sk128
    rng = np.random.default_rng(40 + theta)
    F = rng.integers(0, 4, (3, theta, 4))
    tvs = np.stack([lut.test_vector([lut.int_outputs(lambda m, f=f: f[m], 4) for f in Ft], 4, theta=theta) for Ft in F])
    tv_a, tv_b = lut.encrypt_table(K.rlwe_key[0], tvs, SIGMA_BK, rng)
    m = np.tile(np.arange(4), 3)
    idx = rng.integers(0, 3, 12).astype(np.int32)
    x = enc_int(K, m, 4, 1000 + theta)
    u = ck.lut_bootstrap_enc_wo_keyswitch(tv_a, tv_b, x, theta=theta, lut_index=idx)
    got = ck.lut_bootstrap_enc(tv_a, tv_b, x, theta=theta, lut_index=idx)
    assert u.shape == (12, theta, N + 1) and got.shape == (12, theta, p.n + 1)
    for g in (0, 5, 11):
        wo = TR.lut_enc(orc, [x[g]], (1,), 0, tv_a[idx[g]], tv_b[idx[g]], theta, keyswitch=False)
        assert np.array_equal(u[g], wo)
        assert np.array_equal(got[g], np.stack([orc.keyswitch(r) for r in wo]))
    want = F[idx, :, m]
    assert np.array_equal(dec_int(K, got.reshape(-1, p.n + 1), 4).reshape(12, theta), want)
    from thfhe import lut as L
    assert np.array_equal(L.decode(ring_phase_at0(K, u), 4).reshape(12, theta), want)


def test_enc_on_every_kernel_shape_with_random_words(sk128, ck):
    # random TLWE words (no structure), weights and bias, on the eight-wave ring, four-wave ring, cooperative, and 6 + 6 split
    p, K, orc = sk128
    rng = np.random.default_rng(77)
    recs = [R.encrypt_words(K, rng.integers(-2**31, 2**31, 12), SIGMA, 1100 + q) for q in range(2)]
    weights, bias = (3, -5), int(rng.integers(-2**31, 2**31))
    tv_a, tv_b = (words(rng, 3, N) for _ in range(2))
    idx = rng.integers(0, 3, 12).astype(np.int32)
    for theta in (1, 4):
        kw = dict(weights=weights, bias=bias, theta=theta, lut_index=idx)
        wo = np.stack(pmap(lambda g: TR.lut_enc(orc, [r[g] for r in recs], weights, bias, tv_a[idx[g]], tv_b[idx[g]], theta, keyswitch=False), range(12)))
        ks = np.stack([np.stack([orc.keyswitch(u) for u in s]) for s in wo])
        for coop, ring4 in ((0, 0), (0, 1024), (1 << 20, 1024), (5, 6)):
            with thresholds(ck, coop, ring4):
                assert np.array_equal(ck.lut_bootstrap_enc_wo_keyswitch(tv_a, tv_b, *recs, **kw), wo), (theta, coop, ring4)
                assert np.array_equal(ck.lut_bootstrap_enc(tv_a, tv_b, *recs, **kw), ks), (theta, coop, ring4)


def test_enc_zero_mask_is_the_plaintext_entry(sk128, ck):
    p, K, orc = sk128
    rng = np.random.default_rng(78)
    x = R.encrypt_words(K, rng.integers(-2**31, 2**31, 20), SIGMA, 1200)
    tvs = words(rng, 4, N)
    idx = rng.integers(0, 4, 20).astype(np.int32)
    for theta in (1, 2, 4):
        kw = dict(weights=(-3,), bias=99, theta=theta, lut_index=idx)
        assert np.array_equal(ck.lut_bootstrap_enc(np.zeros_like(tvs), tvs, x, **kw), ck.lut_bootstrap(tvs, x, **kw))
        assert np.array_equal(ck.lut_bootstrap_enc_wo_keyswitch(np.zeros_like(tvs), tvs, x, **kw), ck.lut_bootstrap_wo_keyswitch(tvs, x, **kw))
    assert np.array_equal(ck.lut_bootstrap_enc(np.zeros_like(tvs), tvs, x), ck.lut_bootstrap(tvs[:1], x))   # no index: table 0


def test_enc_one_table_per_sample_above_1024(sk128, ck):
    # 1 100 samples, each with its own fresh encrypted table (the plaintext entry stops at 1 024 tables)
    from thfhe import lut
    p, K, orc = sk128
    rng = np.random.default_rng(79)
    count = 1100
    F = rng.integers(0, 4, (count, 4))
    tvs = np.stack([lut.test_vector(lut.int_outputs(lambda m, f=f: f[m], 4), 4) for f in F])
    tv_a, tv_b = lut.encrypt_table(K.rlwe_key[0], tvs, SIGMA_BK, rng)
    m = rng.integers(0, 4, count)
    x = enc_int(K, m, 4, 1300)
    got = ck.lut_bootstrap_enc(tv_a, tv_b, x, lut_index=np.arange(count))
    assert np.array_equal(dec_int(K, got[:, 0], 4), F[np.arange(count), m])
    for g in (0, 1023, 1024, 1099):
        assert np.array_equal(got[g], TR.lut_enc(orc, [x[g]], (1,), 0, tv_a[g], tv_b[g], 1))


# ---- (b) packing into boxes ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("p_box,outs", [(2, 5), (8, 3), (16, 64), (512, 2)])
def test_pack_boxes_equals_the_model(sk128, pack, p_box, outs):
    from thfhe import threshold as T
    p, K, orc = sk128
    pc, pk = pack
    rng = np.random.default_rng(p_box)
    lwe = words(rng, p_box * outs, p.n + 1)
    lwe[0, :p.n], lwe[-1, :p.n] = -2**31, 2**31 - 1
    a, b = T.PackBoxes(pc, lwe, p_box)
    ra, rb = TR.pack_boxes(lwe, pk, p.ks_t, p.ks_basebit, p_box)
    assert a.shape == ra.shape == (outs, N)
    assert np.array_equal(a, ra) and np.array_equal(b, rb)


def test_pack_boxes_noise_against_the_prediction(sk128, pack):
    # 256 x 16 fresh samples: every coefficient of box i carries sample i's phase + its rounding (once) + the key noise of all N/p shifted
    # copies of the p samples, i.e. the m = N case of section 4.10's prediction
    from thfhe import threshold as T
    p, K, orc = sk128
    pc, pk = pack
    rng = np.random.default_rng(16)
    m = rng.integers(0, 8, 4096)
    lwe = enc_int(K, m, 8, 1400)
    a, b = T.PackBoxes(pc, lwe, 16)
    ph = PR.tlwe_phase(a, b, K.rlwe_key[0])                                   # [256][N]
    src = np.roll(np.repeat(K.phases(lwe).reshape(256, 16), 64, axis=1).astype(np.int64), -32, axis=1)   # coefficient c belongs to box (c + 32) // 64
    src[:, N - 32:] *= -1                                                     # the wrapped half-box of candidate 0
    err = PR.torus(PR.wrap32(ph.astype(np.int64) - src))
    pred = PR.predicted_sigma(N, p.n, p.ks_t, p.ks_basebit, int(K.lwe_key.sum()), SIGMA_BK)
    print("box noise: measured", err.std(), "predicted", pred)
    assert 0.5 * pred <= err.std() <= 1.5 * pred, (err.std(), pred)
    from thfhe import lut
    assert np.array_equal(lut.decode(ph[:, ::64], 8).reshape(-1), m)


# ---- (c) the tree ----------------------------------------------------------------------------------------------------------------------------

def compose(ck, pc, tv1, lo, hi, p_hi, theta, w_lo=(1,), b_lo=0, w_hi=(1,), b_hi=0, table_index=None):
    """The three public entries in a row: thfhe_lut_bootstrap on replicated inputs -> thfhe_pack_boxes -> thfhe_lut_bootstrap_enc."""
    from thfhe import threshold as T
    Rr, count = p_hi // theta, lo[0].shape[0]
    tab = np.zeros(count, np.int64) if table_index is None else np.asarray(table_index, np.int64)
    idx = np.repeat(tab, Rr) * Rr + np.tile(np.arange(Rr), count)
    c1 = ck.lut_bootstrap(np.asarray(tv1).reshape(-1, N), *[np.repeat(x, Rr, axis=0) for x in lo], weights=w_lo, bias=b_lo, theta=theta, lut_index=idx)
    a, b = T.PackBoxes(pc, c1.reshape(count * p_hi, -1), p_hi)
    return ck.lut_bootstrap_enc(a, b, *hi, weights=w_hi, bias=b_hi, lut_index=np.arange(count))[:, 0]


def model(orc, pk, p, tv1_of, lo, hi, g, theta, p_hi, w_lo=(1,), b_lo=0, w_hi=(1,), b_hi=0):
    return TR.tree(orc, pk, p.ks_t, p.ks_basebit, [x[g] for x in lo], w_lo, b_lo, theta, [x[g] for x in hi], w_hi, b_hi, tv1_of, p_hi)[0]


@pytest.mark.parametrize("theta", [1, 2, 4])
def test_tree_every_pair_at_p4(sk128, ck, pack, theta):
    from thfhe import lut
    p, K, orc = sk128
    pc, pk = pack
    F = np.random.default_rng(50 + theta).integers(0, 4, (4, 4))
    tv1 = lut.tree_test_vectors(lambda h, l: F[h, l], 4, 4, 4, theta=theta)
    hi, lo = np.repeat(np.arange(4), 4), np.tile(np.arange(4), 4)
    xh, xl = enc_int(K, hi, 4, 1500 + theta), enc_int(K, lo, 4, 1510 + theta)
    got = ck.tree_lut_bootstrap(pc, tv1, xl, xh, p_hi=4, theta=theta)
    assert got.shape == (16, p.n + 1)
    # decrypt-exact on all 16 pairs; word for word against the model on six of them (the model alone, run on these seeds, decrypts all 16)
    assert np.array_equal(dec_int(K, got, 4), F[hi, lo])
    picks = [0, 3, 6, 9, 12, 15]
    ref = np.stack(pmap(lambda g: model(orc, pk, p, tv1, [xl], [xh], g, theta, 4), picks))
    assert np.array_equal(dec_int(K, ref, 4), F[hi[picks], lo[picks]])
    assert np.array_equal(got[picks], ref)
    assert np.array_equal(got, compose(ck, pc, tv1, [xl], [xh], 4, theta))


def test_tree_six_bits_to_three(sk128, ck, pack):
    # p = 8 digits, theta1 = 2, p_out = 8: a 6-bit -> 3-bit function in 4 + 1 rotations, every (hi, lo) pair
    from thfhe import lut
    p, K, orc = sk128
    pc, pk = pack
    F = np.random.default_rng(60).integers(0, 8, (8, 8))
    tv1 = lut.tree_test_vectors(lambda h, l: F[h, l], 8, 8, 8, theta=2)
    hi, lo = np.repeat(np.arange(8), 8), np.tile(np.arange(8), 8)
    xh, xl = enc_int(K, hi, 8, 1600), enc_int(K, lo, 8, 1601)
    got = ck.tree_lut_bootstrap(pc, tv1, xl, xh, p_hi=8, theta=2)
    assert np.array_equal(dec_int(K, got, 8), F[hi, lo])
    picks = [0, 9, 18, 27, 36, 45, 54, 63]                    # the model alone, run on these seeds, decrypts all 64 (202 s on one core)
    ref = np.stack(pmap(lambda g: model(orc, pk, p, tv1, [xl], [xh], g, 2, 8), picks))
    assert np.array_equal(dec_int(K, ref, 8), F[hi[picks], lo[picks]])
    assert np.array_equal(got[picks], ref)
    err = PR.torus(PR.wrap32(K.phases(got).astype(np.int64) - lut.encode(F[hi, lo], 8)))
    print("tree p=8 theta1=2 p_out=8: std of phase(out) - encode(f) on 64 samples", err.std(), "max", np.abs(err).max())


def test_tree_on_gate_outputs(sk128, ck, pack):
    # both digits are built from gate outputs: NAND -> from_gate_bit-style LUT (bias 1/8, p = 2 -> p = 4) -> digit = b0 + 2 b1, so every
    # tree input is key-switched twice over; f(hi, lo) = hi * lo + 1 mod 4, per-sample table index over two tables
    import thfhe
    from thfhe import lut
    p, K, orc = sk128
    pc, pk = pack
    rng = np.random.default_rng(70)
    count = 32
    bits = rng.integers(0, 2, (8, count))
    enc = [K.encrypt_bits(list(b), SIGMA, 1700 + i) for i, b in enumerate(bits)]
    g = [thfhe.gate_nand(ck, enc[2 * i], enc[2 * i + 1]) for i in range(4)]
    gb = [1 - (bits[2 * i] & bits[2 * i + 1]) for i in range(4)]
    tv_bit = lut.test_vector(lut.int_outputs(lambda m: m, 4, p=2), 2)
    b = [ck.lut_bootstrap(tv_bit, w, bias=lut.MU8)[:, 0] for w in g]
    lo_m, hi_m = gb[0] + 2 * gb[1], gb[2] + 2 * gb[3]
    fs = [lambda h, l: h * l + 1, lambda h, l: h + 3 * l]
    tv1 = np.stack([lut.tree_test_vectors(f, 4, 4, 4, theta=2) for f in fs])
    tab = rng.integers(0, 2, count).astype(np.int32)
    kw = dict(p_hi=4, theta=2, weights_lo=(1, 2), weights_hi=(1, 2), table_index=tab)
    got = ck.tree_lut_bootstrap(pc, tv1, (b[0], b[1]), (b[2], b[3]), **kw)
    want = np.where(tab == 0, hi_m * lo_m + 1, hi_m + 3 * lo_m) % 4
    assert np.array_equal(dec_int(K, got, 4), want)
    picks = [0, 5, 11, 17, 23, 31]
    ref = np.stack(pmap(lambda s: model(orc, pk, p, tv1[tab[s]], [b[0], b[1]], [b[2], b[3]], s, 2, 4, w_lo=(1, 2), w_hi=(1, 2)), picks))
    assert np.array_equal(dec_int(K, ref, 4), want[picks])
    assert np.array_equal(got[picks], ref)
    assert np.array_equal(got, compose(ck, pc, tv1, [b[0], b[1]], [b[2], b[3]], 4, 2, w_lo=(1, 2), w_hi=(1, 2), table_index=tab))


def test_tree_slices_and_table_index(sk128, ck, pack):
    # 37 samples in slices of 10 (40 candidates at p_hi = 4): the same words as one slice and as the three-call composition
    from thfhe import lut
    p, K, orc = sk128
    pc, pk = pack
    rng = np.random.default_rng(80)
    count = 37
    F = rng.integers(0, 4, (3, 4, 4))
    tv1 = np.stack([lut.tree_test_vectors(lambda h, l, f=f: f[h, l], 4, 4, 4, theta=1) for f in F])
    tab = rng.integers(0, 3, count).astype(np.int32)
    hi, lo = rng.integers(0, 4, count), rng.integers(0, 4, count)
    xh, xl = enc_int(K, hi, 4, 1800), enc_int(K, lo, 4, 1801)
    whole = ck.tree_lut_bootstrap(pc, tv1, xl, xh, p_hi=4, table_index=tab)
    try:
        ck.set_tree_slice(40)
        sliced = ck.tree_lut_bootstrap(pc, tv1, xl, xh, p_hi=4, table_index=tab)
        ck.set_tree_slice(1)     # below p_hi: one sample per slice
        single = ck.tree_lut_bootstrap(pc, tv1, xl[:5], xh[:5], p_hi=4, table_index=tab[:5])
    finally:
        ck.set_tree_slice(65536)
    assert np.array_equal(sliced, whole) and np.array_equal(single, whole[:5])
    assert np.array_equal(whole, compose(ck, pc, tv1, [xl], [xh], 4, 1, table_index=tab))
    assert np.array_equal(dec_int(K, whole, 4), F[tab, hi, lo])
    picks = [0, 9, 10, 36]
    assert np.array_equal(whole[picks], np.stack(pmap(lambda g: model(orc, pk, p, tv1[tab[g]], [xl], [xh], g, 1, 4), picks)))


def test_tree_three_lo_and_three_hi_operands_in_slices(sk128, ck, pack):
    # p_hi = 8, theta1 = 4 (R = 2), two tables chosen per sample, three weighted `lo` and three weighted `hi` operands with both biases, 10 samples
    # in slices of 3 (24 candidates).  Random record and table words: every word of the output against the three-call composition.
    p, K, orc = sk128
    pc, pk = pack
    rng = np.random.default_rng(90)
    count = 10
    word = lambda *shape: words(rng, *shape)
    tv1 = word(2, 2, N)
    lo, hi = [word(count, p.n + 1) for _ in range(3)], [word(count, p.n + 1) for _ in range(3)]
    tab = rng.integers(0, 2, count).astype(np.int32)
    w_lo, w_hi, b_lo, b_hi = (3, -5, 7), (-2, 9, 1), 0x12345678, -0x0abcdef1
    try:
        ck.set_tree_slice(24)
        got = ck.tree_lut_bootstrap(pc, tv1, tuple(lo), tuple(hi), p_hi=8, theta=4, weights_lo=w_lo, bias_lo=b_lo, weights_hi=w_hi, bias_hi=b_hi, table_index=tab)
    finally:
        ck.set_tree_slice(65536)
    assert got.shape == (count, p.n + 1)
    assert np.array_equal(got, compose(ck, pc, tv1, lo, hi, 8, 4, w_lo=w_lo, b_lo=b_lo, w_hi=w_hi, b_hi=b_hi, table_index=tab))


def test_tree_131072_level1_jobs(sk128, ck, pack):
    # 8 192 samples x R = 16 (p = 16 digits, theta1 = 1, p_out = 8): 131 072 level-1 rotations in two slices of 65 536, 8 192 level-2 ones.
    # Decrypt-exact on all; the model on two samples (17 oracle rotations each, ~10 s per sample on one core)
    from thfhe import lut
    p, K, orc = sk128
    pc, pk = pack
    rng = np.random.default_rng(90)
    count = 8192
    F = rng.integers(0, 8, (16, 16))
    tv1 = lut.tree_test_vectors(lambda h, l: F[h, l], 16, 16, 8, theta=1)
    hi, lo = rng.integers(0, 16, count), rng.integers(0, 16, count)
    xh, xl = enc_int(K, hi, 16, 1900), enc_int(K, lo, 16, 1901)
    got = ck.tree_lut_bootstrap(pc, tv1, xl, xh, p_hi=16)
    assert np.array_equal(dec_int(K, got, 8), F[hi, lo])
    picks = [4095, 8191]     # the last sample of each slice
    assert np.array_equal(got[picks], np.stack(pmap(lambda g: model(orc, pk, p, tv1, [xl], [xh], g, 1, 16), picks)))
    err = PR.torus(PR.wrap32(K.phases(got).astype(np.int64) - lut.encode(F[hi, lo], 8)))
    print("tree p=16 theta1=1 p_out=8: std of phase(out) - encode(f) on 8192 samples", err.std(), "max", np.abs(err).max())


# ---- (d) error paths -------------------------------------------------------------------------------------------------------------------------

def test_error_paths_leave_both_contexts_usable(sk128, ck, pack):
    import thfhe
    from thfhe import keygen, lut
    from thfhe import threshold as T
    p, K, orc = sk128
    pc, pk = pack
    tv1 = lut.tree_test_vectors(lambda h, l: (h + l) % 4, 4, 4, 4)
    xh, xl = enc_int(K, [1, 2, 3], 4, 2000), enc_int(K, [3, 0, 2], 4, 2001)
    want = ck.tree_lut_bootstrap(pc, tv1, xl, xh, p_hi=4)
    assert np.array_equal(dec_int(K, want, 4), [0, 2, 1])
    bare = T.PolyContext(0)
    with pytest.raises(thfhe.ThfheError, match="error -1.*no packing key"):
        ck.tree_lut_bootstrap(bare, tv1, xl, xh, p_hi=4)
    rng = np.random.default_rng(5)
    bare.set_pack_key(keygen.gen_pack_key(rng, K.lwe_key[:10], K.rlwe_key[0], 8, 2, SIGMA_BK), 8, 2)
    with pytest.raises(thfhe.ThfheError, match="error -1.*dimension"):
        ck.tree_lut_bootstrap(bare, tv1, xl, xh, p_hi=4)
    with pytest.raises(thfhe.ThfheError, match="error -1.*multiple of p"):
        T.PackBoxes(bare, np.zeros((6, 11), np.int32), 4)
    with pytest.raises(thfhe.ThfheError, match="error -1.*power of two"):
        T.PackBoxes(bare, np.zeros((6, 11), np.int32), 3)
    assert T.PackBoxes(bare, np.zeros((0, 11), np.int32), 4)[0].shape == (0, N)
    bare.close()
    if thfhe.lib().thfhe_device_count() > 1:   # a packing context on another device
        other = T.PolyContext(1)
        other.set_pack_key(pk, p.ks_t, p.ks_basebit)
        with pytest.raises(thfhe.ThfheError, match="error -1.*same device"):
            ck.tree_lut_bootstrap(other, tv1, xl, xh, p_hi=4)
        other.close()
    spec, spec2 = thfhe.LutSpec(1, (C.c_int32 * 3)(1, 0, 0), 0, 1), thfhe.LutSpec(1, (C.c_int32 * 3)(1, 0, 0), 0, 2)
    spec4 = thfhe.LutSpec(1, (C.c_int32 * 3)(1, 0, 0), 0, 4)
    i32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    out = np.zeros((3, p.n + 1), np.int32)
    tree = thfhe.lib().thfhe_tree_lut_bootstrap
    args = lambda lo, hi, p_hi: (ck.h, pc.h, C.byref(lo), C.byref(hi), p_hi, i32(tv1), 1, None, i32(xl), None, None, i32(xh), None, None, i32(out), 3)
    assert tree(*args(spec, spec2, 4)) == -1 and b"spec_hi theta" in thfhe.lib().thfhe_last_error()
    assert tree(*args(spec4, spec, 2)) == -1 and b"divide" in thfhe.lib().thfhe_last_error()
    with pytest.raises(thfhe.ThfheError, match="error -1.*n_luts"):
        ck.lut_bootstrap_enc(np.zeros((0, N), np.int32), np.zeros((0, N), np.int32), xl)
    assert ck.tree_lut_bootstrap(pc, tv1, xl[:0], xh[:0], p_hi=4).shape == (0, p.n + 1)
    # both contexts still work, and give the same words
    assert np.array_equal(ck.tree_lut_bootstrap(pc, tv1, xl, xh, p_hi=4), want)
    a, b = T.PackBoxes(pc, xl[[0, 1]], 2)
    ra, rb = TR.pack_boxes(xl[[0, 1]], pk, p.ks_t, p.ks_basebit, 2)
    assert np.array_equal(a, ra) and np.array_equal(b, rb)
