"""The k-output two-digit tree with a multi-value level 1 on the MI355X (pytest -m gpu): thfhe_tree_lut_bootstrap_mvk
word for word against the three public calls in a row (thfhe_mv_lut_bootstrap at q = k p_hi -> thfhe_pack_boxes -> thfhe_lut_bootstrap_enc with
every sample's `hi` operands repeated k times), against thfhe_tree_lut_bootstrap_mv at k = 1, and against the model composed from the CPU oracle
(tree_mvk_reference.py) on a sample of jobs.  The reduced key shapes and threshold pairs are those of support.py.

Word-for-word cases use random int32 taps and random-word base vectors and inputs.  The one decrypting case is inside DESIGN 4.13's supported
set: SK-128, bit-valued tables (p_out = 2) at p_hi = p_lo = 8, |c|_2 <= 3.4.

The CPU model run on that case's seeds decrypts 256 of 256 outputs (std 6.2e-3, largest error 2.0e-2 of the half-step 1.25e-1).  The test prints
the measured std of phase - encode next to the prediction and asserts nothing on it."""

import numpy as np
import pytest

import lut_reference as R
import support
import tree_mvk_reference as TK
from support import KERNELS, N, SIGMA, SIGMA_BK, shape_env, shape_id, sk128_cloud_key, sk128_pack, thresholds, words

pytestmark = pytest.mark.gpu

SHAPES = support.SHAPES[:4]   # (n, l, Bgbit, ks_t, ks_basebit) at l = 1 .. 4
CASES = [(2, 2, 1), (4, 8, 3), (8, 8, 4), (2, 64, 32), (64, 2, 1)]   # (p_hi, p_lo, k): smallest and largest q, q = 64 both ways, k = 1, k no power of two
COUNT = 11


@pytest.fixture(scope="module")
def ck(sk128):
    yield from sk128_cloud_key(sk128)


@pytest.fixture(scope="module")
def pack(sk128):
    yield from sk128_pack(sk128)


@pytest.fixture(scope="module")
def env(O):
    yield from shape_env(O, with_pack=True)


def compose(ck, pc, tv0, w, lo, hi, w_lo=(1,), b_lo=0, w_hi=(1,), b_hi=0, table_index=None):
    """the three public calls in a row: int32[count][k][n+1]"""
    from thfhe import threshold as T
    w = w if w.ndim == 4 else w[None]
    nt, k, p_hi, p_lo = w.shape
    cands = ck.mv_lut_bootstrap(w.reshape(nt, k * p_hi, p_lo), *lo, tv0=tv0, weights=w_lo, bias=b_lo, table_index=table_index)
    a, b = T.PackBoxes(pc, cands.reshape(-1, cands.shape[-1]), p_hi)
    assert len(a) == len(lo[0]) * k
    rep = [np.repeat(x, k, axis=0) for x in hi]
    return ck.lut_bootstrap_enc(a, b, *rep, weights=w_hi, bias=b_hi, lut_index=np.arange(len(a)))[:, 0].reshape(len(lo[0]), k, -1)


def random_case(rng, n, case, count=COUNT, n_lo=1, n_hi=1, n_tables=3):
    p_hi, p_lo, k = case
    tab = (np.arange(count) % n_tables).astype(np.int32)
    rng.shuffle(tab)
    pick = lambda m: tuple(int(v) for v in rng.choice([-7, -5, -3, 2, 3, 5, 9], m))
    return dict(tv0=words(rng, N), w=words(rng, n_tables, k, p_hi, p_lo), lo=[words(rng, count, n + 1) for _ in range(n_lo)],
                hi=[words(rng, count, n + 1) for _ in range(n_hi)], tab=tab, w_lo=pick(n_lo), w_hi=pick(n_hi),
                b_lo=int(rng.integers(-2**31, 2**31)), b_hi=int(rng.integers(-2**31, 2**31)))


def fused(ck, pc, c, sl=slice(None)):
    return ck.tree_lut_bootstrap_mvk(pc, c["w"], tuple(x[sl] for x in c["lo"]), tuple(x[sl] for x in c["hi"]), tv0=c["tv0"], weights_lo=c["w_lo"],
                                     bias_lo=c["b_lo"], weights_hi=c["w_hi"], bias_hi=c["b_hi"], table_index=c["tab"][sl])


def three_calls(ck, pc, c):
    return compose(ck, pc, c["tv0"], c["w"], c["lo"], c["hi"], c["w_lo"], c["b_lo"], c["w_hi"], c["b_hi"], c["tab"])


def model(orc, pk, p, c, g):
    return TK.tree_mvk(orc, pk, p.ks_t, p.ks_basebit, [x[g] for x in c["lo"]], c["w_lo"], c["b_lo"], [x[g] for x in c["hi"]], c["w_hi"], c["b_hi"],
                       c["tv0"], c["w"][c["tab"][g]])[0]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "phi%d-plo%d-k%d" % c)
def test_fused_equals_the_three_public_calls(sk128, ck, pack, case):
    # 11 samples, a per-sample index over 3 tables, random words everywhere, SK-128 at full size
    p, K, orc = sk128
    pc, pk = pack
    c = random_case(np.random.default_rng(5100 + CASES.index(case)), p.n, case)
    got = fused(ck, pc, c)
    assert got.shape == (COUNT, case[2], p.n + 1)
    ref = three_calls(ck, pc, c)
    assert np.array_equal(got, ref), np.argwhere(got != ref)[:6].tolist()
    if case == (4, 8, 3):   # one sample of the CPU model: the mid-size case (a q = 64 sample is 64 oracle key switches and as many packings)
        assert np.array_equal(got[7], model(orc, pk, p, c, 7))


def test_k1_equals_tree_lut_bootstrap_mv(sk128, ck, pack):
    p, K, orc = sk128
    pc, pk = pack
    c = random_case(np.random.default_rng(5200), p.n, (8, 16, 1), n_lo=2, n_hi=1)
    got = fused(ck, pc, c)
    old = ck.tree_lut_bootstrap_mv(pc, c["w"][:, 0], tuple(c["lo"]), tuple(c["hi"]), tv0=c["tv0"], weights_lo=c["w_lo"], bias_lo=c["b_lo"],
                                   weights_hi=c["w_hi"], bias_hi=c["b_hi"], table_index=c["tab"])
    assert np.array_equal(got[:, 0], old)


_shape_cache = {}


@pytest.mark.parametrize("kernel", KERNELS, ids=[k[0] for k in KERNELS])
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_every_decomposition_length_on_every_kernel(env, shape, kernel):
    # l = 1 .. 4 on the eight-wave ring, the four-wave ring, the cooperative kernel and the split: 11 level-1 and 33 selection rotations; the three
    # calls and two samples of the CPU model are computed once per shape under the default thresholds
    p, K, orc, ck, pc, pk = env(shape)
    _, coop, ring4, name = kernel
    if shape not in _shape_cache:
        c = random_case(np.random.default_rng(5300 + SHAPES.index(shape)), p.n, (4, 8, 3), n_lo=1 + SHAPES.index(shape) % 2, n_hi=1)
        ref = three_calls(ck, pc, c)
        for g in (0, 10):
            assert np.array_equal(ref[g], model(orc, pk, p, c, g)), g
        _shape_cache[shape] = (c, ref)
    c, ref = _shape_cache[shape]
    with thresholds(ck, coop, ring4):
        assert ck.rotation_kernel_name(COUNT) == name.format(l=p.l)
        got = fused(ck, pc, c)
    assert np.array_equal(got, ref), np.argwhere(got != ref)[:6].tolist()


def test_slices_and_weighted_three_operand_digits(sk128, ck, pack):
    # 13 samples, k p_hi = 12 candidates each, two weighted `lo` and one `hi` operand, then one `lo` and two `hi` (three together on the DAG, up to
    # three each here): whole, in slices of 3 samples (40 candidates: 3 + 3 + 3 + 3 + 1) and below k p_hi (one sample per slice)
    p, K, orc = sk128
    pc, pk = pack
    for seed, n_lo, n_hi in ((5400, 3, 3), (5401, 1, 2)):
        c = random_case(np.random.default_rng(seed), p.n, (4, 16, 3), count=13, n_lo=n_lo, n_hi=n_hi)
        whole = fused(ck, pc, c)
        try:
            ck.set_tree_slice(40)
            sliced = fused(ck, pc, c)
            ck.set_tree_slice(5)
            single = fused(ck, pc, c, slice(0, 3))
        finally:
            ck.set_tree_slice(65536)
        assert np.array_equal(sliced, whole) and np.array_equal(single, whole[:3])
        assert np.array_equal(whole, three_calls(ck, pc, c))


def sbox_case():
    """the decrypting case: a random 6-bit -> 4-bit table, all 64 (hi, lo) as p = 8 digits, bit j of the value in table j (p_out = 2)"""
    rng = np.random.default_rng(5500)
    table = rng.integers(0, 16, 64)
    hi, lo = np.repeat(np.arange(8), 8), np.tile(np.arange(8), 8)
    return table, hi, lo


def test_six_bits_to_four_bits_decrypt(sk128, ck, pack):
    # SK-128 at full size, 1 + 4 rotations per sample; the messages equal those of four thfhe_tree_lut_bootstrap calls (4 x (4 + 1) rotations)
    from thfhe import lut
    p, K, orc = sk128
    pc, pk = pack
    table, hi, lo = sbox_case()
    fs = [lambda h, l, j=j: (table[8 * h + l] >> j) & 1 for j in range(4)]
    tv0, w = lut.tree_mvk_factors(fs, 8, 8, 2)
    assert w.shape == (4, 8, 8)
    xh, xl = R.encrypt_words(K, lut.encode(hi, 8), SIGMA, 5501), R.encrypt_words(K, lut.encode(lo, 8), SIGMA, 5502)
    got = ck.tree_lut_bootstrap_mvk(pc, w, xl, xh, tv0=tv0)
    assert got.shape == (64, 4, p.n + 1)
    want = np.stack([(table >> j) & 1 for j in range(4)], axis=1)
    ph = K.phases(got.reshape(-1, p.n + 1)).reshape(64, 4)
    err = (ph.astype(np.int64) - lut.encode(want, 2).astype(np.int64) + 2**31) % 2**32 - 2**31
    c2 = np.sqrt((w.astype(float) ** 2).sum(-1)).max()
    s_br, s_ks = 2.5e-3, 2.8e-3
    print(f"\ntree_mvk (8, 8, k = 4), p_out = 2: std of phase - encode {np.std(err / 2.0**32):.3e} (largest {np.abs(err).max() / 2.0**32:.3e}, half-step "
          f"1.25e-01); |c|_2 up to {c2:.2f}: |c|_2 s_br (+) s_br (+) sqrt2 s_ks = {np.sqrt((c2 * s_br)**2 + s_br**2 + 2 * s_ks**2):.3e}")
    dec = lut.decode(ph, 2)
    assert np.array_equal(dec, want)
    for j in range(4):
        old = ck.tree_lut_bootstrap(pc, lut.tree_test_vectors(fs[j], 8, 8, 2, theta=2), xl, xh, p_hi=8, theta=2)
        assert np.array_equal(lut.decode(K.phases(old), 2), dec[:, j]), j


def test_error_paths_leave_both_contexts_usable(sk128, ck, pack):
    import thfhe
    from thfhe import keygen
    from thfhe import threshold as T
    p, K, orc = sk128
    pc, pk = pack
    c = random_case(np.random.default_rng(5600), p.n, (4, 4, 2), count=3, n_tables=1)
    want = fused(ck, pc, c)
    bare = T.PolyContext(0)
    with pytest.raises(thfhe.ThfheError, match="error -1.*no packing key"):
        fused(ck, bare, c)
    bare.set_pack_key(keygen.gen_pack_key(np.random.default_rng(5), K.lwe_key[:10], K.rlwe_key[0], 8, 2, SIGMA_BK), 8, 2)
    with pytest.raises(thfhe.ThfheError, match="error -1.*dimension"):
        fused(ck, bare, c)
    bare.close()
    with pytest.raises(thfhe.ThfheError, match="error -1.*table_index"):
        fused(ck, pc, dict(c, tab=np.array([0, 1, 0], np.int32)))
    with pytest.raises(thfhe.ThfheError, match="error -1.*k p_hi"):
        fused(ck, pc, dict(c, w=np.zeros((1, 17, 4, 4), np.int32)))
    assert fused(ck, pc, c, slice(0, 0)).shape == (0, 2, p.n + 1)
    assert np.array_equal(fused(ck, pc, c), want)
