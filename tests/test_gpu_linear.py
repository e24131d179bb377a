"""Encrypted dense layers on the single-key engine (pytest -m gpu): lwe_linear_kernel and the fused call
thfhe_linear_lut_bootstrap, every word against numpy (tests/linear_reference.py) and against the model composed from the CPU oracle.

  (1) tile edges: every (M, K) around the kernel's output and reduction tiles on a record with one partly filled lane block, with and without bias;
  (2) record widths: every shape of support.SHAPES and SK-128 (631 words: two full lane blocks and a remainder), the edge weights and words of
      test_linear_host.py in the first, last and block-boundary word positions;
  (3) grid bound: 65 538 outputs in one call, and more output tiles than one grid dimension holds;
  (4) fused = composed = model: l = 1, 3, 4, theta = 1, 2, 4, three tables, on the kernel cases of support.KERNELS, with and without key switch;
  (5) slices: the same output at every thfhe_set_linear_slice setting, and no table index surviving from one call to the next;
  (6) a two-layer network on real SK-128 ciphertexts: 7 fresh bits -> 3 threshold neurons -> majority.

(1) - (5) run on random words, not valid ciphertexts; the contract is word equality."""
import numpy as np
import pytest

import linear_reference as LR
import lut_reference as R
from support import KERNELS, N, SHAPES, dec_int, differing, enc_int, pmap, shape_env, shape_id, sk128_cloud_key, thresholds, words

pytestmark = pytest.mark.gpu

M4, K4, COUNT4 = 5, 4, 11
IDX4 = np.array([2, 0, 1, 1, 2], np.int32)   # every one of the three tables
FUSED_SHAPES = [SHAPES[0], SHAPES[2], SHAPES[3]]   # l = 1, 3, 4


@pytest.fixture(scope="module")
def env(O):
    yield from shape_env(O)


@pytest.fixture(scope="module")
def ck128(sk128):
    yield from sk128_cloud_key(sk128)


def tiles(ck):
    tm, tk = ck.linear_tile()
    Ms = [m for m in (1, tm - 1, tm, tm + 1, 2 * tm + 1) if m > 0]
    Ks = [k for k in (1, tk - 1, tk, tk + 1, 2 * tk + 3) if k > 0]
    return sorted(set(Ms)), sorted(set(Ks))


# ---- (1) tile edges -------------------------------------------------------------------------------------------------------------------------

def test_tile_edges(env):
    shape = SHAPES[2]
    assert shape[0] == 37
    p, K, orc, ck = env(shape)
    rec, count = p.n + 1, 3
    Ms, Ks = tiles(ck)
    rng = np.random.default_rng(2401)
    for M in Ms:
        for Kk in Ks:
            W = words(rng, M, Kk)
            x = words(rng, count, Kk, rec)
            b = words(rng, M)
            for bias in (None, b):
                got = ck.lwe_linear(W, x, bias)
                ref = LR.linear(W, x, bias)
                assert got.shape == (count, M, rec)
                assert np.array_equal(got, ref), (M, Kk, bias is not None, differing(got, ref))
            z = ck.lwe_linear(W, np.zeros_like(x), b)   # the bias lands on the body word only
            assert not z[:, :, :-1].any(), (M, Kk)
            assert np.array_equal(z[:, :, -1], np.broadcast_to(b, (count, M))), (M, Kk)


# ---- (2) record widths ------------------------------------------------------------------------------------------------------------------------

def edge_case(rec, seed):
    """M = 5, K = 7, count = 2: random words with the edge weights in W and the edge words at the first, last and block-boundary positions"""
    rng = np.random.default_rng(seed)
    M, Kk, count = 5, 7, 2
    W = words(rng, M, Kk)
    ew, ed = LR.EDGE_WEIGHTS, LR.EDGE_WORDS
    for m in range(M):
        for k in range(5):
            W[m, k] = np.int64(ew[(m + k) % 5]).astype(np.int32)   # every edge weight in every row, the last two columns stay random
    x = words(rng, count, Kk, rec)
    pos = sorted({q for q in (0, 1, rec - 2, rec - 1, 255, 256, 257, 511, 512, 513) if 0 <= q < rec})
    for s in range(count):
        for k in range(Kk):
            for j, q in enumerate(pos):
                x[s, k, q] = np.int64(ed[(s + k + j) % 4]).astype(np.int32)
    return W, x, words(rng, M), pos


def check_widths(ck, rec, seed):
    W, x, b, pos = edge_case(rec, seed)
    for bias in (None, b):
        got = ck.lwe_linear(W, x, bias)
        ref = LR.linear(W, x, bias)
        assert np.array_equal(got, ref), (rec, bias is not None, differing(got, ref))
    big = LR.linear_bigint(W, x[:, :, pos], None)   # the edge positions once more against unbounded integers
    assert np.array_equal(ck.lwe_linear(W, x)[:, :, pos], big), rec


@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_record_widths(env, shape):
    p, K, orc, ck = env(shape)
    check_widths(ck, p.n + 1, 2500 + shape[0])


def test_record_width_of_sk128(ck128):
    assert ck128.words == 631
    check_widths(ck128, 631, 2631)


# ---- (3) grid bound -----------------------------------------------------------------------------------------------------------------------------

def test_more_outputs_than_a_grid_dimension(env):
    p, K, orc, ck = env(SHAPES[3])
    assert p.n == 16
    rng = np.random.default_rng(2600)
    M, Kk, count = 3, 2, 21846
    assert count * M == 65538
    W, x, b = words(rng, M, Kk), words(rng, count, Kk, p.n + 1), words(rng, M)
    got = ck.lwe_linear(W, x, b)
    ref = LR.linear(W, x, b)
    assert np.array_equal(got, ref), differing(got, ref)


def test_more_output_tiles_than_a_grid_dimension(env):
    # one output tile per sample: 65 541 tiles on a grid whose second dimension stops at 65 535, so six workgroups take a second tile
    p, K, orc, ck = env(SHAPES[5])
    assert p.n == 1
    rng = np.random.default_rng(2601)
    M, Kk, count = 2, 3, 65541
    W, x, b = words(rng, M, Kk), words(rng, count, Kk, 2), words(rng, M)
    got = ck.lwe_linear(W, x, b)
    ref = LR.linear(W, x, b)
    assert np.array_equal(got, ref), differing(got, ref)


# ---- (4) fused = composed = model ---------------------------------------------------------------------------------------------------------------

_cache = {}


def fused_case(orc, shape, theta, idx=IDX4):
    """inputs and model outputs of one (shape, theta): the kernel cases and the slice test share them"""
    key = (shape, theta, None if idx is None else tuple(idx))
    if key not in _cache:
        rng = np.random.default_rng(2700 + 10 * SHAPES.index(shape) + theta)
        rec = shape[0] + 1
        W, x, b = words(rng, M4, K4), words(rng, COUNT4, K4, rec), words(rng, M4)
        tv = words(rng, 3, N)
        wo = LR.fused(R.lut_bootstrap, orc, W, x, b, tv, theta, idx, False, pmap)
        ks = np.stack(pmap(lambda u: orc.keyswitch(u), wo.reshape(-1, N + 1))).reshape(COUNT4, M4, theta, rec)
        _cache[key] = (W, x, b, tv, wo, ks)
    return _cache[key]


@pytest.mark.parametrize("kernel", KERNELS, ids=[k[0] for k in KERNELS])
@pytest.mark.parametrize("shape", FUSED_SHAPES, ids=shape_id)
def test_fused_equals_composed_equals_model(env, shape, kernel):
    p, K, orc, ck = env(shape)
    case, coop, ring4, name = kernel
    # the `split` pair cuts 7 .. 12 rotations into 6 on the four-wave ring and the rest cooperative: two samples (10 jobs) per slice put every
    # launch of the fused call there; the other cases run the 55 jobs in one launch
    per_launch = 2 * M4 if case == "split" else COUNT4 * M4
    try:
        ck.set_linear_slice(per_launch)
        with thresholds(ck, coop, ring4):
            assert ck.rotation_kernel_name(per_launch) == name.format(l=p.l)
            for theta in (1, 2, 4):
                W, x, b, tv, wo, ks = fused_case(orc, shape, theta)
                u = ck.linear_lut_bootstrap_wo_keyswitch(tv, W, x, b, theta=theta, lut_index=IDX4)
                assert u.shape == (COUNT4, M4, theta, N + 1)
                assert np.array_equal(u, wo), (theta, differing(u, wo))
                got = ck.linear_lut_bootstrap(tv, W, x, b, theta=theta, lut_index=IDX4)
                assert got.shape == (COUNT4, M4, theta, p.n + 1)
                assert np.array_equal(got, ks), (theta, differing(got, ks))
                # the two public calls in a row
                xs = ck.lwe_linear(W, x, b)
                flat_idx = np.tile(IDX4, COUNT4)
                two = ck.lut_bootstrap(tv, xs.reshape(-1, p.n + 1), theta=theta, lut_index=flat_idx).reshape(got.shape)
                assert np.array_equal(got, two), (theta, differing(got, two))
                two = ck.lut_bootstrap_wo_keyswitch(tv, xs.reshape(-1, p.n + 1), theta=theta, lut_index=flat_idx).reshape(u.shape)
                assert np.array_equal(u, two), (theta, differing(u, two))
    finally:
        ck.set_linear_slice(4096)


# ---- (5) slices -----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("theta", [1, 2, 4])
def test_slices_do_not_change_the_output(env, theta):
    shape = SHAPES[3]
    p, K, orc, ck = env(shape)
    W, x, b, tv, wo, ks = fused_case(orc, shape, theta)
    mt = M4 * theta
    other = np.array([0, 0, 2, 1, 0], np.int32)
    xs = LR.linear(W, x, b)
    try:
        for setting in (1, mt - 1, mt, 2 * mt + 1, M4 - 1, M4, 2 * M4 + 1, None):
            ck.set_linear_slice(4096 if setting is None else setting)
            assert np.array_equal(ck.lwe_linear(W, x, b), xs), setting
            got = ck.linear_lut_bootstrap(tv, W, x, b, theta=theta, lut_index=IDX4)
            assert np.array_equal(got, ks), (setting, differing(got, ks))
            u = ck.linear_lut_bootstrap_wo_keyswitch(tv, W, x, b, theta=theta, lut_index=IDX4)
            assert np.array_equal(u, wo), (setting, differing(u, wo))
            # a second call with another index, then one without: neither sees the indices of the call before
            for idx in (other, None):
                flat = None if idx is None else np.tile(idx, COUNT4)
                want = ck.lut_bootstrap(tv, xs.reshape(-1, p.n + 1), theta=theta, lut_index=flat).reshape(ks.shape)
                assert not np.array_equal(want, ks)
                got = ck.linear_lut_bootstrap(tv, W, x, b, theta=theta, lut_index=idx)
                assert np.array_equal(got, want), (setting, idx, differing(got, want))
    finally:
        ck.set_linear_slice(4096)


def test_second_index_against_the_model(env):
    # the call after another index, against the oracle-composed model (not only against the GPU's own two-call form)
    shape = SHAPES[3]
    p, K, orc, ck = env(shape)
    other = np.array([0, 0, 2, 1, 0], np.int32)
    W, x, b, tv, wo, ks = fused_case(orc, shape, 2)
    W2, x2, b2, tv2, wo2, ks2 = fused_case(orc, shape, 2, other)
    assert np.array_equal(W, W2) and np.array_equal(tv, tv2) and not np.array_equal(ks, ks2)
    assert np.array_equal(ck.linear_lut_bootstrap(tv, W, x, b, theta=2, lut_index=IDX4), ks)
    got = ck.linear_lut_bootstrap(tv, W, x, b, theta=2, lut_index=other)
    assert np.array_equal(got, ks2), differing(got, ks2)


def test_linear_last_timings(env):
    # the device events of the linear stage: refused before a profiled call, then upload and kernel inside upload start .. key-switch end, which
    # contains the PBS stages thfhe_last_timings reports for the same slice
    import thfhe
    shape = SHAPES[1]
    p, K, orc, ck = env(shape)
    rng = np.random.default_rng(2750)
    W, x, tv = words(rng, M4, K4), words(rng, COUNT4, K4, p.n + 1), words(rng, 1, N)
    ck.linear_lut_bootstrap(tv, W, x)
    with pytest.raises(thfhe.ThfheError, match="no profiled call"):
        ck.linear_last_timings()
    ck.set_profiling(True)
    try:
        ck.linear_lut_bootstrap(tv, W, x)
        t, pbs = ck.linear_last_timings(), ck.last_timings()
        assert t["upload_ms"] > 0 and t["linear_ms"] > 0
        assert t["total_ms"] >= t["upload_ms"] + t["linear_ms"] + pbs["total_ms"] - 5e-3
        ck.lwe_linear(W, x)
        t = ck.linear_last_timings()
        assert abs(t["total_ms"] - (t["upload_ms"] + t["linear_ms"])) < 5e-3   # no key switch: the kernel's end (5 us covers the float32 rounding of three event differences)
    finally:
        ck.set_profiling(False)


# ---- (6) a small network on real ciphertexts ------------------------------------------------------------------------------------------------------

def test_two_layer_network_on_sk128(sk128, ck128):
    """Layer 1: 7 fresh bits (sigma = 2^-15) encoded at p = 8, W1 in {0,1}^(3x7) (every sum <= 7 < p), table `sum >= threshold_m` emitted as a bit at
    p = 4.  Layer 2: the three outputs, weights (1, 1, 1) (sum <= 3 < 4), table = majority.  Margins, derived (DESIGN 4.24 has the measured sigma):
    layer 1 half-box 1/32 against the mod-switch sigma 2.5e-3 of section 4.7 (the fresh noise, sqrt(7) 2^-15 = 8.1e-5, is below it): 12 sigma;
    layer 2 half-box 1/16 against sqrt(3) times a bootstrapped record's noise (3.3e-3, the key switch's share included) joined with the same
    mod-switch term, 6.6e-3: 9 sigma (tools/linear_margins.py measures both on the CPU oracle)."""
    from thfhe import circuits, lut
    p, K, orc = sk128
    ck = ck128
    rng = np.random.default_rng(2800)
    S = 4
    bits = rng.integers(0, 2, (S, 7))
    bits[0], bits[1] = 0, 1                     # the all-zero sample (phase at the negacyclic wrap) and the all-one sample (sum 7, the top box)
    W1 = np.array([[1, 1, 1, 1, 1, 1, 1], [1, 1, 1, 1, 0, 0, 0], [1, 0, 1, 0, 1, 0, 1]], np.int32)
    thr = [4, 2, 2]
    W2 = np.array([[1, 1, 1]], np.int32)
    tv1 = np.stack([lut.test_vector(lut.int_outputs(lambda s, t=t: int(s >= t), 4, 8), 8) for t in thr])
    tv2 = lut.test_vector(lut.int_outputs(lambda s: int(s >= 2), 4, 4), 4)[None]
    idx = np.arange(3, dtype=np.int32)
    x = enc_int(K, bits.reshape(-1), 8, 2801).reshape(S, 7, p.n + 1)

    sums1 = circuits.dense_plain(W1, None, bits, 8)
    want1 = (sums1 >= np.array(thr)).astype(np.int64)
    sums2 = circuits.dense_plain(W2, None, want1, 4)
    want2 = (sums2 >= 2).astype(np.int64)
    assert sums1.max() < 8 and sums2.max() < 4 and len(set(want2.reshape(-1).tolist())) == 2   # both answers occur

    # the condition: the CPU reference alone decrypts every intermediate and final value to the plaintext network's
    ref_x1 = LR.linear(W1, x)
    assert np.array_equal(dec_int(K, ref_x1.reshape(-1, p.n + 1), 8).reshape(S, 3), sums1)
    ref1 = LR.fused(R.lut_bootstrap, orc, W1, x, None, tv1, 1, idx, True, pmap)          # 12 full-size rotations
    assert np.array_equal(dec_int(K, ref1.reshape(-1, p.n + 1), 4).reshape(S, 3), want1)
    h = ref1.reshape(S, 3, p.n + 1)
    ref_x2 = LR.linear(W2, h)
    assert np.array_equal(dec_int(K, ref_x2.reshape(-1, p.n + 1), 4).reshape(S, 1), sums2)
    ref2 = LR.fused(R.lut_bootstrap, orc, W2, h, None, tv2, 1, None, True, pmap)         # 4 more
    assert np.array_equal(dec_int(K, ref2.reshape(-1, p.n + 1), 4).reshape(S, 1), want2)

    # the GPU: word for word, and it decrypts to the plaintext network's answer
    got1 = ck.linear_lut_bootstrap(tv1, W1, x, lut_index=idx)
    assert np.array_equal(got1, ref1), differing(got1, ref1)
    got2 = ck.linear_lut_bootstrap(tv2, W2, got1.reshape(S, 3, p.n + 1))
    assert np.array_equal(got2, ref2), differing(got2, ref2)
    assert np.array_equal(dec_int(K, got2.reshape(-1, p.n + 1), 4).reshape(S, 1), want2)
