"""Multi-value bootstrapping on every kernel shape (pytest -m gpu): launch_rotations<kLutMv> at every decomposition
length l = 1 .. 4 on the eight-wave ring, four-wave ring and cooperative kernels, every word of every job against the model composed from
the CPU oracle (mv_lut_reference.py).  The shapes and threshold pairs are those of support.py.

  (1) a sweep of parameter shapes: a random-word base vector, random int32 factors in three tables with a per-sample index, 1 .. 3 weighted
      inputs and a bias, at (p, q) = (2, 1), (16, 9), (64, 17), (8, 64): q off the eight waves of the cooperative kernel, q > 8, both limits
      of p and q.  The model's rotations do not depend on (p, q): one accumulator per job serves the four cases;
  (2) every rotation amount: records with an all-zero mask run no CMux, so the accumulator is (0, X^{-barb} tv0) and numpy alone gives the
      expected words -- every amount in Z_2N, the words next to the 2^32 wrap included; and, with helper-built factors, the same records
      against thfhe_lut_bootstrap_wo_keyswitch on the product test vectors, bit for bit;
  (3) zero-mask jobs interleaved with ordinary ones in the same workgroups;
  (4) one call cut at a set_tree_slice boundary.

The inputs are random words, not valid ciphertexts; the contract is word equality."""
import numpy as np
import pytest

import lut_reference as R
import mv_lut_reference as MV
import oracle_lib as OL
from support import KERNELS, N, SHAPES, differing, pmap, shape_env, shape_id, spread_index, thresholds, words

pytestmark = pytest.mark.gpu

PQ = [(2, 1), (16, 9), (64, 17), (8, 64)]
N_TABLES = 3
# 11 jobs: the eight-wave ring's second workgroup holds 3, the four-wave ring's third holds 3, the split is 6 (4 + 2) + 5 cooperative
COUNT = 11


@pytest.fixture(scope="module")
def env(O):
    yield from shape_env(O)


def outputs_of(orc, accs, factors, idx):
    """the model's records of every job from its accumulator: (int32[count][q][N+1], int32[count][q][n+1])"""
    wo = np.stack([MV.combine(acc, factors[t], N) for acc, t in zip(accs, idx)])
    ks = np.stack(pmap(orc.keyswitch, wo.reshape(-1, N + 1))).reshape(wo.shape[0], wo.shape[1], -1)
    return wo, ks


_cache = {}


def sweep_inputs(orc, shape):
    """inputs and model accumulators of one shape: the (p, q) cases and the four kernel cases share them"""
    if shape not in _cache:
        s = SHAPES.index(shape)
        rng = np.random.default_rng(7100 + s)
        n = shape[0]
        n_inputs = 1 + s % 3
        recs = [words(rng, COUNT, n + 1) for _ in range(n_inputs)]
        weights = tuple(int(w) for w in rng.choice([-7, -5, -3, -2, 2, 3, 5, 6, 7], n_inputs))
        bias = int(rng.integers(-2**31, 2**31))
        tv0 = words(rng, N)
        idx = spread_index(rng, COUNT, N_TABLES)
        assert not np.array_equal(idx[:5], idx[6:])             # the split's second launch must not pass on the first one's indices
        factors = {pq: words(rng, N_TABLES, pq[1], pq[0]) for pq in PQ}
        accs = pmap(lambda g: MV.rotate(orc, R.prologue([r[g] for r in recs], weights, bias), tv0), range(COUNT))
        _cache[shape] = (recs, weights, bias, tv0, idx, factors, accs, {})
    return _cache[shape]


def sweep_case(orc, shape, pq):
    recs, weights, bias, tv0, idx, factors, accs, outs = sweep_inputs(orc, shape)
    if pq not in outs:
        outs[pq] = outputs_of(orc, accs, factors[pq], idx)
    return (recs, weights, bias, tv0, idx, factors[pq]) + outs[pq]


# ---- (1) shape sweep ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kernel", KERNELS, ids=[k[0] for k in KERNELS])
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_every_word_on_every_shape(env, shape, kernel):
    p, K, orc, ck = env(shape)
    _, coop, ring4, name = kernel
    with thresholds(ck, coop, ring4):
        assert ck.rotation_kernel_name(COUNT) == name.format(l=p.l)
        for pq in PQ:
            recs, weights, bias, tv0, idx, w, wo, ks = sweep_case(orc, shape, pq)
            kw = dict(tv0=tv0, weights=weights, bias=bias, table_index=idx)
            u = ck.mv_lut_bootstrap_wo_keyswitch(w, *recs, **kw)
            assert u.shape == (COUNT, pq[1], N + 1)
            assert np.array_equal(u, wo), (pq, differing(u, wo))
            got = ck.mv_lut_bootstrap(w, *recs, **kw)
            assert got.shape == (COUNT, pq[1], p.n + 1)
            assert np.array_equal(got, ks), (pq, differing(got, ks))


def test_no_index_is_table_zero(env):
    shape = SHAPES[2]
    p, K, orc, ck = env(shape)
    recs, weights, bias, tv0, idx, w, wo, ks = sweep_case(orc, shape, (16, 9))
    kw = dict(tv0=tv0, weights=weights, bias=bias)
    got = ck.mv_lut_bootstrap(w, *recs, **kw)
    assert np.array_equal(got, ck.mv_lut_bootstrap(w[:1], *recs, **kw))
    zero = np.flatnonzero(idx == 0)
    assert len(zero) and np.array_equal(got[zero], ks[zero])
    assert not np.array_equal(got[idx != 0], ks[idx != 0])


# ---- (2) every rotation amount ------------------------------------------------------------------------------------------------------------

AMOUNT_SHAPES = {1: (3, 1, 8, 8, 2), 2: (3, 2, 10, 8, 2), 3: (5, 3, 7, 8, 2), 4: (2, 4, 8, 5, 3)}   # by l; no CMux runs, n only sizes the (idle) key stream
AMOUNT_PQ = {1: (2, 1), 2: (16, 9), 3: (64, 17), 4: (8, 10)}   # by l: the sweep's cases, the 64 outputs cut to 10 (1 001 jobs x 64 records are 263 MB a call)
CALL = 1001   # jobs per call: below one eight-wave round, so the thresholds alone choose the kernel; 1001 = 125 x 8 + 1 = 250 x 4 + 1


def amount_words(rng):
    """body words whose mod-switch takes every value of Z_2N, each at a random place inside its rounding interval, then the interval ends
    around 0 = 2^32 (the wrap), around 1/2 (barb = N = -N) and around +-1"""
    step = (1 << 32) // (2 * N)
    k = np.arange(2 * N, dtype=np.int64)
    w = k * step + rng.integers(-(step // 2) + 1, step // 2, k.shape[0])
    edges = []
    for c in (0, 1 << 31, step, (1 << 32) - step):
        edges += [c, c - 1, c + 1, c - step // 2, c - step // 2 - 1, c + step // 2 - 1, c + step // 2]
    return R.to_i32(np.concatenate([w, np.array(edges, np.int64)]))


def zero_mask_records(n, body):
    x = np.zeros((len(body), n + 1), np.int32)
    x[:, n] = body                                              # all-zero mask: every bara is 0, no CMux
    return x


def rotation_only_reference(tv0, factors, idx, bar):
    """the records of the accumulators (0, X^{-bar} tv0), per job: int32[jobs][q][N+1]; the mask words are zero, the body is the p-tap sum"""
    q, p = factors.shape[1:]
    box = N // p
    J = N - box // 2 - box * np.arange(p)
    out = np.zeros((len(bar), q, N + 1), np.int32)
    for g, b in enumerate(bar):
        taps = R.monomial(tv0, -int(b), N)[J]
        out[g, :, N] = MV._low32(np.uint64(0) - MV._u64(factors[idx[g]]) @ MV._u64(taps))
    return out


@pytest.mark.parametrize("kernel", KERNELS[:3], ids=[k[0] for k in KERNELS[:3]])
@pytest.mark.parametrize("l", [1, 2, 3, 4])
def test_every_rotation_amount(env, l, kernel):
    shape = AMOUNT_SHAPES[l]
    p, K, orc, ck = env(shape)
    _, coop, ring4, name = kernel
    rng = np.random.default_rng(9000 + l)
    body = amount_words(rng)
    body = body[rng.permutation(len(body))]                     # neighbouring jobs of a workgroup get unrelated amounts
    bar = np.array([OL.lib().oracle_modswitch(int(w), N) for w in body], np.int64)
    seen = set((bar % (2 * N)).tolist())
    assert seen == set(range(2 * N))
    x = zero_mask_records(p.n, body)
    pt, q = AMOUNT_PQ[l]
    tv0, w = words(rng, N), words(rng, N_TABLES, q, pt)
    idx = rng.integers(0, N_TABLES, len(body)).astype(np.int32)
    ref = rotation_only_reference(tv0, w, idx, bar)
    with thresholds(ck, coop, ring4):
        for first in range(0, len(body), CALL):
            sl = slice(first, min(first + CALL, len(body)))
            count = sl.stop - sl.start
            assert count < 2048 and ck.rotation_kernel_name(count) == name.format(l=l)
            u = ck.mv_lut_bootstrap_wo_keyswitch(w, x[sl], tv0=tv0, table_index=idx[sl])
            bad = np.argwhere(u != ref[sl])
            assert bad.size == 0, ("barb, output, word of the first mismatches", [(int(bar[first + g]), int(j), int(k)) for g, j, k in bad[:6]])


def test_amounts_across_an_eight_wave_round_and_its_remainder(env):
    # default thresholds, 2 048 + 300 jobs: one whole eight-wave round, then the cooperative kernel on the slice that starts at job 2 048
    # (launch_br's piece(): amounts, table indices and the q records per job of the second launch are offsets into the same arrays)
    shape = AMOUNT_SHAPES[2]
    p, K, orc, ck = env(shape)
    rng = np.random.default_rng(4343)
    count, pt, q = 2048 + 300, 4, 3
    body = words(rng, count)
    bar = np.array([OL.lib().oracle_modswitch(int(w), N) for w in body], np.int64)
    tv0, w = words(rng, N), words(rng, 5, q, pt)
    idx = rng.integers(0, 5, count).astype(np.int32)
    assert not np.array_equal(idx[:300], idx[2048:])
    assert ck.rotation_kernel_name(count) == "sk_blind_rotate_ring_kernel<2>"
    u = ck.mv_lut_bootstrap_wo_keyswitch(w, zero_mask_records(p.n, body), tv0=tv0, table_index=idx)
    bad = np.argwhere(u != rotation_only_reference(tv0, w, idx, bar))
    assert bad.size == 0, ("job, output, word", bad[:6].tolist())


@pytest.mark.parametrize("kernel", KERNELS[:3], ids=[k[0] for k in KERNELS[:3]])
def test_helper_factors_equal_the_product_test_vectors(env, kernel):
    # the cross-check against an existing entry: with mv_base / mv_factors, output j of a rotation without CMuxes is, bit for bit, what
    # thfhe_lut_bootstrap_wo_keyswitch extracts from test_vector(f_j * step) rotated by the same amount
    from thfhe import lut
    shape = AMOUNT_SHAPES[3]
    p, K, orc, ck = env(shape)
    _, coop, ring4, name = kernel
    rng = np.random.default_rng(515)
    x = zero_mask_records(p.n, amount_words(rng)[::7])
    with thresholds(ck, coop, ring4):
        for pt, q, step in ((8, 5, 1 << 28), (64, 3, 1 << 25), (2, 2, 0x1234568)):
            f = rng.integers(-9, 10, (q, pt))
            u = ck.mv_lut_bootstrap_wo_keyswitch(lut.mv_factors(f, pt), x, tv0=lut.mv_base(step))
            for j in range(q):
                want = ck.lut_bootstrap_wo_keyswitch(lut.test_vector(R.to_i32(f[j] * step), pt), x)
                assert np.array_equal(u[:, j], want[:, 0]), (pt, j)


# ---- (3) zero-mask jobs among ordinary ones -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kernel", KERNELS, ids=[k[0] for k in KERNELS])
@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[3]], ids=shape_id)
def test_zero_mask_jobs_between_ordinary_jobs(env, shape, kernel):
    # jobs 0, 3, 4, 6, 9 have an all-zero mask (their waves stream the key and keep the barriers without working), jobs 1 and 10 a mask that
    # is zero except for its last word, job 7 one whose first half mod-switches to 0 -- in every workgroup of both ring shapes
    p, K, orc, ck = env(shape)
    _, coop, ring4, name = kernel
    rng = np.random.default_rng(600 + SHAPES.index(shape))
    x = words(rng, COUNT, p.n + 1)
    x[[0, 3, 4, 6, 9], :p.n] = 0
    x[[1, 10], :p.n - 1] = 0
    x[7, :p.n // 2] = rng.integers(-(1 << 18), 1 << 18, p.n // 2)   # below half a mod-switch step: bara = 0
    bias = int(rng.integers(-2**31, 2**31))
    tv0, w = words(rng, N), words(rng, N_TABLES, 9, 16)
    idx = spread_index(rng, COUNT, N_TABLES)
    key = ("mixed", shape)
    if key not in _cache:
        accs = pmap(lambda g: MV.rotate(orc, R.prologue([x[g]], (1,), bias), tv0), range(COUNT))
        _cache[key] = outputs_of(orc, accs, w, idx)
    wo, ks = _cache[key]
    with thresholds(ck, coop, ring4):
        assert ck.rotation_kernel_name(COUNT) == name.format(l=p.l)
        kw = dict(tv0=tv0, bias=bias, table_index=idx)
        u = ck.mv_lut_bootstrap_wo_keyswitch(w, x, **kw)
        assert np.array_equal(u, wo), differing(u, wo)
        got = ck.mv_lut_bootstrap(w, x, **kw)
        assert np.array_equal(got, ks), differing(got, ks)


# ---- (4) slices ---------------------------------------------------------------------------------------------------------------------------

def test_a_call_across_a_slice_boundary(env):
    # 11 samples of 9 records in slices of at most 40 records: 4 + 4 + 3 samples, each slice with its own inputs, table indices and outputs
    shape = SHAPES[0]
    p, K, orc, ck = env(shape)
    recs, weights, bias, tv0, idx, w, wo, ks = sweep_case(orc, shape, (16, 9))
    kw = dict(tv0=tv0, weights=weights, bias=bias, table_index=idx)
    try:
        ck.set_tree_slice(40)
        u = ck.mv_lut_bootstrap_wo_keyswitch(w, *recs, **kw)
        got = ck.mv_lut_bootstrap(w, *recs, **kw)
    finally:
        ck.set_tree_slice(65536)
    assert np.array_equal(u, wo), differing(u, wo)
    assert np.array_equal(got, ks), differing(got, ks)
    assert len(ck.mv_lut_bootstrap(w, *[r[:0] for r in recs], tv0=tv0, weights=weights, bias=bias)) == 0   # count 0
