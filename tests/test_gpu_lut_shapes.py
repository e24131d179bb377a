"""The lookup-table bootstraps beyond SK-128 (pytest -m gpu; DESIGN.md sections 4.7 and 4.11): every decomposition length l = 1 .. 4 of
launch_rotations<kLut> and <kLutEnc> on the eight-wave ring, four-wave ring and cooperative kernels, every word of every job against the
model composed from the CPU oracle (lut_reference.py, tree_lut_reference.py).

  (1) a sweep of parameter shapes (n <= 64 keeps an oracle rotation at tens of milliseconds): random non-constant tables with a per-sample
      index, 1 .. 3 weighted inputs and a bias, theta = 1, 2, 4, on the four threshold pairs of support.KERNELS;
  (2) every rotation amount: records with an all-zero mask run no CMux, so the output is the extraction of X^{-barb} * table, which numpy
      gives without an oracle rotation -- every multiple of theta in Z_2N, the words next to the 2^32 wrap included, on each kernel shape;
  (3) zero-mask jobs interleaved with ordinary ones in the same workgroups (idle waves keep the ring's lock step).

The inputs are random words, not valid ciphertexts; the contract is word equality."""
import numpy as np
import pytest

import lut_reference as R
import oracle_lib as OL
import tree_lut_reference as TR
from support import KERNELS, N, SHAPES, differing, pmap, shape_env, shape_id, spread_index, thresholds, words

pytestmark = pytest.mark.gpu

KINDS = ["plain", "enc"]
# 11 jobs: the eight-wave ring's second workgroup holds 3, the four-wave ring's third holds 3, the split is 6 (4 + 2) + 5 cooperative
COUNT = 11


@pytest.fixture(scope="module")
def env(O):
    yield from shape_env(O)


def call(ck, kind, keyswitch, tabs, recs, **kw):
    if kind == "enc":
        return (ck.lut_bootstrap_enc if keyswitch else ck.lut_bootstrap_enc_wo_keyswitch)(tabs[0], tabs[1], *recs, **kw)
    return (ck.lut_bootstrap if keyswitch else ck.lut_bootstrap_wo_keyswitch)(tabs[1], *recs, **kw)


def model_wo(orc, kind, tabs, recs, weights, bias, idx, theta, g):
    """one job of the model, without the key switch: int32[theta][N+1]"""
    ins = [r[g] for r in recs]
    if kind == "enc":
        return TR.lut_enc(orc, ins, weights, bias, tabs[0][idx[g]], tabs[1][idx[g]], theta, keyswitch=False)
    return R.lut_bootstrap(orc, ins, weights, bias, tabs[1][idx[g]], theta, keyswitch=False)


def model(orc, kind, tabs, recs, weights, bias, idx, theta):
    """every job of the model: (int32[count][theta][N+1], int32[count][theta][n+1])"""
    wo = np.stack(pmap(lambda g: model_wo(orc, kind, tabs, recs, weights, bias, idx, theta, g), range(len(idx))))
    ks = np.stack(pmap(lambda u: orc.keyswitch(u), wo.reshape(-1, N + 1))).reshape(wo.shape[0], theta, -1)
    return wo, ks


_sweep_cache = {}


def sweep_case(orc, shape, kind, theta):
    """inputs and model outputs of one (shape, table kind, theta): the four kernel cases share them"""
    key = (shape, kind, theta)
    if key not in _sweep_cache:
        s = SHAPES.index(shape)
        rng = np.random.default_rng(100 * s + 10 * theta + KINDS.index(kind))
        n = shape[0]
        n_inputs = 1 + (s + theta.bit_length()) % 3            # 1 .. 3 inputs, every count at every theta over the shapes
        recs = [words(rng, COUNT, n + 1) for _ in range(n_inputs)]
        weights = tuple(int(w) for w in rng.choice([-7, -5, -3, -2, 2, 3, 5, 6, 7], n_inputs))
        bias = int(rng.integers(-2**31, 2**31))
        n_luts = 3 + s % 2
        tabs = (words(rng, n_luts, N), words(rng, n_luts, N))   # random words: (masks, bodies); the plaintext entry takes the bodies
        idx = spread_index(rng, COUNT, n_luts)
        assert not np.array_equal(idx[:5], idx[6:])             # the split's second launch must not pass on the first one's indices
        _sweep_cache[key] = (recs, weights, bias, tabs, idx) + model(orc, kind, tabs, recs, weights, bias, idx, theta)
    return _sweep_cache[key]


# ---- (1) shape sweep ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kernel", KERNELS, ids=[k[0] for k in KERNELS])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_every_word_on_every_shape(env, shape, kind, kernel):
    p, K, orc, ck = env(shape)
    _, coop, ring4, name = kernel
    with thresholds(ck, coop, ring4):
        assert ck.rotation_kernel_name(COUNT) == name.format(l=p.l)
        for theta in (1, 2, 4):
            recs, weights, bias, tabs, idx, wo, ks = sweep_case(orc, shape, kind, theta)
            kw = dict(weights=weights, bias=bias, theta=theta, lut_index=idx)
            u = call(ck, kind, False, tabs, recs, **kw)
            assert u.shape == (COUNT, theta, N + 1)
            assert np.array_equal(u, wo), (theta, differing(u, wo))
            got = call(ck, kind, True, tabs, recs, **kw)
            assert got.shape == (COUNT, theta, p.n + 1)
            assert np.array_equal(got, ks), (theta, differing(got, ks))


# ---- (2) every rotation amount --------------------------------------------------------------------------------------------------------------

AMOUNT_SHAPES = {1: (3, 1, 8, 8, 2), 2: (3, 2, 10, 8, 2), 3: (5, 3, 7, 8, 2), 4: (2, 4, 8, 5, 3)}   # by l; no CMux runs, n only sizes the (idle) key stream
CALL = 1001   # jobs per call: below one eight-wave round, so the thresholds alone choose the kernel; 1001 = 125 x 8 + 1 = 250 x 4 + 1


def amount_words(theta, rng):
    """body words whose theta-rounded mod-switch takes every multiple of theta in Z_2N, each at a random place inside its rounding interval,
    then the interval ends around 0 = 2^32 (the wrap), around 1/2 (barb = N = -N) and around theta itself"""
    step = (1 << 32) // (2 * N // theta)                        # one mod-switch step: 2^21 theta
    k = np.arange(2 * N // theta, dtype=np.int64)
    w = k * step + rng.integers(-(step // 2) + 1, step // 2, k.shape[0])
    edges = []
    for c in (0, 1 << 31, step, (1 << 32) - step):
        edges += [c, c - 1, c + 1, c - step // 2, c - step // 2 - 1, c + step // 2 - 1, c + step // 2]
    return R.to_i32(np.concatenate([w, np.array(edges, np.int64)]))


def rotation_only_reference(kind, tabs, idx, bar, theta):
    """extraction of X^{-bar} * table at coefficients 0 .. theta-1, per job: int32[jobs][theta][N+1]"""
    out = np.empty((len(bar), theta, N + 1), np.int32)
    for g, b in enumerate(bar):
        acc = np.zeros(2 * N, np.int32)
        if kind == "enc":
            acc[:N] = R.monomial(tabs[0][idx[g]], -int(b), N)
        acc[N:] = R.monomial(tabs[1][idx[g]], -int(b), N)
        for j in range(theta):
            out[g, j] = R.extract_at(acc, j, N)
    return out


@pytest.mark.parametrize("kernel", KERNELS[:3], ids=[k[0] for k in KERNELS[:3]])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("theta", [1, 2, 4])
@pytest.mark.parametrize("l", [1, 2, 3, 4])
def test_every_rotation_amount(env, l, theta, kind, kernel):
    shape = AMOUNT_SHAPES[l]
    p, K, orc, ck = env(shape)
    _, coop, ring4, name = kernel
    rng = np.random.default_rng(1000 * l + 10 * theta + KINDS.index(kind))
    body = amount_words(theta, rng)
    order = rng.permutation(len(body))                          # neighbouring jobs of a workgroup get unrelated amounts
    body = body[order]
    bar = np.array([OL.lib().oracle_modswitch(int(w), N // theta) * theta for w in body], np.int64)
    seen = set((bar % (2 * N)).tolist())
    assert seen == set(range(0, 2 * N, theta))                  # every amount, and nothing off the theta grid
    x = np.zeros((len(body), p.n + 1), np.int32)
    x[:, p.n] = body                                            # all-zero mask: every bara is 0, no CMux
    tabs = (words(rng, 3, N), words(rng, 3, N))
    idx = rng.integers(0, 3, len(body)).astype(np.int32)
    ref = rotation_only_reference(kind, tabs, idx, bar, theta)
    with thresholds(ck, coop, ring4):
        covered = set()
        for first in range(0, len(body), CALL):
            sl = slice(first, min(first + CALL, len(body)))
            count = sl.stop - sl.start
            assert count < 2048 and ck.rotation_kernel_name(count) == name.format(l=l)
            u = call(ck, kind, False, tabs, [x[sl]], theta=theta, lut_index=idx[sl])
            bad = np.argwhere(u != ref[sl])
            assert bad.size == 0, ("barb, output, word of the first mismatches", [(int(bar[first + g]), int(j), int(q)) for g, j, q in bad[:6]])
            covered |= set((bar[sl] % (2 * N)).tolist())
        assert covered == seen


@pytest.mark.parametrize("kind", KINDS)
def test_amounts_across_an_eight_wave_round_and_its_remainder(env, kind):
    # default thresholds, 2 048 + 300 jobs: one whole eight-wave round, then the cooperative kernel on the slice that starts at job 2 048
    # (launch_br's piece(): tables, amounts and outputs of the second launch are offsets into the same arrays)
    shape = AMOUNT_SHAPES[2]
    p, K, orc, ck = env(shape)
    rng = np.random.default_rng(4242 + KINDS.index(kind))
    count, theta = 2048 + 300, 2
    body = words(rng, count)
    bar = np.array([OL.lib().oracle_modswitch(int(w), N // theta) * theta for w in body], np.int64)
    x = np.zeros((count, p.n + 1), np.int32)
    x[:, p.n] = body
    tabs = (words(rng, 5, N), words(rng, 5, N))
    idx = rng.integers(0, 5, count).astype(np.int32)
    assert not np.array_equal(idx[:300], idx[2048:])
    assert ck.rotation_kernel_name(count) == "sk_blind_rotate_ring_kernel<2>"
    u = call(ck, kind, False, tabs, [x], theta=theta, lut_index=idx)
    ref = rotation_only_reference(kind, tabs, idx, bar, theta)
    bad = np.argwhere(u != ref)
    assert bad.size == 0, ("job, output, word", bad[:6].tolist())


# ---- (3) zero-mask jobs among ordinary ones -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kernel", KERNELS, ids=[k[0] for k in KERNELS])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[3]], ids=shape_id)
def test_zero_mask_jobs_between_ordinary_jobs(env, shape, kind, kernel):
    # 11 jobs again: jobs 0, 3, 4, 6, 9 have an all-zero mask (their waves stream the key and keep the barriers without working), jobs 1 and
    # 10 a mask that is zero except for its last word, job 7 one whose first half mod-switches to 0 -- in every workgroup of both ring shapes
    p, K, orc, ck = env(shape)
    _, coop, ring4, name = kernel
    rng = np.random.default_rng(500 + SHAPES.index(shape) + 10 * KINDS.index(kind))
    x = words(rng, COUNT, p.n + 1)
    x[[0, 3, 4, 6, 9], :p.n] = 0
    x[[1, 10], :p.n - 1] = 0
    x[7, :p.n // 2] = rng.integers(-(1 << 18), 1 << 18, p.n // 2)   # below half a step of every theta: bara = 0
    theta = 2
    weights, bias = (1,), int(rng.integers(-2**31, 2**31))
    tabs = (words(rng, 3, N), words(rng, 3, N))
    idx = spread_index(rng, COUNT, 3)
    key = ("mixed", shape, kind)
    if key not in _sweep_cache:
        _sweep_cache[key] = model(orc, kind, tabs, [x], weights, bias, idx, theta)
    wo, ks = _sweep_cache[key]
    with thresholds(ck, coop, ring4):
        assert ck.rotation_kernel_name(COUNT) == name.format(l=p.l)
        kw = dict(weights=weights, bias=bias, theta=theta, lut_index=idx)
        u = call(ck, kind, False, tabs, [x], **kw)
        assert np.array_equal(u, wo), differing(u, wo)
        got = call(ck, kind, True, tabs, [x], **kw)
        assert np.array_equal(got, ks), differing(got, ks)
