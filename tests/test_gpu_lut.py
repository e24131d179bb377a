"""Programmable bootstrapping on the MI355X (pytest -m gpu): thfhe_lut_bootstrap(_wo_keyswitch) against thfhe_bootstrap with a constant
test vector, bit for bit against the reference composed from the CPU oracle's pieces (tests/lut_reference.py) on every kernel shape, and
function values that decrypt correctly -- single LUTs, a bivariate table, chains, a many-LUT ripple adder and a 5 096-sample batch."""
import ctypes as C

import numpy as np
import pytest

import lut_reference as R
from support import SIGMA, dec_int, enc_int, sk128_cloud_key, thresholds, words

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ck(sk128):
    yield from sk128_cloud_key(sk128)


def test_constant_test_vector_is_the_gate_bootstrap(sk128, ck):
    p, K, orc = sk128
    x = K.encrypt_bits([0, 1, 1, 0, 1, 0, 0, 1, 1], SIGMA, 101)
    for mu in (1 << 29, 1 << 28):
        tv = np.full(p.N, mu, np.int32)
        u = ck.lut_bootstrap_wo_keyswitch(tv, x)
        assert u.shape == (len(x), 1, p.N + 1)
        assert np.array_equal(u[:, 0], ck.bootstrap_wo_keyswitch(x, mu))
        got = ck.lut_bootstrap(tv, x)
        assert got.shape == (len(x), 1, p.n + 1)
        assert np.array_equal(got[:, 0], ck.bootstrap(x, mu))


def _random_case(K, rng, count, n_inputs, seed):
    recs = [R.encrypt_words(K, rng.integers(-2**31, 2**31, count), SIGMA, seed + q) for q in range(n_inputs)]
    weights = tuple(int(w) for w in rng.integers(-7, 8, n_inputs))
    bias = int(rng.integers(-2**31, 2**31))
    return recs, weights, bias


def _reference(orc, recs, weights, bias, tvs, idx, theta, picks):
    wo = np.stack([R.lut_bootstrap(orc, [r[g] for r in recs], weights, bias, tvs[idx[g]], theta, keyswitch=False) for g in picks])
    ks = np.stack([np.stack([orc.keyswitch(u) for u in s]) for s in wo])
    return wo, ks


@pytest.mark.parametrize("theta,n_inputs", [(1, 1), (2, 2), (4, 3), (1, 3), (4, 1)])
def test_bit_exact_against_the_composed_oracle(sk128, ck, theta, n_inputs):
    # random tables (3 LUTs, random per-sample index), non-trivial weights and bias: the _wo_keyswitch records and the key-switched ones word for word
    p, K, orc = sk128
    rng = np.random.default_rng(10 * theta + n_inputs)
    count = 12
    recs, weights, bias = _random_case(K, rng, count, n_inputs, 200 + 10 * theta + n_inputs)
    tvs = words(rng, 3, p.N)
    idx = rng.integers(0, 3, count).astype(np.int32)
    kw = dict(weights=weights, bias=bias, theta=theta, lut_index=idx)
    u = ck.lut_bootstrap_wo_keyswitch(tvs, *recs, **kw)
    got = ck.lut_bootstrap(tvs, *recs, **kw)
    assert u.shape == (count, theta, p.N + 1) and got.shape == (count, theta, p.n + 1)
    wo, ks = _reference(orc, recs, weights, bias, tvs, idx, theta, range(count))
    assert np.array_equal(u, wo)
    assert np.array_equal(got, ks)


def test_every_blind_rotate_kernel_shape(sk128, ck):
    # the threshold pairs of test_gpu_parity.py::test_every_blind_rotate_kernel_bit_exact: eight-wave ring, four-wave ring, cooperative, and
    # 6 four-wave + 6 cooperative; 12 samples leave every workgroup partially filled
    p, K, orc = sk128
    rng = np.random.default_rng(7)
    recs, weights, bias = _random_case(K, rng, 12, 2, 300)
    tvs = words(rng, 3, p.N)
    idx = rng.integers(0, 3, 12).astype(np.int32)
    for theta in (1, 4):
        kw = dict(weights=weights, bias=bias, theta=theta, lut_index=idx)
        wo, ks = _reference(orc, recs, weights, bias, tvs, idx, theta, range(12))
        for coop, ring4 in ((0, 0), (0, 1024), (1 << 20, 1024), (5, 6)):
            with thresholds(ck, coop, ring4):
                assert np.array_equal(ck.lut_bootstrap_wo_keyswitch(tvs, *recs, **kw), wo), (theta, coop, ring4)
                assert np.array_equal(ck.lut_bootstrap(tvs, *recs, **kw), ks), (theta, coop, ring4)


@pytest.mark.parametrize("p_msg", [2, 4, 8])
def test_function_values_decrypt(sk128, ck, p_msg):
    from thfhe import lut
    p, K, orc = sk128
    rng = np.random.default_rng(p_msg)
    f = rng.integers(0, p_msg, p_msg)
    tv = lut.test_vector(lut.int_outputs(lambda m: f[m], p_msg), p_msg)
    m = np.repeat(np.arange(p_msg), 6)
    got = ck.lut_bootstrap(tv, enc_int(K, m, p_msg, 400 + p_msg))
    assert np.array_equal(dec_int(K, got[:, 0], p_msg), f[m])


def test_bivariate_table(sk128, ck):
    # f(a, b) on two 2-bit inputs through w = (4, 1) at p = 16: one rotation
    from thfhe import lut
    p, K, orc = sk128
    a, b = np.repeat(np.arange(4), 4), np.tile(np.arange(4), 4)
    f = lambda m: (m >> 2) * (m & 3) + 1                      # a*b + 1 in [1, 10]
    tv = lut.test_vector(lut.int_outputs(f, 16), 16)
    got = ck.lut_bootstrap(tv, enc_int(K, a, 16, 500), enc_int(K, b, 16, 501), weights=(4, 1))
    assert np.array_equal(dec_int(K, got[:, 0], 16), a * b + 1)


def test_bootstrapped_inputs_chain(sk128, ck):
    # three LUTs in a row at p = 4, each fed the key-switched output of the one before
    from thfhe import lut
    p, K, orc = sk128
    fs = [lambda m: (m + 1) % 4, lambda m: 3 - m, lambda m: (2 * m + 1) % 4]
    m = np.repeat(np.arange(4), 4)
    x, want = enc_int(K, m, 4, 600), m.copy()
    for f in fs:
        x = ck.lut_bootstrap(lut.test_vector(lut.int_outputs(f, 4), 4), x)[:, 0]
        want = np.array([f(v) for v in want])
        assert np.array_equal(dec_int(K, x, 4), want)


def test_many_lut_ripple_adder(sk128, ck):
    # a + b on 64 pairs of 8-bit integers: bit i is ONE theta = 2 rotation of a_i + b_i + c_i at p = 4 with sum = parity, carry = majority
    # (the boolean ripple adder of conftest.full_adder spends 5 bootstraps per bit)
    from thfhe import lut
    p, K, orc = sk128
    rng = np.random.default_rng(64)
    A, B = rng.integers(0, 256, 64), rng.integers(0, 256, 64)
    tv = lut.test_vector([lut.int_outputs(lambda m: m & 1, 4), lut.int_outputs(lambda m: m >= 2, 4)], 4, theta=2)
    rotations = 0
    carry, sums = None, []
    for i in range(8):
        ai, bi = enc_int(K, (A >> i) & 1, 4, 700 + 2 * i), enc_int(K, (B >> i) & 1, 4, 701 + 2 * i)
        if carry is None:
            out = ck.lut_bootstrap(tv, ai, bi, weights=(1, 1), theta=2)
        else:
            out = ck.lut_bootstrap(tv, ai, bi, carry, weights=(1, 1, 1), theta=2)
        rotations += 1
        sums.append(out[:, 0])
        carry = out[:, 1]
    assert rotations == 8   # per addition (the 64 additions share each launch)
    bits = np.stack([dec_int(K, s, 4) for s in sums] + [dec_int(K, carry, 4)])
    assert np.all(bits <= 1)
    total = sum(bits[i].astype(np.int64) << i for i in range(9))
    assert np.array_equal(total, A + B)
    assert np.array_equal(bits[8], (A + B) >> 8)


def test_large_batch(sk128, ck):
    # 4096 + 1000 samples: two whole eight-wave rounds plus a four-wave remainder
    from thfhe import lut
    p, K, orc = sk128
    rng = np.random.default_rng(5096)
    count = 4096 + 1000
    fs = rng.integers(0, 4, (3, 4))
    tvs = np.stack([lut.test_vector(lut.int_outputs(lambda m, f=f: f[m], 4), 4) for f in fs])
    idx = rng.integers(0, 3, count).astype(np.int32)
    m = rng.integers(0, 4, count)
    x = enc_int(K, m, 4, 800)
    u = ck.lut_bootstrap_wo_keyswitch(tvs, x, lut_index=idx)
    got = ck.lut_bootstrap(tvs, x, lut_index=idx)
    assert np.array_equal(dec_int(K, got[:, 0], 4), fs[idx, m])
    picks = np.sort(rng.choice(count, 8, replace=False))
    wo, ks = _reference(orc, [x], (1,), 0, tvs, idx, 1, picks)
    assert np.array_equal(u[picks], wo)
    assert np.array_equal(got[picks], ks)


def test_invalid_calls_are_refused_and_the_context_stays_usable(sk128, ck):
    import thfhe
    from thfhe import lut
    p, K, orc = sk128
    x = enc_int(K, [1, 2], 4, 900)
    tvs = np.stack([lut.test_vector(lut.int_outputs(lambda m: m, 4), 4)] * 2)
    with pytest.raises(thfhe.ThfheError, match="error -1.*lut_index"):
        ck.lut_bootstrap(tvs, x, lut_index=[0, 2])
    with pytest.raises(thfhe.ThfheError, match="error -1.*n_luts"):
        ck.lut_bootstrap(np.zeros((0, p.N), np.int32), x)
    with pytest.raises(thfhe.ThfheError, match="error -1.*theta"):
        ck.lut_bootstrap(tvs, x, theta=3)
    spec = thfhe.LutSpec(4, (C.c_int32 * 3)(1, 1, 1), 0, 1)
    out = np.zeros((2, 1, p.n + 1), np.int32)
    i32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    rc = thfhe.lib().thfhe_lut_bootstrap(ck.h, C.byref(spec), i32(tvs), 2, None, i32(x), i32(x), i32(x), i32(out), 2)
    assert rc == -1 and b"n_inputs" in thfhe.lib().thfhe_last_error()
    assert ck.lut_bootstrap(tvs, x[:0]).shape == (0, 1, p.n + 1)
    got = ck.lut_bootstrap(tvs, x, lut_index=[1, 0])
    assert np.array_equal(dec_int(K, got[:, 0], 4), [1, 2])
    assert np.array_equal(got[:, 0], ck.lut_bootstrap(tvs[:1], x)[:, 0])
