"""Multi-key programmable bootstrapping on the MI355X (pytest -m gpu): thfhe_mk_lut_bootstrap(_wo_keyswitch) against thfhe_mk_bootstrap with a
constant test vector, bit for bit against the reference composed from the CPU oracle's pieces (tests/mk_lut_reference.py) on every rotation shape
of the 3-gen engine, and function values that decrypt correctly -- single LUTs, a bivariate table, a chain and a many-LUT ripple adder."""
import numpy as np
import pytest

import mk_lut_reference as R

pytestmark = pytest.mark.gpu


def _keys(O, name, seed, **over):
    import thfhe
    p = O.make_params(name, **over)
    s = O.SIGMAS[name]
    K = O.MKKeys(p, seed, s["bk"], s["ks"])
    ck = thfhe.MKCloudKey(thfhe.make_params(**p.as_dict()), K.bk, K.ksk, device=0)
    return p, K, ck


@pytest.fixture(scope="module")
def mk2(O):
    p, K, ck = _keys(O, "MK2", 0x5EED0002)
    yield p, K, ck
    ck.close()


def enc_int(O, K, name, m, p_msg, seed):
    from thfhe import lut
    return R.encrypt_words(K, lut.encode(np.asarray(m), p_msg), O.SIGMAS[name]["lwe"], seed)


def dec_int(K, recs, p_msg):
    from thfhe import lut
    return lut.decode(K.phases(recs), p_msg)


def _check_exact(O, name, p, K, ck, theta, n_inputs, count, seed, picks=None):
    """Random tables (three LUTs, random lut_index), weights and bias: both outputs word for word against the composed reference."""
    orc = O.MKOracle(p, K.bk, K.ksk)
    rng = np.random.default_rng(seed)
    recs = [R.encrypt_words(K, rng.integers(-2**31, 2**31, count), O.SIGMAS[name]["lwe"], seed + q) for q in range(n_inputs)]
    recs[0][0, 1] = 0   # a zero mask word on the first sample (with weight != 0 on the others it may stay non-zero: both cases occur)
    weights = tuple(int(w) for w in rng.integers(-7, 8, n_inputs))
    bias = int(rng.integers(-2**31, 2**31))
    tvs = rng.integers(-2**63, 2**63, (3, p.N), dtype=np.int64)
    idx = rng.integers(0, 3, count).astype(np.int32)
    wo = ck.lut_bootstrap_wo_keyswitch(tvs, *recs, weights=weights, bias=bias, theta=theta, lut_index=idx)
    ks = ck.lut_bootstrap(tvs, *recs, weights=weights, bias=bias, theta=theta, lut_index=idx)
    assert wo.shape == (count, theta, p.N + 1) and ks.shape == (count, theta, p.parties * p.n + 1)
    for g in (range(count) if picks is None else picks):
        ref = R.lut_bootstrap(orc, [r[g] for r in recs], weights, bias, tvs[idx[g]], theta, keyswitch=False)
        assert np.array_equal(wo[g], ref), (name, theta, n_inputs, g)
        assert np.array_equal(ks[g], np.stack([orc.keyswitch(u) for u in ref])), (name, theta, n_inputs, g)


def test_constant_test_vector_is_the_mk_bootstrap(O, mk2):
    p, K, ck = mk2
    x = K.encrypt_bits([0, 1, 1, 0, 1, 0, 0, 1, 1], O.SIGMAS["MK2"]["lwe"], 101)
    for mu in (1 << 61, 1 << 60):
        tv = np.full(p.N, mu, np.int64)
        u = ck.lut_bootstrap_wo_keyswitch(tv, x)
        assert u.shape == (len(x), 1, p.N + 1)
        got = ck.lut_bootstrap(tv, x)
        assert got.shape == (len(x), 1, p.parties * p.n + 1)
        assert np.array_equal(got[:, 0], ck.bootstrap(x, mu))


@pytest.mark.parametrize("theta,n_inputs", [(1, 1), (2, 2), (4, 3), (1, 3), (4, 1)])
def test_mk2_bit_exact_against_the_composed_oracle(O, theta, n_inputs):
    p, K, ck = _keys(O, "MK2", 41, n=40)
    _check_exact(O, "MK2", p, K, ck, theta, n_inputs, 5, 300 + 10 * theta + n_inputs)
    ck.close()


@pytest.mark.parametrize("name,over,count,threshold,kernel", [
    ("MK2", dict(n=30), 4, 256, "mk_blind_rotate_coop_kernel<2>"),
    ("MK2", dict(n=30), 5, 0, "mk_blind_rotate_pair_kernel<2>"),          # an odd batch on the pair kernel
    ("MK4", dict(n=20), 3, 256, "mk_blind_rotate_coop_kernel<3>"),
    ("MK4", dict(n=20), 4, 0, "mk_blind_rotate_pair_kernel<3>"),
    ("MK8", dict(n=12), 3, 256, "mk_blind_rotate_coop_kernel<4>"),          # l = 4: coop only
    ("MK4-N2048", dict(n=10, parties=2), 3, 256, "mk_blind_rotate_coop2k_kernel<3>"),
    ("MK4-N2048", dict(n=10, parties=2), 3, 0, "mk_blind_rotate_pair2k_kernel<3>"),
    ("MK16", dict(n=8, parties=2), 3, 256, "mk_blind_rotate_coop2k_kernel<3>"),   # 26-bit base: three digit parts
    ("MK256", dict(n=6, parties=2), 3, 256, "kms_tlev_rotate_kernel"),      # the batched two-level path
    ("MK64-fft", dict(n=4, parties=2), 3, 256, "r4k_rotate_kernel"),        # N = 4096
])
def test_every_rotation_shape_bit_exact(O, name, over, count, threshold, kernel):
    p, K, ck = _keys(O, name, 43, **over)
    ck.set_pair_threshold(threshold)
    assert ck.rotation_kernel_name(count) == kernel
    for theta, n_inputs in ((1, 1), (4, 2)):
        _check_exact(O, name, p, K, ck, theta, n_inputs, count, 500 + theta)
    # the acceptance identity on this shape
    x = K.encrypt_bits([1, 0, 1, 1, 0][:count], O.SIGMAS[name]["lwe"], 77)
    tv = np.full(p.N, 1 << 61, np.int64)
    assert np.array_equal(ck.lut_bootstrap(tv, x)[:, 0], ck.bootstrap(x, 1 << 61))
    ck.close()


@pytest.mark.parametrize("name", ["MK2", "MK4"])
def test_function_values_decrypt(O, name, mk2):
    # every message of p = 2 and 4, theta = 1, 2, 4 (theta independent tables on the same input)
    from thfhe import lut
    if name == "MK2":
        p, K, ck = mk2
    else:
        p, K, ck = _keys(O, "MK4", 0x5EED0004)
    for p_msg in (2, 4):
        m = np.repeat(np.arange(p_msg), 3)
        x = enc_int(O, K, name, m, p_msg, 400 + p_msg)
        for theta in (1, 2, 4):
            fs = [lambda v, j=j: (v * (j + 1) + j) % p_msg for j in range(theta)]
            tv = lut.test_vector([lut.int_outputs(f, p_msg, torus_bits=64) for f in fs], p_msg, theta, p.N, torus_bits=64)
            out = ck.lut_bootstrap(tv, x, theta=theta)
            for j, f in enumerate(fs):
                assert np.array_equal(dec_int(K, out[:, j], p_msg), [f(v) for v in m]), (name, p_msg, theta, j)
    if name == "MK4":
        ck.close()


def test_bivariate_table(O, mk2):
    # f(a, b) = a XOR b ... as one table on 2a + b at p = 4 (weights (2, 1)), per-sample choice between two functions
    from thfhe import lut
    p, K, ck = mk2
    a, b = np.array([0, 0, 1, 1] * 2), np.array([0, 1, 0, 1] * 2)
    fa = lambda m: (m >> 1) ^ (m & 1)
    fb = lambda m: (m >> 1) & (m & 1)
    tv = np.stack([lut.test_vector(lut.int_outputs(f, 4, torus_bits=64), 4, 1, p.N, torus_bits=64) for f in (fa, fb)])
    idx = np.array([0, 0, 0, 0, 1, 1, 1, 1], np.int32)
    out = ck.lut_bootstrap(tv, enc_int(O, K, "MK2", a, 4, 500), enc_int(O, K, "MK2", b, 4, 501), weights=(2, 1), lut_index=idx)
    assert np.array_equal(dec_int(K, out[:, 0], 4), np.where(idx == 0, a ^ b, a & b))


def test_bootstrapped_input_chain(O, mk2):
    # two LUTs in a row at p = 4, the second fed the key-switched output of the first
    from thfhe import lut
    p, K, ck = mk2
    fs = [lambda m: (m + 1) % 4, lambda m: 3 - m]
    m = np.repeat(np.arange(4), 3)
    x, want = enc_int(O, K, "MK2", m, 4, 600), m.copy()
    for f in fs:
        x = ck.lut_bootstrap(lut.test_vector(lut.int_outputs(f, 4, torus_bits=64), 4, 1, p.N, torus_bits=64), x)[:, 0]
        want = np.array([f(v) for v in want])
        assert np.array_equal(dec_int(K, x, 4), want)


def test_many_lut_ripple_adder(O, mk2):
    # a + b on 16 pairs of 4-bit integers: bit i is ONE theta = 2 rotation of a_i + b_i + c_i at p = 4 with sum = parity, carry = majority
    from thfhe import lut
    p, K, ck = mk2
    rng = np.random.default_rng(65)
    A, B = rng.integers(0, 16, 16), rng.integers(0, 16, 16)
    tv = lut.test_vector([lut.int_outputs(lambda m: m & 1, 4, torus_bits=64), lut.int_outputs(lambda m: m >= 2, 4, torus_bits=64)], 4, 2, p.N,
                         torus_bits=64)
    carry, sums = None, []
    for i in range(4):
        ai, bi = enc_int(O, K, "MK2", (A >> i) & 1, 4, 700 + 2 * i), enc_int(O, K, "MK2", (B >> i) & 1, 4, 701 + 2 * i)
        if carry is None:
            out = ck.lut_bootstrap(tv, ai, bi, weights=(1, 1), theta=2)
        else:
            out = ck.lut_bootstrap(tv, ai, bi, carry, weights=(1, 1, 1), theta=2)
        sums.append(out[:, 0])
        carry = out[:, 1]
    bits = np.stack([dec_int(K, s, 4) for s in sums] + [dec_int(K, carry, 4)])
    assert np.all(bits <= 1)
    assert np.array_equal(sum(bits[i].astype(np.int64) << i for i in range(5)), A + B)


def test_invalid_calls_are_refused_and_the_context_stays_usable(O, mk2):
    import thfhe
    p, K, ck = mk2
    x = K.encrypt_bits([1, 0], O.SIGMAS["MK2"]["lwe"], 9)
    tv = np.full(p.N, 1 << 61, np.int64)
    with pytest.raises(thfhe.ThfheError):
        ck.lut_bootstrap(tv, x, lut_index=[0, 1])
    with pytest.raises(thfhe.ThfheError):
        ck.lut_bootstrap(tv, x, theta=3)
    assert ck.lut_bootstrap(tv, x[:0]).shape == (0, 1, p.parties * p.n + 1)
    assert np.array_equal(ck.lut_bootstrap(tv, x)[:, 0], ck.bootstrap(x, 1 << 61))


def test_a_profiled_dag_run_leaves_the_flat_calls_timings(O):
    # A stage of a gate-DAG run records no profiling events: after a profiled run, last_timings() still answers from the four events of the last
    # flat call and returns the same four floats.
    import thfhe
    p, K, ck = _keys(O, "MK2", 43, n=30)
    try:
        ck.set_profiling(True)
        rng = np.random.default_rng(811)
        x = R.encrypt_words(K, rng.integers(-2**31, 2**31, 3), O.SIGMAS["MK2"]["lwe"], 812)
        tvs = rng.integers(-2**63, 2**63, (2, p.N), dtype=np.int64)
        flat = ck.lut_bootstrap(tvs, x, lut_index=[0, 1, 0])
        before = ck.last_timings()
        assert all(np.isfinite(v) and v >= 0 for v in before.values())
        nodes = np.array([[thfhe.LUT, 0, -1, -1, 0, 0], [thfhe.LUT, 1, -1, -1, 0, 1]], np.int32)   # node g: table g on input g
        out, stats = ck.dag_run_lut_batch(x[None], nodes, [(1, (1, 0, 0), 0, 1)], tvs)
        assert stats["rotations"] == 2
        assert ck.last_timings() == before
        assert np.array_equal(out[0], flat[:2, 0])
    finally:
        ck.close()
