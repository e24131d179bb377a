"""Multi-value bootstrapping on every rotation shape of the 3-gen multi-key engine (pytest -m gpu): the ten shapes of
test_gpu_mk_lut.py::test_every_rotation_shape_bit_exact -- same reduced n, parties, counts, thresholds and kernel names -- with random-word records,
a random int64 base vector, random int32 taps, two tables with a per-sample index and a random out_bias: every word with and without the key switch
against the model composed from the CPU oracle's pieces (tests/mk_mv_lut_reference.py), a zero-mask sample among ordinary ones, and a call cut into
slices against the uncut one.

The single-tap identity.  With tv0 = 2^61 everywhere and one output whose only tap is c[p-1] = -1, tv0 * F is, by the identity of
test_mk_mv_lut_host.py, the test vector of the constant table +2^61 (asserted on the CPU first: the sign is +).  The output therefore encrypts what
mk_lut_bootstrap_wo_keyswitch of that test vector encrypts.  It is the same WORDS only where no CMux runs (the zero-mask sample): the two calls start
from accumulators that differ by the monomial X^(-box/2), and the gadget decomposition inside a CMux does not commute with the sign changes of a
negacyclic shift (it truncates the low bits, so digits(-x) != -digits(x)), so after the first CMux the masks differ in every word -- the model shows
the same on the CPU, all N + 1 words.  The test asserts word equality on the zero-mask sample and, on the ordinary samples, that both records decrypt
under the ring key sum_i z_i to the same +-2^29 within 2^27 (the rotation noise of these reduced sets is below 2^25 at one sigma, section 4.19's table scaled
by sqrt(n / n_full))."""
import numpy as np
import pytest

import mk_lut_reference as R
import mk_mv_lut_reference as MV
from support import differing, pmap

pytestmark = pytest.mark.gpu

# the rows of test_gpu_mk_lut.py::test_every_rotation_shape_bit_exact
SHAPES = [
    ("MK2", dict(n=30), 4, 256, "mk_blind_rotate_coop_kernel<2>"),
    ("MK2", dict(n=30), 5, 0, "mk_blind_rotate_pair_kernel<2>"),
    ("MK4", dict(n=20), 3, 256, "mk_blind_rotate_coop_kernel<3>"),
    ("MK4", dict(n=20), 4, 0, "mk_blind_rotate_pair_kernel<3>"),
    ("MK8", dict(n=12), 3, 256, "mk_blind_rotate_coop_kernel<4>"),
    ("MK4-N2048", dict(n=10, parties=2), 3, 256, "mk_blind_rotate_coop2k_kernel<3>"),
    ("MK4-N2048", dict(n=10, parties=2), 3, 0, "mk_blind_rotate_pair2k_kernel<3>"),
    ("MK16", dict(n=8, parties=2), 3, 256, "mk_blind_rotate_coop2k_kernel<3>"),
    ("MK256", dict(n=6, parties=2), 3, 256, "kms_tlev_rotate_kernel"),
    ("MK64-fft", dict(n=4, parties=2), 3, 256, "r4k_rotate_kernel"),
]


def _keys(O, name, seed, **over):
    import thfhe
    p = O.make_params(name, **over)
    s = O.SIGMAS[name]
    K = O.MKKeys(p, seed, s["bk"], s["ks"])
    ck = thfhe.MKCloudKey(thfhe.make_params(**p.as_dict()), K.bk, K.ksk, device=0)
    return p, K, ck


def _check_exact(O, name, p, K, ck, orc, taps, q, n_inputs, count, seed):
    """one (p, q) case: both outputs against the model word for word, then the sliced calls against the uncut one"""
    rng = np.random.default_rng(seed)
    sigma = O.SIGMAS[name]["lwe"]
    recs = [R.encrypt_words(K, rng.integers(-2**31, 2**31, count), sigma, seed + i) for i in range(n_inputs)]
    for r in recs:
        r[1, :-1] = 0     # a zero-mask sample among ordinary ones: every CMux of its chain is skipped
    weights = tuple(int(w) for w in rng.integers(-7, 8, n_inputs))
    bias = int(rng.integers(-2**31, 2**31))
    tv0 = rng.integers(-2**63, 2**63, p.N, dtype=np.int64)
    fac = rng.integers(-2**31, 2**31, (2, q, taps)).astype(np.int32)
    idx = (np.arange(count) % 2).astype(np.int32)[::-1].copy()
    out_bias = int(rng.integers(-2**63, 2**63, dtype=np.int64))
    kw = dict(tv0=tv0, weights=weights, bias=bias, table_index=idx, out_bias=out_bias)
    wo = ck.mv_lut_bootstrap_wo_keyswitch(fac, *recs, **kw)
    ks = ck.mv_lut_bootstrap(fac, *recs, **kw)
    assert wo.shape == (count, q, p.N + 1) and ks.shape == (count, q, p.parties * p.n + 1)
    ref = pmap(lambda g: MV.mv_lut(orc, [r[g] for r in recs], weights, bias, tv0, fac[idx[g]], out_bias, keyswitch=False), range(count))
    for g in range(count):
        assert np.array_equal(wo[g], ref[g]), (name, taps, q, g, differing(wo[g], ref[g]))
    picks = [(g, j) for g in range(count) for j in range(q)]
    ref_ks = pmap(lambda gj: orc.keyswitch(ref[gj[0]][gj[1]]), picks)
    for (g, j), want in zip(picks, ref_ks):
        assert np.array_equal(ks[g, j], want), (name, taps, q, g, j)
    try:   # one sample per slice (count >= 3 slices), then two: only a slice's inputs and table indices go up, its records come down
        for per_slice in (1, 2):
            ck.set_mv_slice(per_slice * q)
            assert np.array_equal(ck.mv_lut_bootstrap_wo_keyswitch(fac, *recs, **kw), wo), (name, taps, q, per_slice)
            assert np.array_equal(ck.mv_lut_bootstrap(fac, *recs, **kw), ks), (name, taps, q, per_slice)
    finally:
        ck.set_mv_slice(4096)


def _ring_phase(K, rec):
    """phase of an extracted record of N + 1 words under the ring key sum_i z_i, as a Torus32 word"""
    z = K.rlwe_keys.astype(np.int64).sum(axis=0)
    return int((int(rec[-1]) - int(np.dot(rec[:-1].astype(np.int64), z))) % (1 << 32))


def _check_single_tap_identity(O, name, p, K, ck, count, taps):
    from thfhe import lut
    from test_mk_mv_lut_host import factor_poly, negacyclic_mul64
    N = p.N
    tv0 = np.full(N, 1 << 61, np.int64)
    c = np.zeros((1, taps), np.int32)
    c[0, taps - 1] = -1
    tvc = lut.test_vector(np.full(taps, 1 << 61, np.int64), taps, N=N, torus_bits=64)
    assert np.array_equal(negacyclic_mul64(tv0, factor_poly(c[0], N), N), tvc)   # the sign, from the identity, on the CPU
    x = R.encrypt_words(K, np.random.default_rng(taps).integers(-2**31, 2**31, count), O.SIGMAS[name]["lwe"], 900 + taps)
    x[1, :-1] = 0
    a = ck.mv_lut_bootstrap_wo_keyswitch(c, x, tv0=tv0)[:, 0]
    b = ck.lut_bootstrap_wo_keyswitch(tvc, x)[:, 0]
    assert np.array_equal(a[1], b[1]), name
    for g in range(count):   # random-word inputs: the rotation ends in the positive or the negated half of the test vector, the same in both calls
        want = (1 << 29) if _ring_phase(K, b[g]) < (1 << 31) else -(1 << 29)
        for rec in (a[g], b[g]):
            d = (_ring_phase(K, rec) - want + (1 << 31)) % (1 << 32) - (1 << 31)
            assert abs(d) < 1 << 27, (name, g, d)


@pytest.mark.parametrize("name,over,count,threshold,kernel", SHAPES, ids=[f"{s[0]}-{s[4]}" for s in SHAPES])
def test_every_rotation_shape_bit_exact(O, name, over, count, threshold, kernel):
    p, K, ck = _keys(O, name, 43, **over)
    try:
        ck.set_pair_threshold(threshold)
        assert ck.rotation_kernel_name(count) == kernel
        orc = O.MKOracle(p, K.bk, K.ksk)
        cases = [(64, 9, 2)]
        if name in ("MK2", "MK64-fft"):
            cases += [(2, 1, 1), (8, 64, 3)]
        for taps, q, n_inputs in cases:
            _check_exact(O, name, p, K, ck, orc, taps, q, n_inputs, count, 700 + taps)
        _check_single_tap_identity(O, name, p, K, ck, count, 64)
    finally:
        ck.close()
