"""Encrypted lookup tables on the 3-gen multi-key engine on the MI355X (pytest -m gpu): thfhe_mk_lut_bootstrap_enc and its
_wo_keyswitch form, bit for bit against the reference composed from the CPU oracle's pieces (tests/mk_pack_reference.py) on every rotation shape of
the engine -- the shapes, batch sizes, thresholds and kernel names of tests/test_gpu_mk_lut.py -- with random words on both polynomials of the
tables, and against thfhe_mk_lut_bootstrap where the mask polynomial is zero."""
import numpy as np
import pytest

import mk_lut_reference as R
import mk_pack_reference as MP
from support import differing

pytestmark = pytest.mark.gpu


def _keys(O, name, seed, **over):
    import thfhe
    p = O.make_params(name, **over)
    s = O.SIGMAS[name]
    K = O.MKKeys(p, seed, s["bk"], s["ks"])
    ck = thfhe.MKCloudKey(thfhe.make_params(**p.as_dict()), K.bk, K.ksk, device=0)
    return p, K, ck


def _check_exact(O, name, p, K, ck, theta, n_inputs, count, seed):
    """Three random encrypted tables with a random index, random weights and bias: every word of both outputs against the composed reference."""
    orc = O.MKOracle(p, K.bk, K.ksk)
    rng = np.random.default_rng(seed)
    recs = [R.encrypt_words(K, rng.integers(-2**31, 2**31, count), O.SIGMAS[name]["lwe"], seed + q) for q in range(n_inputs)]
    recs[0][0, :-1] = 0     # a sample whose first operand has a zero mask (with one input: no CMux at all, the start alone is extracted)
    recs[0][1, 1] = 0       # a zero mask word
    weights = tuple(int(w) for w in rng.integers(-7, 8, n_inputs))
    bias = int(rng.integers(-2**31, 2**31))
    tv_a = rng.integers(-2**63, 2**63, (3, p.N), dtype=np.int64)
    tv_b = rng.integers(-2**63, 2**63, (3, p.N), dtype=np.int64)
    idx = rng.integers(0, 3, count).astype(np.int32)
    wo = ck.lut_bootstrap_enc_wo_keyswitch(tv_a, tv_b, *recs, weights=weights, bias=bias, theta=theta, lut_index=idx)
    ks = ck.lut_bootstrap_enc(tv_a, tv_b, *recs, weights=weights, bias=bias, theta=theta, lut_index=idx)
    assert wo.shape == (count, theta, p.N + 1) and ks.shape == (count, theta, p.parties * p.n + 1)
    for g in range(count):
        ref = MP.lut_bootstrap_enc(orc, [r[g] for r in recs], weights, bias, tv_a[idx[g]], tv_b[idx[g]], theta, keyswitch=False)
        assert np.array_equal(wo[g], ref), (name, theta, n_inputs, g, differing(wo[g], ref))
        assert np.array_equal(ks[g], np.stack([orc.keyswitch(u) for u in ref])), (name, theta, n_inputs, g)
    # a zero mask polynomial: the words of the plaintext entry
    plain = ck.lut_bootstrap(tv_b, *recs, weights=weights, bias=bias, theta=theta, lut_index=idx)
    assert np.array_equal(ck.lut_bootstrap_enc(np.zeros_like(tv_a), tv_b, *recs, weights=weights, bias=bias, theta=theta, lut_index=idx), plain)


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
    try:
        ck.set_pair_threshold(threshold)
        assert ck.rotation_kernel_name(count) == kernel
        for theta, n_inputs in ((1, 1), (4, 2)):
            _check_exact(O, name, p, K, ck, theta, n_inputs, count, 600 + theta)
    finally:
        ck.close()


def test_invalid_calls_are_refused_and_the_context_stays_usable(O):
    import thfhe
    p, K, ck = _keys(O, "MK2", 43, n=30)
    try:
        x = K.encrypt_bits([1, 0], O.SIGMAS["MK2"]["lwe"], 9)
        tv = np.full((1, p.N), 1 << 61, np.int64)
        zero = np.zeros_like(tv)
        with pytest.raises(thfhe.ThfheError):
            ck.lut_bootstrap_enc(zero, tv, x, lut_index=[0, 1])
        with pytest.raises(thfhe.ThfheError):
            ck.lut_bootstrap_enc(zero, tv, x, theta=3)
        assert ck.lut_bootstrap_enc(zero, tv, x[:0]).shape == (0, 1, p.parties * p.n + 1)
        assert np.array_equal(ck.lut_bootstrap_enc(zero, tv, x)[:, 0], ck.bootstrap(x, 1 << 61))
    finally:
        ck.close()
