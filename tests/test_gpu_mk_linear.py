"""Encrypted dense layers on the 3-gen multi-key engine (pytest -m gpu), on the reduced MK2 shape of
test_gpu_mk_mv_lut_shapes.py (n = 30, two parties: records of 2 n + 1 = 61 words): thfhe_mk_lwe_linear against numpy, the fused call with theta = 1
and 2 against the model composed from the CPU oracle (tests/mk_lut_reference.py) and against the two public calls in a row, with and without the key
switch, and one slice boundary.  Random words, not valid ciphertexts; the contract is word equality."""
import numpy as np
import pytest

import linear_reference as LR
import mk_lut_reference as R
from support import differing, pmap, words

pytestmark = pytest.mark.gpu

M, K, COUNT = 3, 5, 5
IDX = np.array([1, 2, 0], np.int32)


@pytest.fixture(scope="module")
def mk2(O):
    import thfhe
    p = O.make_params("MK2", n=30)
    s = O.SIGMAS["MK2"]
    keys = O.MKKeys(p, 43, s["bk"], s["ks"])
    ck = thfhe.MKCloudKey(thfhe.make_params(**p.as_dict()), keys.bk, keys.ksk, device=0)
    yield p, O.MKOracle(p, keys.bk, keys.ksk), ck
    ck.close()


def test_mk_lwe_linear(mk2):
    p, orc, ck = mk2
    rec = p.parties * p.n + 1
    assert ck.words == rec == 61
    rng = np.random.default_rng(2900)
    W, x, b = words(rng, M, K), words(rng, COUNT, K, rec), words(rng, M)
    for bias in (None, b):
        got = ck.lwe_linear(W, x, bias)
        ref = LR.linear(W, x, bias)
        assert got.shape == (COUNT, M, rec) and np.array_equal(got, ref), differing(got, ref)


@pytest.mark.parametrize("theta", [1, 2])
def test_mk_fused_equals_composed_equals_model(mk2, theta):
    p, orc, ck = mk2
    rec, N = p.parties * p.n + 1, p.N
    rng = np.random.default_rng(2910 + theta)
    W, x, b = words(rng, M, K), words(rng, COUNT, K, rec), words(rng, M)
    tv = rng.integers(-2**63, 2**63, (3, N), dtype=np.int64)
    assert ck.rotation_kernel_name(COUNT * M) == "mk_blind_rotate_coop_kernel<2>"
    wo = LR.fused(R.lut_bootstrap, orc, W, x, b, tv, theta, IDX, False, pmap)
    ks = np.stack(pmap(lambda u: orc.keyswitch(u), wo.reshape(-1, N + 1))).reshape(COUNT, M, theta, rec)
    xs = ck.lwe_linear(W, x, b)
    flat = np.tile(IDX, COUNT)
    try:
        for setting in (4096, 2 * M):   # one slice, then slices of two samples: 2 + 2 + 1
            ck.set_linear_slice(setting)
            u = ck.linear_lut_bootstrap_wo_keyswitch(tv, W, x, b, theta=theta, lut_index=IDX)
            assert u.shape == (COUNT, M, theta, N + 1)
            assert np.array_equal(u, wo), (setting, differing(u, wo))
            got = ck.linear_lut_bootstrap(tv, W, x, b, theta=theta, lut_index=IDX)
            assert got.shape == (COUNT, M, theta, rec)
            assert np.array_equal(got, ks), (setting, differing(got, ks))
            two = ck.lut_bootstrap(tv, xs.reshape(-1, rec), theta=theta, lut_index=flat).reshape(got.shape)
            assert np.array_equal(got, two), (setting, differing(got, two))
            two = ck.lut_bootstrap_wo_keyswitch(tv, xs.reshape(-1, rec), theta=theta, lut_index=flat).reshape(u.shape)
            assert np.array_equal(u, two), (setting, differing(u, two))
            # a call without an index after one with: table 0 for every output
            none = ck.linear_lut_bootstrap(tv, W, x, b, theta=theta)
            want = ck.lut_bootstrap(tv, xs.reshape(-1, rec), theta=theta).reshape(got.shape)
            assert np.array_equal(none, want) and not np.array_equal(none, got), setting
    finally:
        ck.set_linear_slice(4096)
