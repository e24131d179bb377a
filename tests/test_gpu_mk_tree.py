"""The two-digit tree on the 3-gen multi-key engine on the MI355X (pytest -m gpu): thfhe_mk_tree_lut_bootstrap word for word
against the three flat calls it stands for (thfhe_mk_lut_bootstrap_wo_keyswitch -> thfhe_mk_pack_boxes -> thfhe_mk_lut_bootstrap_enc) and against
the model composed from the CPU oracle's pieces (tests/mk_pack_reference.py), at every ring degree, whole and one sample per slice, on packing
keys of random words; the refused calls; and one full-size case on MK4 with a generated packing key, fresh inputs and every (hi, lo) decrypted."""
import time

import numpy as np
import pytest

import mk_lut_reference as R
import mk_pack_reference as MP
from support import differing, pmap

pytestmark = pytest.mark.gpu

# section 4.19's measured figures for MK4, torus units: the rotation's own noise and the multi-key key switch's
SIGMA_BR_MK4, SIGMA_KS_MK4 = 2.4e-3, 2.1e-2


def _keys(O, name, seed, **over):
    import thfhe
    p = O.make_params(name, **over)
    s = O.SIGMAS[name]
    K = O.MKKeys(p, seed, s["bk"], s["ks"])
    ck = thfhe.MKCloudKey(thfhe.make_params(**p.as_dict()), K.bk, K.ksk, device=0)
    return p, K, ck


def _flat(ck, tv1, lo, hi, p_hi, theta, wlo, blo, whi, bhi, idx):
    """the three flat calls in a row"""
    count, R_ = lo.shape[0], p_hi // theta
    lut_index = (idx[:, None] * R_ + np.arange(R_)[None, :]).reshape(-1)
    cand = ck.lut_bootstrap_wo_keyswitch(tv1.reshape(-1, tv1.shape[-1]), np.repeat(lo, R_, axis=0), weights=wlo, bias=blo, theta=theta, lut_index=lut_index)
    ta, tb = ck.pack_boxes(cand.reshape(count * p_hi, -1), p_hi)
    return ck.lut_bootstrap_enc(ta, tb, hi, weights=whi, bias=bhi, lut_index=np.arange(count))[:, 0]


@pytest.mark.parametrize("name,over,digits", [
    ("MK2", dict(n=30), (3, 2)),
    ("MK4-N2048", dict(n=10, parties=2), (2, 2)),
    ("MK64-fft", dict(n=4, parties=2), (2, 1)),
])
def test_tree_equals_the_flat_calls_and_the_model(O, name, over, digits):
    from thfhe import lut
    p, K, ck = _keys(O, name, 47, **over)
    try:
        orc = O.MKOracle(p, K.bk, K.ksk)
        rng = np.random.default_rng(p.N + 1)
        t, basebit = digits
        pk = rng.integers(-2**63, 2**63, (p.N, t, (1 << basebit) - 1, 2, p.N), dtype=np.int64)
        ck.pack_key_set(pk, t, basebit)
        ck.set_profiling(True)
        count = 5
        for p_hi, p_lo, theta in ((4, 4, 1), (4, 4, 2), (2, 8, 1)):
            tabs = rng.integers(0, 4, (2, p_hi, p_lo))
            tv1 = np.stack([lut.tree_test_vectors(lambda h, l, T=T: T[h, l], p_hi, p_lo, 4, theta, p.N, torus_bits=64) for T in tabs])
            lo = R.encrypt_words(K, rng.integers(-2**31, 2**31, count), O.SIGMAS[name]["lwe"], 50 + p_hi)
            hi = R.encrypt_words(K, rng.integers(-2**31, 2**31, count), O.SIGMAS[name]["lwe"], 60 + p_hi)
            idx = rng.integers(0, 2, count).astype(np.int32)
            wlo, blo, whi, bhi = (3,), int(rng.integers(-2**31, 2**31)), (-5,), int(rng.integers(-2**31, 2**31))
            kw = dict(p_hi=p_hi, weights_lo=wlo, bias_lo=blo, theta=theta, weights_hi=whi, bias_hi=bhi, table_index=idx)
            got = ck.tree_lut_bootstrap(tv1, lo, hi, **kw)
            assert got.shape == (count, p.parties * p.n + 1)
            ms = ck.last_timings()
            assert all(np.isfinite(v) and v >= 0 for v in ms.values()) and len(ms) == 4
            flat = _flat(ck, tv1, lo, hi, p_hi, theta, wlo, blo, whi, bhi, idx)
            assert np.array_equal(got, flat), (name, p_hi, theta, differing(got, flat))
            ref = pmap(lambda g: MP.tree(orc, pk, t, basebit, tv1[idx[g]], [lo[g]], [hi[g]], p_hi, wlo, blo, theta, whi, bhi), range(count))
            assert np.array_equal(got, np.stack(ref)), (name, p_hi, theta, differing(got, np.stack(ref)))
            ck.set_tree_slice(p_hi)       # one sample per slice
            try:
                sliced = ck.tree_lut_bootstrap(tv1, lo, hi, **kw)
            finally:
                ck.set_tree_slice(16384)
            assert np.array_equal(sliced, got), (name, p_hi, theta, "sliced")
            assert np.array_equal(ck.tree_lut_bootstrap(tv1[:1], lo, hi, **{**kw, "table_index": None}),
                                  _flat(ck, tv1, lo, hi, p_hi, theta, wlo, blo, whi, bhi, np.zeros(count, np.int32)))
    finally:
        ck.close()


def test_refused_calls_leave_the_context_usable(O):
    import thfhe
    from thfhe import lut
    p, K, ck = _keys(O, "MK2", 47, n=30)
    try:
        rng = np.random.default_rng(5)
        x = R.encrypt_words(K, rng.integers(-2**31, 2**31, 2), O.SIGMAS["MK2"]["lwe"], 70)
        tv1 = lut.tree_test_vectors(lambda h, l: h ^ l, 4, 4, 4, N=p.N, torus_bits=64)
        with pytest.raises(thfhe.ThfheError, match="no packing key"):
            ck.tree_lut_bootstrap(tv1, x, x, p_hi=4)
        small = rng.integers(-2**63, 2**63, (p.parties * p.n, 2, 3, 2, p.N), dtype=np.int64)
        ck.pack_key_set(small, 2, 2)
        with pytest.raises(thfhe.ThfheError, match="D = N"):
            ck.tree_lut_bootstrap(tv1, x, x, p_hi=4)
        pk = rng.integers(-2**63, 2**63, (p.N, 2, 3, 2, p.N), dtype=np.int64)
        ck.pack_key_set(pk, 2, 2)
        with pytest.raises(thfhe.ThfheError, match="p_hi"):
            ck.tree_lut_bootstrap(tv1[:3], x, x, p_hi=3)
        with pytest.raises(ValueError):                                   # theta_lo does not divide p_hi: the host layer has no row count to offer
            ck.tree_lut_bootstrap(tv1[:1], x, x, p_hi=2, theta=4)
        with pytest.raises(thfhe.ThfheError, match="table_index"):
            ck.tree_lut_bootstrap(tv1, x, x, p_hi=4, table_index=[0, 1])
        assert ck.tree_lut_bootstrap(tv1, x[:0], x[:0], p_hi=4).shape == (0, p.parties * p.n + 1)
        got = ck.tree_lut_bootstrap(tv1, x, x, p_hi=4)
        assert np.array_equal(got, _flat(ck, tv1[None], x, x, 4, 1, (1,), 0, (1,), 0, np.zeros(2, np.int32)))
    finally:
        ck.close()


@pytest.fixture(scope="module")
def mk4_full(O):
    """Full-size MK4 with the oracle's keys and a packing key from Z to Z of 12 one-bit digits (12 288 rows, 192 MiB), its ring products on the device."""
    import thfhe
    from thfhe import keygen
    p = O.make_params("MK4")
    s = O.SIGMAS["MK4"]
    K = O.MKKeys(p, 0x5EED0004, s["bk"], s["ks"])
    ck = thfhe.MKCloudKey(thfhe.make_params("MK4"), K.bk, K.ksk, device=0)
    Z = K.rlwe_keys.sum(axis=0)
    t0 = time.perf_counter()
    pk = keygen.gen_mk_pack_key(np.random.default_rng(0x5EED0014), Z, K.rlwe_keys, 12, 1, s["bk"], device=0)
    print(f"MK4 packing key (12, 1): {pk.shape[0] * 12} rows generated in {time.perf_counter() - t0:.2f} s")
    ck.pack_key_set(pk, 12, 1)
    yield p, s, K, ck, pk, Z
    ck.close()


def test_device_keygen_draws_the_host_words(O, mk4_full):
    # the same random stream either way: a few rows of the key on the host equal the device-generated ones
    from thfhe import keygen
    p, s, K, ck, pk, Z = mk4_full
    host = keygen.gen_mk_pack_key(np.random.default_rng(0x5EED0014), Z[:5], K.rlwe_keys, 6, 2, s["bk"], chunk=32)
    dev = keygen.gen_mk_pack_key(np.random.default_rng(0x5EED0014), Z[:5], K.rlwe_keys, 6, 2, s["bk"], chunk=32, device=0)
    assert host.shape == (5, 6, 3, 2, p.N) and np.array_equal(host, dev)
    # ... and the fixture's key is a key: its first rows decrypt under Z to their messages
    rows = pk[:2].reshape(-1, 2, p.N)
    ph = (rows[:, 1].view(np.uint64) - keygen.polymul_small64(rows[:, 0], Z).view(np.uint64)).view(np.int64)
    msg = np.repeat(Z[:2], 12).astype(np.uint64) << (63 - np.tile(np.arange(12), 2)).astype(np.uint64)
    ph[:, 0] = (ph[:, 0].view(np.uint64) - msg).view(np.int64)
    assert np.abs(ph).max() <= 6 * s["bk"] * 2.0 * 2.0**64


def test_mk4_full_size_tree_decrypts_every_pair_and_feeds_the_gates(O, mk4_full):
    import thfhe
    from thfhe import lut
    p, s, K, ck, pk, Z = mk4_full
    orc = O.MKOracle(p, K.bk, K.ksk)
    f = lambda h, l: ((h * 5 + l * 3 + (h & l)) >> 1) & 1
    tv1 = np.stack([lut.test_vector(lut.bool_outputs(lambda l, h=h: f(h, l), 4, torus_bits=64), 4, N=p.N, torus_bits=64) for h in range(4)])
    pairs = np.array([(h, l) for h in range(4) for l in range(4)])
    hi = R.encrypt_words(K, lut.encode(pairs[:, 0], 4), s["lwe"], 0x5EED0041)
    lo = R.encrypt_words(K, lut.encode(pairs[:, 1], 4), s["lwe"], 0x5EED0042)
    got = ck.tree_lut_bootstrap(tv1, lo, hi, p_hi=4)
    want = np.array([f(h, l) for h, l in pairs]).astype(bool)
    # the model, word for word, where the oracle is fast enough: one sample's five rotations of 2 040 CMuxes each, level 1 side by side
    g = 6
    cand = np.concatenate(pmap(lambda row: R.lut_bootstrap(orc, [lo[g]], (1,), 0, row, 1, keyswitch=False), tv1))
    ta, tb = MP.pack(cand, pk, 12, 1, 4)
    ref = MP.lut_bootstrap_enc(orc, [hi[g]], (1,), 0, ta[0], tb[0], 1)[0]
    assert np.array_equal(got[g], ref), (g, differing(got[g], ref))
    assert K.decrypt_bits(ref[None])[0] == want[g]
    # every output decrypts; none is left out of the count
    err = (K.phases(got).astype(np.int64) - np.where(want, 1 << 29, -(1 << 29))) / 2.0**32
    rounding = np.sqrt(float((Z.astype(np.float64)**2).sum()) / 12) * 2.0**-12
    key = np.sqrt(p.N * p.N * 12 * p.parties * 0.5) * s["bk"]           # half of the one-bit digits are non-zero
    pred = np.sqrt(2 * SIGMA_BR_MK4**2 + rounding**2 + key**2 + SIGMA_KS_MK4**2)
    print(f"MK4 tree p = 4 x 4 -> 2: measured std {err.std():.3e} over {len(err)} outputs, max |err| {np.abs(err).max():.3e}; predicted {pred:.3e} "
          f"(rounding {rounding:.2e}, key {key:.2e}); half-step / predicted {0.125 / pred:.1f}")
    assert np.array_equal(K.decrypt_bits(got), want)
    assert 0.5 * pred <= err.std() <= 2 * pred
    # two outputs into the multi-key NAND
    a, b = got[0::2], got[1::2]
    nand = ck.gates(thfhe.NAND, a, b)
    assert np.array_equal(K.decrypt_bits(nand), ~(want[0::2] & want[1::2]))
