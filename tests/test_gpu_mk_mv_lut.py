"""Multi-value bootstrapping on the 3-gen multi-key engine with real keys on the MI355X (pytest -m gpu), full-size parameter
sets and fresh inputs: bit functions of one encrypted digit in the gates' encoding (thfhe.lut.mv_bool_factors: 0/1 tables at step 2^62, out_bias
-2^61) from ONE blind rotation, word for word against the model composed from the CPU oracle's pieces and decrypted.  The model runs first on the
fixed seeds; an output counts as a decryption case only where the model decrypts it, and the tests assert that every case inside section 4.19's
supported set is one -- a case the model loses there would be a finding for the noise table, not a seed to change.  MK16 is decrypt-only: an oracle
rotation of its 9 440 CMuxes takes 16 s per sample."""
import numpy as np
import pytest

import mk_lut_reference as R
import mk_mv_lut_reference as MV
from support import differing, pmap

pytestmark = pytest.mark.gpu

# section 4.19's table: the rotation's own noise and the key switch's, torus units
SIGMA_BR = {"MK2": 1.6e-2, "MK4": 2.4e-3}
SIGMA_KS = {"MK2": 2.2e-2, "MK4": 2.1e-2}


def _keys(O, name, seed):
    import thfhe
    p = O.make_params(name)
    s = O.SIGMAS[name]
    K = O.MKKeys(p, seed, s["bk"], s["ks"])
    return p, K, thfhe.MKCloudKey(thfhe.make_params(name), K.bk, K.ksk, device=0)


def _digit_case(O, name, seed, tables, reps):
    """every message of a p = 4 digit, `reps` fresh encryptions each, through the bit tables: (K, ck, orc, messages, GPU records, model records)"""
    from thfhe import lut
    p, K, ck = _keys(O, name, seed)
    orc = O.MKOracle(p, K.bk, K.ksk)
    m = np.repeat(np.arange(4), reps)
    x = R.encrypt_words(K, lut.encode(m, 4), O.SIGMAS[name]["lwe"], seed + 1)
    tv0, c, ob = lut.mv_bool_factors(tables, 4, 64, p.N)
    got = ck.mv_lut_bootstrap(c, x, tv0=tv0, out_bias=ob)
    wo = ck.mv_lut_bootstrap_wo_keyswitch(c, x, tv0=tv0, out_bias=ob)
    ref_wo = pmap(lambda g: MV.mv_lut(orc, [x[g]], (1,), 0, tv0, c, ob, keyswitch=False), range(len(m)))
    for g in range(len(m)):
        assert np.array_equal(wo[g], ref_wo[g]), (name, g, differing(wo[g], ref_wo[g]))
    ref = np.stack(pmap(lambda g: np.stack([orc.keyswitch(u) for u in ref_wo[g]]), range(len(m))))
    assert np.array_equal(got, ref), (name, differing(got, ref))
    return p, K, ck, orc, m, got, ref, c


def _report(name, K, recs, want, norms):
    """measured standard deviation of the outputs' phases around +-2^29 next to the prediction |c|_2 sigma_br (+) sigma_ks"""
    ph = K.phases(recs.reshape(-1, recs.shape[-1])).astype(np.int64).reshape(recs.shape[:-1])
    err = (ph - np.where(want, 1 << 29, -(1 << 29))) / 2.0**32
    for j, nrm in enumerate(norms):
        pred = np.hypot(nrm * SIGMA_BR[name], SIGMA_KS[name])
        print(f"{name} output {j}: |c|_2 {nrm:.2f}  measured std {err[:, j].std():.2e} over {err.shape[0]} samples  predicted {pred:.2e}  "
              f"half-step / predicted {0.125 / pred:.1f}")


def test_mk2_three_step_functions_of_a_digit_feed_the_gates(O):
    import thfhe
    tables = [[int(v >= t) for v in range(4)] for t in (1, 2, 3)]
    p, K, ck, orc, m, got, ref, c = _digit_case(O, "MK2", 0x5EED0002, tables, 2)
    try:
        want = np.array([[v >= t for t in (1, 2, 3)] for v in m])
        model_ok = np.stack([K.decrypt_bits(ref[:, j]) for j in range(3)], axis=1) == want
        _report("MK2", K, got, want, np.linalg.norm(c, axis=1))
        assert model_ok.all(), ("the model loses a step function of a fresh p = 4 digit on MK2", np.argwhere(~model_ok).tolist())
        assert np.array_equal(np.stack([K.decrypt_bits(got[:, j]) for j in range(3)], axis=1), want)
        # the outputs are gate operands as they are: NAND of neighbouring thresholds, word for word against the oracle's gate; two such operands sum
        # to 2.8 sigma of a gate's half-box (section 4.19), so a decryption counts only where the oracle's own gate decrypts
        for a, b in ((0, 1), (1, 2)):
            g = ck.gates(thfhe.NAND, got[:, a], got[:, b])
            r = orc.gates(O.NAND, ref[:, a], ref[:, b])
            assert np.array_equal(g, r), (a, b)
            nand = ~(want[:, a] & want[:, b])
            ok = K.decrypt_bits(r) == nand
            print(f"MK2 NAND of outputs {a}, {b}: the oracle decrypts {int(ok.sum())} of {len(ok)}")
            assert np.array_equal(K.decrypt_bits(g)[ok], nand[ok])
    finally:
        ck.close()


def test_mk4_bits_and_thresholds_of_a_digit(O):
    # q = 5: the two bits of m and [m >= 1], [m >= 2], [m >= 3]; |c|_2 = 2 for the low bit, sqrt 2 for the others
    tables = [[v & 1 for v in range(4)], [v >> 1 for v in range(4)]] + [[int(v >= t) for v in range(4)] for t in (1, 2, 3)]
    p, K, ck, orc, m, got, ref, c = _digit_case(O, "MK4", 0x5EED0004, tables, 1)
    try:
        norms = np.linalg.norm(c, axis=1)
        assert norms.max() <= 2.0
        want = np.array([[tab[v] for tab in tables] for v in m]).astype(bool)
        model_ok = np.stack([K.decrypt_bits(ref[:, j]) for j in range(5)], axis=1) == want
        _report("MK4", K, got, want, norms)
        assert model_ok.all(), ("the model loses a bit function of a fresh p = 4 digit on MK4", np.argwhere(~model_ok).tolist())
        assert np.array_equal(np.stack([K.decrypt_bits(got[:, j]) for j in range(5)], axis=1), want)
    finally:
        ck.close()


def test_mk16_sixteen_random_bit_tables_decrypt(O):
    # 16 arbitrary bit tables of a p = 8 digit from one rotation of 9 440 CMuxes: |c|_2 <= 3.3 times sigma_br = 3.1e-5 is nothing next to the key switch
    from thfhe import lut
    p, K, ck = _keys(O, "MK16", 85)
    try:
        rng = np.random.default_rng(16)
        tables = rng.integers(0, 2, (16, 8))
        m = np.array([0, 3, 5, 7])
        x = R.encrypt_words(K, lut.encode(m, 8), O.SIGMAS["MK16"]["lwe"], 86)
        tv0, c, ob = lut.mv_bool_factors(tables, 8, 64, p.N)
        got = ck.mv_lut_bootstrap(c, x, tv0=tv0, out_bias=ob)
        assert got.shape == (4, 16, p.parties * p.n + 1)
        dec = np.stack([K.decrypt_bits(got[:, j]) for j in range(16)], axis=1)
        assert np.array_equal(dec, tables[:, m].T.astype(bool))
    finally:
        ck.close()
