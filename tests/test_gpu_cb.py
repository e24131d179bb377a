"""Circuit bootstrapping under real keys on the MI355X (pytest -m gpu): SK-128 and SK-80 with n reduced to 16, the level-2
context and the private key at full D = 2048 (tests/cb_cases.py; the keys are generated on the device once per module).  Address bits are NAND
outputs.  Every TGSW word equals the model; the rows' noise lies inside [0.5, 2] x the prediction; a leveled lookup and an automaton on the
bootstrapped set equal, word for word, the same calls on a set created by tgsw_set from the same words, equal the model, and decode.
tests/test_cb_host.py runs the same cases on the CPU model alone, which decodes every one of them (cb_cases.case asserts it before the device is
asked)."""
import numpy as np
import pytest

import cb_cases as CC
from support import N, differing

pytestmark = pytest.mark.gpu


class Dev:
    """the two contexts of a named set with the private key uploaded"""
    def __init__(self, O, name):
        import thfhe
        self.S = S = CC.keys(O, name, device=0)
        self.ck = thfhe.CloudKey(S.tp, S.K.bk, S.K.ksk, device=0)
        self.ck2 = thfhe.MKCloudKey(S.tp2, S.K2.bk, S.K2.ksk, device=0)
        self.ck.cb_key_set(self.ck2, S.pks, CC.T, CC.BASEBIT)
        self.case = CC.case(O, name, device=0)

    def close(self):
        self.ck.close()
        self.ck2.close()


@pytest.fixture(scope="module")
def sk128(O):
    d = Dev(O, "SK-128")
    yield d
    d.close()


@pytest.fixture(scope="module")
def sk80(O):
    d = Dev(O, "SK-80")
    yield d
    d.close()


@pytest.fixture(scope="module")
def boot128(sk128):
    """the 24 lookup bits as 8 samples of d = 3 and the 24 comparison bits as 4 samples of d = 6, with their words"""
    c = sk128.case
    lk, w_lk = sk128.ck.circuit_bootstrap(c["recs"][:24], 3, return_words=True)
    cmp_, w_cmp = sk128.ck.circuit_bootstrap(c["recs"][24:], 6, return_words=True)
    yield lk, w_lk, cmp_, w_cmp
    lk.close()
    cmp_.close()


def test_nand_layer_is_the_models(O, sk128):
    import thfhe
    S, c = sk128.S, sk128.case
    want = c["bits"].astype(bool)
    x = np.random.default_rng(0xCB00 + S.tp.l).integers(0, 2, want.shape[0]).astype(bool) | ~want
    got = sk128.ck.gates(thfhe.NAND, S.K.encrypt(x, 0xCB00 + S.tp.l + 1), S.K.encrypt(np.where(want, ~x, True), 0xCB00 + S.tp.l + 2))
    assert np.array_equal(got, c["recs"])       # the records the set is bootstrapped from are gate outputs of this device


def test_every_tgsw_word_equals_the_model(sk128, boot128):
    lk, w_lk, cmp_, w_cmp = boot128
    rows = sk128.case["rows"]
    assert (lk.count, lk.d, cmp_.count, cmp_.d) == (8, 3, 4, 6)
    assert np.array_equal(w_lk, rows[:24]), differing(w_lk, rows[:24])
    assert np.array_equal(w_cmp, rows[24:]), differing(w_cmp, rows[24:])


def test_row_noise_inside_the_band(sk128, boot128):
    S, c = sk128.S, sk128.case
    rows = np.concatenate([boot128[1], boot128[3]])
    std, pred = CC.row_noise(S, rows, c["bits"]), S.sigma_row()
    print(f"\ncb row noise SK-128: measured std {std:.3e} over {rows.size // 2} coefficients (GPU == CPU model word for word), predicted {pred:.3e}, "
          f"ratio {std / pred:.2f}")
    assert 0.5 * pred <= std <= 2 * pred


def check_lookup(d, tset, words):
    from thfhe import lut
    S, c = d.S, d.case
    got = d.ck.lhe_lookup(tset, c["tab"], d_tree=1, d_rot=2)
    with d.ck.tgsw_set(words, 3) as ts:
        same = d.ck.lhe_lookup(ts, c["tab"], d_tree=1, d_rot=2)
    assert np.array_equal(got, same), differing(got, same)
    assert np.array_equal(got, c["lookup"]), differing(got, c["lookup"])
    assert np.array_equal(lut.decode(S.K.phase(got).reshape(8), CC.P_OUT), c["table"][CC.ADDR])
    assert sorted(CC.ADDR.tolist()) == list(range(8))


def test_lookup_on_the_bootstrapped_set(sk128, boot128):
    check_lookup(sk128, boot128[0], boot128[1])


def test_equality_automaton_on_two_bootstrapped_operands(sk128, boot128):
    from thfhe import lut
    S, c = sk128.S, sk128.case
    trans, step_bit, fin_b, start = c["aut"]
    got = sk128.ck.lhe_wfa([boot128[2]], trans, step_bit, fin_b, start)
    with sk128.ck.tgsw_set(boot128[3], 6) as ts:
        same = sk128.ck.lhe_wfa([ts], trans, step_bit, fin_b, start)
    assert np.array_equal(got, same), differing(got, same)
    assert np.array_equal(got, c["wfa"]), differing(got, c["wfa"])
    assert np.array_equal(lut.decode(S.K.phase(got).reshape(4), CC.P_OUT), c["equal"])
    assert c["equal"].tolist() == [1, 0, 1, 0]


def test_sk80_lookup(sk80):
    c = sk80.case
    tset, words = sk80.ck.circuit_bootstrap(c["recs"], 3, return_words=True)
    try:
        assert np.array_equal(words, c["rows"]), differing(words, c["rows"])
        check_lookup(sk80, tset, words)
    finally:
        tset.close()


def test_slices_and_kernels_do_not_change_a_word(sk128, boot128):
    # one call over all 48 bits as d = 1 samples, on the plain kernel: the same words as the two calls above on the library's choice
    ck = sk128.ck
    ck.cb_set_batch_threshold(1 << 40)
    try:
        tset, words = ck.circuit_bootstrap(sk128.case["recs"], 1, return_words=True)
        tset.close()
    finally:
        ck.cb_set_batch_threshold(0)
    assert np.array_equal(words, sk128.case["rows"])


def test_key_generators_give_the_same_words_on_host_and_device(sk128):
    import thfhe
    from thfhe import keygen
    S = sk128.S
    z2 = S.z2[:24]
    for t, basebit in ((3, 5), (7, 4)):
        host = keygen.gen_cb_key(np.random.default_rng(77), z2, S.K.rlwe_key, t, basebit, 2.0**-31, chunk=50)
        dev = keygen.gen_cb_key(np.random.default_rng(77), z2, S.K.rlwe_key, t, basebit, 2.0**-31, chunk=50, device=0)
        assert host.shape == (2, 24, t, 2, N) and np.array_equal(host, dev)
    p2 = thfhe.make_params(**dict(thfhe.CB_PARAM_SETS["CB-128"], n=3))
    kw = dict(seed=78, sigma_bk=2.0**-62, lwe_keys=[[1, 0, 1]])
    a, b = keygen.MKSecretKeySet(p2, **kw), keygen.MKSecretKeySet(p2, device=0, **kw)
    assert np.array_equal(a.bk, b.bk) and np.array_equal(a.ksk, b.ksk) and a.lwe_keys.tolist() == [[1, 0, 1]]


def test_circuit_example(sk128):
    # circuits.cb_lookup: XOR gates compute the address, circuit bootstrapping makes it TGSW, a leveled lookup reads the table
    from thfhe import circuits, lut
    S = sk128.S
    rng = np.random.default_rng(0xCB40)
    a, b = rng.integers(0, 8, 4), rng.integers(0, 8, 4)
    table = rng.integers(0, 8, 8)
    enc = lambda v, seed: S.K.encrypt(lut.lhe_address_bits(v, 3), seed)
    got = circuits.cb_lookup(sk128.ck, enc(a, 0xCB41), enc(b, 0xCB42), table, p_out=8)
    assert got.shape == (4, S.tp.n + 1)
    assert np.array_equal(lut.decode(S.K.phase(got), 8), circuits.cb_lookup_plain(a, b, table))
