"""Circuit bootstrapping in one-rotation mode on the MI355X (pytest -m gpu): the l records of a bit from ONE level-2
rotation.  The cases are those of tests/test_gpu_cb.py (tests/cb_cases.py: SK-128 and SK-80 with n = 16, level 2 and the private key at full
D = 2048, (t, basebit) = (7, 4)); the model is tests/cb_one_reference.py, which has decoded every lookup and comparison before the device is asked.
Every word is compared, no tolerance:

  stage A alone      thfhe_cb_stage_a in both modes against the two models: SK-128 uses three of theta = 4 slots, SK-80 both of theta = 2
  the full call      words, row noise, a leveled lookup and an automaton on the returned set, circuits.cb_lookup
  interleaving       both modes, stage B alone, gates and a level-2 bootstrap on ONE pair of contexts
  boundaries         257 bits (the pair kernel's last workgroup holds one job) and 2 049 bits (slices of 2 048 + 1) at d = 1, on both sets

A large batch is a random draw (cb_cases.drawn) from the pool whose one-rotation rows the model holds; words are compared in chunks of 256 bits and
a mismatch names the first differing bit."""
import numpy as np
import pytest

import cb_cases as CC
import cb_one_reference as R
import lhe_reference as LR
from support import N, differing
from test_gpu_cb import Dev

pytestmark = pytest.mark.gpu

PAIR, SINGLE = "kms_tlev_rotate_pair_kernel", "kms_tlev_rotate_kernel"
CHUNK = 256
SETS = ("SK-128", "SK-80")


@pytest.fixture(scope="module")
def devs(O):
    made = {}

    def get(name):
        if name not in made:
            d = Dev(O, name)
            d.m = R.models(O, name, device=0)
            made[name] = d
        return made[name]
    yield get
    for d in made.values():
        d.close()


def assert_rows(words, rows, idx, what):
    """the words of a call on a drawn batch against the same draw from the model's rows, chunk by chunk"""
    assert words.shape == (len(idx),) + rows.shape[1:], (what, words.shape)
    for b0 in range(0, len(idx), CHUNK):
        g, w = words[b0:b0 + CHUNK], rows[idx[b0:b0 + CHUNK]]
        if not np.array_equal(g, w):
            bad = differing(g, w)
            raise AssertionError("%s: first difference at bit %d of %d; (bit - %d, row, part, word) of the first mismatches: %s" % (
                what, b0 + bad[0][0], len(idx), b0, bad))


def one(d, recs, dd):
    tset, words = d.ck.circuit_bootstrap(recs, dd, return_words=True, one_rotation=True)
    tset.close()
    return words


# ---- stage A alone ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", SETS)
def test_stage_a_alone_equals_the_model_in_both_modes(devs, name):
    d = devs(name)
    S, c, m = d.S, d.case, d.m
    l = S.tp.l
    assert (len(c["recs"]), R.theta(l), l) == ((48, 4, 3) if name == "SK-128" else (24, 2, 2))   # one slot empty / every slot used
    got = d.ck.cb_stage_a(c["recs"], one_rotation=True)
    assert got.shape == m["lwe2_one"].shape == (len(c["recs"]), l, CC.D2 + 1)
    assert np.array_equal(got, m["lwe2_one"]), differing(got, m["lwe2_one"])
    err = int(np.abs(R.lwe2_errors(S.z2, got, c["bits"], l, S.tp.Bgbit)).max())
    print(f"\nstage A {name}, one rotation, device: worst |phase - m g_j| = {err} units of 2^-32 (half-step {1 << (31 - l * S.tp.Bgbit)})")
    assert 4 * err < 1 << (31 - l * S.tp.Bgbit)
    plain = d.ck.cb_stage_a(c["recs"])
    assert np.array_equal(plain, m["lwe2"]), differing(plain, m["lwe2"])
    # stage B alone on the device's stage A is the full call
    rows = d.ck.cb_private_keyswitch(got)
    assert np.array_equal(rows, m["rows"]), differing(rows, m["rows"])


# ---- the full call ---------------------------------------------------------------------------------------------------------------------------

def check_lookup(d, tset, words):
    from thfhe import lut
    S, c, m = d.S, d.case, d.m
    got = d.ck.lhe_lookup(tset, c["tab"], d_tree=1, d_rot=2)
    with d.ck.tgsw_set(words, 3) as ts:
        same = d.ck.lhe_lookup(ts, c["tab"], d_tree=1, d_rot=2)
    assert np.array_equal(got, same), differing(got, same)
    assert np.array_equal(got, m["lookup"]), differing(got, m["lookup"])
    assert np.array_equal(lut.decode(S.K.phase(got).reshape(8), CC.P_OUT), c["table"][CC.ADDR])
    assert sorted(CC.ADDR.tolist()) == list(range(8))


def test_sk128_full_call_words_noise_lookup_and_automaton(devs):
    from thfhe import lut
    d = devs("SK-128")
    S, c, m = d.S, d.case, d.m
    lk, w_lk = d.ck.circuit_bootstrap(c["recs"][:24], 3, return_words=True, one_rotation=True)
    cmp_, w_cmp = d.ck.circuit_bootstrap(c["recs"][24:], 6, return_words=True, one_rotation=True)
    try:
        assert (lk.count, lk.d, cmp_.count, cmp_.d) == (8, 3, 4, 6)
        assert np.array_equal(w_lk, m["rows"][:24]), differing(w_lk, m["rows"][:24])
        assert np.array_equal(w_cmp, m["rows"][24:]), differing(w_cmp, m["rows"][24:])
        assert not np.array_equal(w_lk, c["rows"][:24])                           # the mode gives other words than the default
        std, pred = CC.row_noise(S, np.concatenate([w_lk, w_cmp]), c["bits"]), S.sigma_row()
        print(f"\ncb row noise SK-128, one rotation: measured std {std:.3e}, predicted {pred:.3e}, ratio {std / pred:.2f}")
        assert 0.5 * pred <= std <= 2 * pred
        check_lookup(d, lk, w_lk)
        trans, step_bit, fin_b, start = c["aut"]
        got = d.ck.lhe_wfa([cmp_], trans, step_bit, fin_b, start)
        with d.ck.tgsw_set(w_cmp, 6) as ts:
            same = d.ck.lhe_wfa([ts], trans, step_bit, fin_b, start)
        assert np.array_equal(got, same), differing(got, same)
        assert np.array_equal(got, m["wfa"]), differing(got, m["wfa"])
        assert np.array_equal(lut.decode(S.K.phase(got).reshape(4), CC.P_OUT), c["equal"])
        assert c["equal"].tolist() == [1, 0, 1, 0]
    finally:
        lk.close()
        cmp_.close()


def test_sk80_full_call_words_noise_and_lookup(devs):
    d = devs("SK-80")
    S, c, m = d.S, d.case, d.m
    tset, words = d.ck.circuit_bootstrap(c["recs"], 3, return_words=True, one_rotation=True)
    try:
        assert np.array_equal(words, m["rows"]), differing(words, m["rows"])
        std, pred = CC.row_noise(S, words, c["bits"]), S.sigma_row()
        print(f"\ncb row noise SK-80, one rotation: measured std {std:.3e}, predicted {pred:.3e}, ratio {std / pred:.2f}")
        assert 0.5 * pred <= std <= 2 * pred
        check_lookup(d, tset, words)
    finally:
        tset.close()


@pytest.mark.parametrize("name", SETS)
def test_circuit_example_in_one_rotation_mode(devs, name):
    from thfhe import circuits, lut
    d = devs(name)
    S = d.S
    rng = np.random.default_rng(0xCB50)
    a, b = rng.integers(0, 8, 4), rng.integers(0, 8, 4)
    table = rng.integers(0, 8, 8)
    enc = lambda v, seed: S.K.encrypt(lut.lhe_address_bits(v, 3), seed)
    got = circuits.cb_lookup(d.ck, enc(a, 0xCB51), enc(b, 0xCB52), table, p_out=8, one_rotation=True)
    assert got.shape == (4, S.tp.n + 1)
    assert np.array_equal(lut.decode(S.K.phase(got), 8), circuits.cb_lookup_plain(a, b, table))


# ---- interleaving on one pair of contexts ----------------------------------------------------------------------------------------------------

def test_modes_interleave_on_one_pair_of_contexts(O, devs):
    """the two modes share the grow-only buffers of the gate context, the level-2 context's workspace and the lent stream"""
    import thfhe
    d = devs("SK-128")
    S, c, m, ck, ck2 = d.S, d.case, d.m, d.ck, d.ck2
    # 1. one rotation, 24 bits
    first = one(d, c["recs"][:24], 3)
    assert np.array_equal(first, m["rows"][:24]), ("sequence 1", differing(first, m["rows"][:24]))
    # 2. the default mode: the existing model's words
    tset, w = ck.circuit_bootstrap(c["recs"][:24], 3, return_words=True)
    tset.close()
    assert np.array_equal(w, c["rows"][:24]), ("sequence 2: default mode after one rotation", differing(w, c["rows"][:24]))
    # 3. stage B alone on two samples of the model's stage A
    pick = np.array([5, 40])
    got = ck.cb_private_keyswitch(m["lwe2_one"][pick])
    assert np.array_equal(got, m["rows"][pick]), ("sequence 3: stage B alone", differing(got, m["rows"][pick]))
    # 4. one rotation again
    again = one(d, c["recs"][:24], 3)
    assert np.array_equal(again, first), ("sequence 4: one rotation after the default mode", differing(again, first))
    # 5. a NAND layer on the gate context and a bootstrap on the level-2 key: the lent stream was handed back, the level-2 workspace is its own
    rng = np.random.default_rng(0x51E5)
    x, y = S.K.encrypt(rng.integers(0, 2, 19), 0x51E6), S.K.encrypt(rng.integers(0, 2, 19), 0x51E7)
    got, ref = ck.gates(thfhe.NAND, x, y), S.orc.gates(O.NAND, x, y)
    assert np.array_equal(got, ref), ("sequence 5: 19 NAND gates", differing(got, ref))
    x2 = c["recs"][[7, 30]]
    got = ck2.bootstrap(x2)
    ref = np.stack([S.orc2.keyswitch(S.orc2.bootstrap_wo_keyswitch(v, thfhe.MU8_64)) for v in x2])
    assert np.array_equal(got, ref), ("sequence 5: level-2 bootstrap", differing(got, ref))
    # 6. one rotation again
    again = one(d, c["recs"][:24], 3)
    assert np.array_equal(again, first), ("sequence 6: one rotation after gates and a level-2 bootstrap", differing(again, first))


# ---- boundaries ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", SETS)
def test_257_bits_last_workgroup_of_the_pair_kernel_holds_one_job(devs, name):
    """ONE launch of 257 rotations: 129 workgroups of the pair kernel, the last with one job.  Stage B gets 771 (l = 3) / 514 (l = 2) inputs."""
    d = devs(name)
    l = d.S.tp.l
    bits = CC.PAIR_THRESHOLD + 1
    recs, idx = CC.drawn(d.case, bits, 0x51F0 + l)
    assert bits % 2 == 1 and bits * l == (771 if l == 3 else 514)
    assert d.ck2.rotation_kernel_name(bits) == PAIR
    assert_rows(one(d, recs, 1), d.m["rows"], idx, "%s, 257 bits, one rotation" % name)


@pytest.mark.parametrize("name", SETS)
def test_2049_bits_two_slices_and_the_spectra_across_the_boundary(devs, name):
    """slices of 2 048 + 1 bits at d = 1: the second slice's single rotation runs on the single-job kernel, and the b0 offsets of lwe, words and
    the set's spectra are all non-zero there.  The spectra, which the words do not show, are read by one lookup (d_tree = 0, d_rot = 1) on the
    samples on both sides of the boundary."""
    from thfhe import lut
    d = devs(name)
    S, c, m, ck, ck2 = d.S, d.case, d.m, d.ck, d.ck2
    l = S.tp.l
    bits = CC.SLICE_BITS + 1
    recs, idx = CC.drawn(c, bits, 0x51F8 + l)
    assert ck2.rotation_kernel_name(CC.SLICE_BITS) == PAIR and ck2.rotation_kernel_name(1) == SINGLE
    tset, words = ck.circuit_bootstrap(recs, 1, return_words=True, one_rotation=True)
    try:
        assert (tset.count, tset.d) == (bits, 1)
        assert_rows(words, m["rows"], idx, "%s, 2049 bits, one rotation" % name)
        first = CC.SLICE_BITS - 2                                       # samples 2046, 2047 | 2048
        got = ck.lhe_lookup(tset, m["tab2"], d_tree=0, d_rot=1, first=first, count=3)
        with ck.tgsw_set(words[first:], 1) as ts:
            same = ck.lhe_lookup(ts, m["tab2"], d_tree=0, d_rot=1)
    finally:
        tset.close()
    assert np.array_equal(got, same), differing(got, same)
    tail = idx[first:]
    Cs = m["rows"][tail].reshape(3, 1, 2 * l, 2, N)
    ref = np.stack([LR.lookup(S.orc, Cs[s], None, m["tab2"], 0, 1, 1) for s in range(3)])
    assert np.array_equal(got, ref), differing(got, ref)
    assert np.array_equal(lut.decode(S.K.phase(got).reshape(3), CC.P_OUT), m["table2"][c["bits"][tail]])
