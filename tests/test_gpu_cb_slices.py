"""Circuit bootstrapping across its slice and launch boundaries on the MI355X (pytest -m gpu).  tests/test_gpu_cb.py and
tests/test_gpu_cb_shapes.py stay inside the first iteration of every batch-splitting loop; here every loop takes a second turn, and every word
is compared with the model, no tolerance:

  cb_fill               slices of 2 048 bits: 2 049 bits are two slices, at d = 3 with the boundary inside a sample
  cb_enqueue            launches of 4096 // l * l inputs: 4 095 + 3 and 4 095 + 2 049 at l = 3, exactly 4 096 at l = 2
  cb_private_keyswitch  host slices of 2048 // l samples: 682, 682 + 1, 682 + 682 + 1 at l = 3; 1 024, 1 024 + 1 at l = 2
  stage B kernels       nsplit == 1 over a three-stage loop (8 tiles of 256 inputs) on the matrix cores, one un-split range on the plain kernel
  stage A               more than 256 jobs: kms_tlev_rotate_pair_kernel at an odd job count
  one long-lived pair of contexts: large and small calls, stage B alone, the level-2 key used directly and a refused call in between

The boundaries are tests/cb_cases.BOUNDARIES, which tests/test_cb_host.py checks against the text of the sources.  A large batch is a random draw
(cb_cases.drawn) from the 48 (SK-80: 24) NAND-output records whose rows the model already holds: stages A, B and C are deterministic functions of
one record, so the model of the batch is the same draw from case["rows"].  Words are compared in chunks of 256 bits, so that no second array of
the size of a call's output (up to 100 MB) is made; a mismatch reports the first differing bit."""
import time

import numpy as np
import pytest

import cb_cases as CC
import cb_reference as CB
import lhe_reference as LR
from support import N, differing, shape_env
from test_gpu_cb import Dev
from test_gpu_cb_shapes import AUTO, LEVEL1, MFMA, PLAIN, rand_words

pytestmark = pytest.mark.gpu

PAIR, SINGLE = "kms_tlev_rotate_pair_kernel", "kms_tlev_rotate_kernel"
CHUNK = 256
KERNELS = (("plain", PLAIN), ("mfma", MFMA), ("auto", AUTO))


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


def assert_same(got, want_of, count, what):
    """got[b] == want_of(b0, b1)[b - b0] for every b < count, chunk by chunk; the message names the first differing bit (or sample)"""
    assert got.shape[0] == count, (what, got.shape, count)
    for b0 in range(0, count, CHUNK):
        g, w = got[b0:b0 + CHUNK], want_of(b0, min(b0 + CHUNK, count))
        assert g.shape == w.shape and g.dtype == w.dtype, (what, g.shape, g.dtype, w.shape, w.dtype)
        if not np.array_equal(g, w):
            bad = differing(g, w)
            raise AssertionError("%s: first difference at index %d of %d; (index - %d, row, part, word) of the first mismatches: %s" % (
                what, b0 + bad[0][0], count, b0, bad))


def assert_rows(words, rows, idx, what):
    """the words of a call on a drawn batch against the same draw from the model's rows"""
    assert words.shape == (len(idx),) + rows.shape[1:], (what, words.shape)
    assert_same(words, lambda b0, b1: rows[idx[b0:b1]], len(idx), what)


def assert_equal_runs(a, b, what):
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert_same(a, lambda b0, b1: b[b0:b1], a.shape[0], what)


def boot(dv, recs, d, thr=AUTO, what=""):
    """circuit_bootstrap with the stage-B kernel chosen by `thr`, the default restored; prints the call's wall time"""
    dv.ck.cb_set_batch_threshold(thr)
    try:
        t = time.perf_counter()
        tset, words = dv.ck.circuit_bootstrap(recs, d, return_words=True)
        print("\n%s: %d bits at d = %d, threshold %d: %.0f ms" % (what, len(recs), d, thr, 1e3 * (time.perf_counter() - t)))
    finally:
        dv.ck.cb_set_batch_threshold(AUTO)
    return tset, words


def boot_words(dv, recs, d, thr=AUTO, what=""):
    tset, words = boot(dv, recs, d, thr, what)
    tset.close()
    return words


# ---- SK-128: l = 3, pool 48 --------------------------------------------------------------------------------------------------------------

def test_257_bits_run_stage_a_on_the_pair_kernel_with_an_odd_job_count(sk128):
    """257 jobs per level-2 rotation launch: 129 workgroups of the pair kernel, the last with one job.  Stage B gets 771 inputs: 4 tiles, the last
    with 3 inputs.  The single-job kernel on the same batch gives the same words."""
    c, ck2 = sk128.case, sk128.ck2
    bits = CC.PAIR_THRESHOLD + 1
    recs, idx = CC.drawn(c, bits, 0x51C0)
    assert bits % 2 == 1 and bits * sk128.S.tp.l == 3 * CC.TILE_INPUTS + 3
    assert ck2.rotation_kernel_name(bits) == PAIR
    words = boot_words(sk128, recs, 1, what="257 bits, pair kernel")
    assert_rows(words, c["rows"], idx, "257 bits, pair kernel")
    ck2.set_pair_threshold(1 << 20)
    try:
        assert ck2.rotation_kernel_name(bits) == SINGLE
        single = boot_words(sk128, recs, 1, what="257 bits, single-job kernel")
    finally:
        ck2.set_pair_threshold(CC.PAIR_THRESHOLD)
    assert ck2.rotation_kernel_name(bits) == PAIR and ck2.rotation_kernel_name(bits - 1) == SINGLE
    assert_equal_runs(single, words, "257 bits, single-job kernel against the pair kernel")


def test_1366_bits_d2_two_launches_of_stage_b_on_every_kernel(sk128):
    """one slice of 4 098 inputs: launches of 4 095 + 3, the second at an input offset, into the digit matrix the first one used"""
    c, l = sk128.case, sk128.S.tp.l
    recs, idx = CC.drawn(c, 1366, 0x51C1)
    per_launch = CC.LAUNCH_INPUTS // l * l
    assert 1366 <= CC.SLICE_BITS and 1366 % 2 == 0 and 1366 * l == per_launch + 3 and per_launch == 4095
    first = None
    for name, thr in KERNELS:
        words = boot_words(sk128, recs, 2, thr, "1366 bits " + name)
        assert_rows(words, c["rows"], idx, "1366 bits, d = 2, " + name)
        if first is None:
            first = words
        else:
            assert_equal_runs(words, first, "1366 bits, d = 2, %s against plain" % name)


def test_2049_bits_d3_slice_boundary_inside_the_last_sample(sk128):
    """slices of 2 048 + 1 bits; sample 682 holds bits 2 046 .. 2 048, so the boundary falls inside it.  The first slice is stage B launches of
    4 095 + 2 049 inputs, the second one level-2 job per rotation and 3 inputs.  The spectra, which the words do not show, are read by a lookup on
    samples 680 .. 682."""
    from thfhe import lut
    S, c, ck, ck2 = sk128.S, sk128.case, sk128.ck, sk128.ck2
    l = S.tp.l
    bits = CC.SLICE_BITS + 1
    recs, idx = CC.drawn(c, bits, 0x51C2, pool=24)             # the lookup's records: bits 0 .. 23 of the case, whose table the model has
    assert bits % 3 == 0 and 3 * 682 < CC.SLICE_BITS < 3 * 683 == bits
    assert CC.SLICE_BITS * l == CC.LAUNCH_INPUTS // l * l + 2049
    assert ck2.rotation_kernel_name(CC.SLICE_BITS) == PAIR and ck2.rotation_kernel_name(1) == SINGLE
    tset, words = boot(sk128, recs, 3, what="2049 bits")
    try:
        assert (tset.count, tset.d) == (683, 3)
        assert_rows(words, c["rows"], idx, "2049 bits, d = 3")
        got = ck.lhe_lookup(tset, c["tab"], d_tree=1, d_rot=2, first=680, count=3)
        with ck.tgsw_set(words[3 * 680:], 3) as ts:
            same = ck.lhe_lookup(ts, c["tab"], d_tree=1, d_rot=2)
    finally:
        tset.close()
    assert np.array_equal(got, same), differing(got, same)
    tail = idx[3 * 680:]
    Cs = c["rows"][tail].reshape(3, 3, 2 * l, 2, N)
    ref = np.stack([LR.lookup(S.orc, Cs[s], None, c["tab"], 1, 2, 1) for s in range(3)])
    assert np.array_equal(got, ref), differing(got, ref)
    address = (c["bits"][tail].reshape(3, 3).astype(np.int64) << np.arange(3)).sum(axis=1)     # low bit first (lut.lhe_address_bits)
    assert np.array_equal(lut.decode(S.K.phase(got).reshape(3), CC.P_OUT), c["table"][address])


# ---- SK-80: l = 2, pool 24 ---------------------------------------------------------------------------------------------------------------

def test_sk80_2049_bits_full_slice_is_one_launch_of_exactly_4096_inputs(sk80):
    """l = 2: the full slice is one launch of 4 096 inputs (16 full tiles, the stages of a workgroup not split), the second slice holds one bit"""
    c, l = sk80.case, sk80.S.tp.l
    bits = CC.SLICE_BITS + 1
    recs, idx = CC.drawn(c, bits, 0x51C3)
    assert len(c["recs"]) == 24 and CC.SLICE_BITS * l == CC.LAUNCH_INPUTS == CC.LAUNCH_INPUTS // l * l == 16 * CC.TILE_INPUTS
    auto = boot_words(sk80, recs, 1, AUTO, "SK-80 2049 bits auto")
    assert_rows(auto, c["rows"], idx, "SK-80, 2049 bits, default threshold")
    plain = boot_words(sk80, recs, 1, PLAIN, "SK-80 2049 bits plain")
    assert_rows(plain, c["rows"], idx, "SK-80, 2049 bits, plain kernel")
    assert_equal_runs(plain, auto, "SK-80, 2049 bits, plain against the default")


# ---- stage B alone on random words ---------------------------------------------------------------------------------------------------------

STAGE_B_D, STAGE_B_T, STAGE_B_BASEBIT = 43, 7, 4          # K = 301 pairs: three stages of 128, the last padded
STAGE_B_COUNTS = {3: (682, 683, 1365), 2: (1024, 1025)}   # samples: one host slice, one more, (l = 3) two and one more


@pytest.fixture(scope="module")
def env(O):
    yield from shape_env(O)


@pytest.fixture(scope="module")
def stage_b():
    """l -> (key, lwe2, model rows) at the largest count, computed once: inputs are independent, the smaller batches are prefixes"""
    made = {}

    def get(l):
        if l not in made:
            D, t, basebit = STAGE_B_D, STAGE_B_T, STAGE_B_BASEBIT
            rng = np.random.default_rng(0x51CB + l)
            key = rand_words(rng, 2, D, t, 2, N)
            lwe2 = rand_words(rng, max(STAGE_B_COUNTS[l]), l, D + 1)
            made[l] = key, lwe2, CB.private_keyswitch(key, lwe2, l, t, basebit)
        return made[l]
    return get


@pytest.mark.parametrize("l,count", [(l, c) for l in (3, 2) for c in STAGE_B_COUNTS[l]], ids=lambda v: str(v))
def test_stage_b_host_slices_and_unsplit_kernels(env, stage_b, l, count):
    shape = next(s for s in LEVEL1 if s[1] == l)
    ck = env(shape)[3]
    key, lwe2, want = stage_b(l)
    per_slice = max(1, CC.HOST_SLICE_INPUTS // l)
    assert per_slice == (682 if l == 3 else 1024) and count in (per_slice, per_slice + 1, 2 * per_slice + 1)
    assert -(-STAGE_B_D * STAGE_B_T // 128) == 3 and STAGE_B_D * STAGE_B_T % 128
    assert -(-per_slice * l // CC.TILE_INPUTS) == 8           # 8 tiles x 128 word tiles = 1 024 workgroups: the stages are not split
    ck.cb_key_set(None, key, STAGE_B_T, STAGE_B_BASEBIT)
    try:
        first = None
        for name, thr in KERNELS:
            ck.cb_set_batch_threshold(thr)
            got = ck.cb_private_keyswitch(lwe2[:count])
            assert_same(got, lambda s0, s1: want[s0:s1], count, "stage B alone, l = %d, %d samples, %s" % (l, count, name))
            if first is None:
                first = got
            else:
                assert_equal_runs(got, first, "stage B alone, l = %d, %d samples, %s against plain" % (l, count, name))
    finally:
        ck.cb_set_batch_threshold(AUTO)


# ---- one long-lived pair of contexts -------------------------------------------------------------------------------------------------------

def test_long_lived_contexts_share_buffers_and_stream(O, sk128):
    """large and small bootstraps, stage B alone, the level-2 key used directly, gates and a refused call on ONE pair of contexts: circuit_bootstrap
    and cb_private_keyswitch share grow-only buffers, and circuit_bootstrap lends the gate context's stream to the level-2 context"""
    import thfhe
    S, c, ck, ck2 = sk128.S, sk128.case, sk128.ck, sk128.ck2
    l, rows = S.tp.l, c["rows"]
    # 1. two slices
    recs, idx = CC.drawn(c, CC.SLICE_BITS + 1, 0x51D0)
    assert_rows(boot_words(sk128, recs, 1, what="sequence 1"), rows, idx, "sequence 1: 2049 bits")
    # 2. stage B alone on two samples of the model's stage A (the key is the real D = 2048 key): rows 5 and 40 of the pool
    pick = np.array([5, 40])
    lwe2 = CB.stage_a(S.orc2, c["recs"][pick], l, S.tp.Bgbit)
    got = ck.cb_private_keyswitch(lwe2)
    assert np.array_equal(got, rows[pick]), ("sequence 2: stage B alone after a large bootstrap", differing(got, rows[pick]))
    # 3. a small bootstrap after the large one
    three = np.array([47, 0, 23])
    w3 = boot_words(sk128, c["recs"][three], 3, what="sequence 3")
    assert np.array_equal(w3, rows[three]), ("sequence 3: 3 bits", differing(w3, rows[three]))
    # 4. the level-2 key directly: the lent stream was handed back
    x2 = c["recs"][[7, 30]]
    got = ck2.bootstrap(x2)
    ref = np.stack([S.orc2.keyswitch(S.orc2.bootstrap_wo_keyswitch(x, thfhe.MU8_64)) for x in x2])
    assert np.array_equal(got, ref), ("sequence 4: level-2 bootstrap", differing(got, ref))
    # 5. gates on the gate context
    rng = np.random.default_rng(0x51D5)
    x, y = S.K.encrypt(rng.integers(0, 2, 19), 0x51D6), S.K.encrypt(rng.integers(0, 2, 19), 0x51D7)
    got, ref = ck.gates(thfhe.NAND, x, y), S.orc.gates(O.NAND, x, y)
    assert np.array_equal(got, ref), ("sequence 5: 19 NAND gates", differing(got, ref))
    # 6. a large call again, two launches of stage B
    recs, idx = CC.drawn(c, 1366, 0x51D8)
    assert_rows(boot_words(sk128, recs, 2, what="sequence 6"), rows, idx, "sequence 6: 1366 bits")
    # 7. the 3-bit call again
    again = boot_words(sk128, c["recs"][three], 3, what="sequence 7")
    assert np.array_equal(again, w3), ("sequence 7: 3 bits after 1366", differing(again, w3))
    # 8. a call the host refuses (d = 17) leaves no trace
    with pytest.raises(thfhe.ThfheError, match="d must be"):
        ck.circuit_bootstrap(c["recs"][:17], 17)
    after = boot_words(sk128, c["recs"][three], 3, what="sequence 8")
    assert np.array_equal(after, w3), ("sequence 8: 3 bits after a refused call", differing(after, w3))
