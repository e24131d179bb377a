"""The private key switch of circuit bootstrapping on the MI355X, stage B alone (pytest -m gpu): random words for key and
inputs (no valid key is needed: every word is an exact integer), every output word equal to the model of tests/cb_reference.py, no tolerance.
Level-1 shapes (l, Bgbit) = (3, 7) and (2, 10); input dimensions D = 1, 64, 130 and 2048; digit shapes (t, basebit) = (1, 1), (7, 4), (8, 4),
(10, 3), (4, 8); batch sizes 1, around the threshold between the plain and the matrix-core kernel, and one sample more than a whole 256-input tile
of the matrix-core kernel.  At every shape both kernels are driven (thfhe_cb_set_batch_threshold) and compared with each other and with the model,
and the library's own choice once more.  D = 2048 takes one digit shape per batch size, so that the file stays in seconds.  The model of a batch is
computed once, at the largest size: inputs are independent, so the smaller batches are its prefixes."""
import numpy as np
import pytest

import cb_reference as CB
from support import N, differing, shape_env

pytestmark = pytest.mark.gpu

LEVEL1 = [(24, 3, 7, 8, 2), (24, 2, 10, 8, 2)]            # support.shape_env shapes: l = 3 and l = 2
DIGITS = [(1, 1), (7, 4), (8, 4), (10, 3), (4, 8)]
PLAIN, MFMA, AUTO = 1 << 40, 1, 0                          # batch thresholds that force a kernel; 0: the library's default


@pytest.fixture(scope="module")
def env(O):
    yield from shape_env(O)


def rand_words(rng, *shape):
    return np.frombuffer(rng.bytes(4 * int(np.prod(shape))), np.int32).reshape(shape)


def counts(l):
    """five batch sizes in samples: 1, the threshold - 1, the threshold, the threshold + 1 (the threshold counts inputs = samples x l: the first
    sample count that reaches it, and its neighbours; with the measured threshold of 3 inputs, l = 2 has 2 inputs below it and 4 above, l = 3
    starts on it) and one sample past a 256-input tile of the matrix-core kernel.  Sizes below 1 or equal to an earlier one are moved up."""
    import thfhe
    c = -(-thfhe.CB_BATCH_MIN_INPUTS // l)
    out = []
    for v in (1, c - 1, c, c + 1, -(-256 // l) + 1):
        v = max(v, 1)
        while v in out:
            v += 1
        out.append(v)
    return out


def run_all(ck, lwe2, want, what):
    got = {}
    for name, thr in (("plain", PLAIN), ("mfma", MFMA), ("auto", AUTO)):
        ck.cb_set_batch_threshold(thr)
        got[name] = ck.cb_private_keyswitch(lwe2)
    assert np.array_equal(got["plain"], want), (what, "plain", differing(got["plain"], want))
    assert np.array_equal(got["mfma"], want), (what, "mfma", differing(got["mfma"], want))
    assert np.array_equal(got["mfma"], got["plain"]) and np.array_equal(got["auto"], want), (what, "auto")


@pytest.mark.parametrize("t,basebit", DIGITS, ids=lambda v: str(v))
@pytest.mark.parametrize("D", [1, 64, 130])
@pytest.mark.parametrize("shape", LEVEL1, ids=lambda s: "l%d" % s[1])
def test_every_word_small_dimensions(env, shape, D, t, basebit):
    l, ck = shape[1], env(shape)[3]
    rng = np.random.default_rng(1000 * D + 10 * t + l)
    key = rand_words(rng, 2, D, t, 2, N)
    ck.cb_key_set(None, key, t, basebit)
    cs = counts(l)
    lwe2 = rand_words(rng, max(cs), l, D + 1)
    want = CB.private_keyswitch(key, lwe2, l, t, basebit)
    for c in cs:
        run_all(ck, lwe2[:c], want[:c], (l, D, t, basebit, c))


@pytest.mark.parametrize("which", range(5))
@pytest.mark.parametrize("shape", LEVEL1, ids=lambda s: "l%d" % s[1])
def test_every_word_full_dimension(env, shape, which):
    # D = 2048: batch size `which` with digit shape `which`; the large batch goes with the cheapest digits
    l, ck = shape[1], env(shape)[3]
    t, basebit = [(7, 4), (8, 4), (10, 3), (4, 8), (1, 1)][which]
    c = counts(l)[which]
    rng = np.random.default_rng(2048 + 10 * which + l)
    key = rand_words(rng, 2, 2048, t, 2, N)
    ck.cb_key_set(None, key, t, basebit)
    lwe2 = rand_words(rng, c, l, 2049)
    run_all(ck, lwe2, CB.private_keyswitch(key, lwe2, l, t, basebit), (l, 2048, t, basebit, c))


@pytest.mark.parametrize("t,basebit", [(7, 4), (4, 8)])
def test_extreme_inputs(env, t, basebit):
    """every mask word 0x7FFFFFFF, every mask word 0x80000000, and the all-carry word (every digit -B/2) on key words 0x7FFFFFFF (f = 0) and
    0x80000000 (f = 1), whose top byte plane is -128 everywhere: the int32 partial sums of the matrix-core kernel stand at their bound
    D t 2^(basebit-1) 128"""
    shape = LEVEL1[0]
    l, ck, D = shape[1], env(shape)[3], 2048
    B = 1 << basebit
    key = np.empty((2, D, t, 2, N), np.int32)
    key[0], key[1] = 0x7FFFFFFF, -2**31
    ck.cb_key_set(None, key, t, basebit)
    carry = (-sum((B // 2) << (32 - (p + 1) * basebit) for p in range(t))) & 0xFFFFFFFF
    lwe2 = np.empty((3, l, D + 1), np.int64)
    lwe2[0], lwe2[1], lwe2[2] = 0x7FFFFFFF, 0x80000000, carry
    lwe2[:, :, D] = [[0x12345678, 0x7FFFFFFF, 0x80000000][:l]] * 3
    lwe2 = lwe2.astype(np.uint32).view(np.int32)
    assert np.all(CB.digits(lwe2[2, :, :D], t, basebit) == -(B // 2))
    bound = D * t * (B // 2) * 128
    assert CB.plane_sums(key, lwe2, l, t, basebit, [0, N]) == bound and bound < 2**31
    run_all(ck, lwe2, CB.private_keyswitch(key, lwe2, l, t, basebit), ("extreme", t, basebit))
    ck.cb_set_batch_threshold(AUTO)


def test_a_second_key_replaces_the_first_and_calls_without_a_key_fail(O):
    import thfhe
    p = O.make_params("SK-128", n=8)
    K = O.SKKeys(p, 91, 2.0**-25, 2.0**-15)
    ck = thfhe.CloudKey(thfhe.make_params("SK-128", n=8), K.bk, K.ksk, device=0)
    try:
        with pytest.raises(thfhe.ThfheError):
            ck.cb_private_keyswitch(np.zeros((1, 3, 5), np.int32))
        rng = np.random.default_rng(92)
        for D, t, basebit in ((4, 7, 4), (9, 3, 5)):
            key = rand_words(rng, 2, D, t, 2, N)
            ck.cb_key_set(None, key, t, basebit)
            lwe2 = rand_words(rng, 2, 3, D + 1)
            assert np.array_equal(ck.cb_private_keyswitch(lwe2), CB.private_keyswitch(key, lwe2, 3, t, basebit))
        with pytest.raises(ValueError):
            ck.cb_private_keyswitch(np.zeros((1, 3, 5), np.int32))    # records of the first key's dimension
    finally:
        ck.close()
