"""The ring kernels' forward transform with the unmasked exchange over the phased key copy (variant "p") on the MI355X
(pytest -m gpu).  The ring kernels read the digits at nu = lane_nu(lane), leave rho^(-32) on the spectra of the lanes with bit 3 set and stream a
second key array that carries rho^(+32) there (the spectrum of X^32 b, made at context creation); the cooperative kernel keeps the plain array.  A
wrong sign, bit or rotation shows in every output word, so the cases are the kernel's instantiations and paths, small: every gadget depth at
n = 1, 2, 3, 5 on both ring shapes at every job count that leaves waves idle, a zero mask word beside working neighbours, the three lookup-table
instantiations at n = 3, the crafted CMux with every limb sum at the exactness bound, and one context whose batch is cut into an eight-wave, a
four-wave and a cooperative piece, so that its two key arrays must give the same words, on rotation amounts around the +-32 wrap of the phase.
Every output word against the exact oracle, every launch twice on the same inputs with byte-equal outputs."""
import numpy as np
import pytest

import bound_inputs as B
import lut_reference as R
import mv_lut_reference as MV
import tree_lut_reference as TR
from support import KERNELS, differing, pmap, thresholds, words
from test_gpu_ring_exchange import JOBS, MU, RING, setup, twice

pytestmark = pytest.mark.gpu

BY_ID = {k[0]: k for k in KERNELS}
WRAP_AMOUNTS = (1, 31, 32, 33, 1023, 1024, 2047)   # mod-switched mask words: below, at and above the phase 32, and the sign wraps of X^a


@pytest.mark.parametrize("n", [1, 2, 3, 5])
@pytest.mark.parametrize("l, Bgbit", [(1, 8), (2, 10), (3, 7), (4, 8)], ids=["l1", "l2", "l3", "l4"])
def test_depths_lengths_and_job_counts(O, l, Bgbit, n):
    p, orc, ck = setup(O, 0x7A00 + 16 * l + n, n=n, l=l, Bgbit=Bgbit)
    try:
        xs = words(np.random.default_rng(0x7B00 + 16 * l + n), 17, p.n + 1)
        ref = np.stack(pmap(lambda x: orc.bootstrap_wo_keyswitch(x, MU), xs))
        for shape, counts in JOBS.items():
            for jobs in counts:
                twice(ck, shape, l, jobs, lambda: ck.bootstrap_wo_keyswitch(xs[:jobs], MU), ref[:jobs])
    finally:
        ck.close()


def test_zero_mask_word_beside_working_neighbours(O):
    # n = 3, 9 jobs: job j skips CMux j mod 3 while the other waves of its workgroup stream the phased key and multiply; job 4 skips every CMux
    p, orc, ck = setup(O, 0x7C0, n=3)
    try:
        xs = words(np.random.default_rng(0x7C1), 9, p.n + 1)
        zero = {j: {j % p.n} for j in range(9)}
        zero[4] = set(range(p.n))
        for j in range(9):
            for i in range(p.n):
                bar = O.lib().oracle_modswitch(int(xs[j, i]), p.N) % (2 * p.N)
                if i in zero[j]:
                    xs[j, i] = 0
                elif bar == 0:
                    xs[j, i] = 1 << 21        # mod-switches to 1
                assert (O.lib().oracle_modswitch(int(xs[j, i]), p.N) % (2 * p.N) == 0) == (i in zero[j])
        ref = np.stack(pmap(lambda x: orc.bootstrap_wo_keyswitch(x, MU), xs))
        for shape in RING:
            twice(ck, shape, p.l, 9, lambda: ck.bootstrap_wo_keyswitch(xs, MU), ref)
    finally:
        ck.close()


@pytest.fixture(scope="module")
def lut_env(O):
    p, orc, ck = setup(O, 0x7E0, n=3)
    yield p, orc, ck, words(np.random.default_rng(0x7E1), 9, p.n + 1)
    ck.close()


def test_lut_instantiation_theta4_n3(lut_env):
    p, orc, ck, xs = lut_env
    tv = words(np.random.default_rng(0x7E2), p.N)
    ref = np.stack(pmap(lambda x: R.lut_bootstrap(orc, [x], (1,), 0, tv, 4, keyswitch=False), xs))
    for shape in RING:
        twice(ck, shape, p.l, len(xs), lambda: ck.lut_bootstrap_wo_keyswitch(tv, xs, theta=4), ref)


def test_encrypted_table_instantiation_n3(lut_env):
    p, orc, ck, xs = lut_env
    rng = np.random.default_rng(0x7E3)
    tv_a, tv_b = words(rng, 2, p.N), words(rng, 2, p.N)
    idx = (np.arange(len(xs)) % 2).astype(np.int32)
    ref = np.stack(pmap(lambda g: TR.lut_enc(orc, [xs[g]], (1,), 0, tv_a[idx[g]], tv_b[idx[g]], 2, keyswitch=False), range(len(xs))))
    for shape in RING:
        twice(ck, shape, p.l, len(xs), lambda: ck.lut_bootstrap_enc_wo_keyswitch(tv_a, tv_b, xs, theta=2, lut_index=idx), ref)


def test_multi_value_instantiation_n3(lut_env):
    p, orc, ck, xs = lut_env
    rng = np.random.default_rng(0x7E4)
    tv0 = words(rng, p.N)
    factors = words(rng, 2, 9, 16)            # two tables of q = 9 outputs, p = 16 taps
    idx = (np.arange(len(xs)) % 2).astype(np.int32)
    accs = pmap(lambda x: MV.rotate(orc, R.prologue([x], (1,), 0), tv0), xs)
    ref = np.stack([MV.combine(acc, factors[t], p.N) for acc, t in zip(accs, idx)])
    for shape in RING:
        twice(ck, shape, p.l, len(xs), lambda: ck.mv_lut_bootstrap_wo_keyswitch(factors, xs, tv0=tv0, table_index=idx), ref)


def test_both_shapes_at_the_bound(O):
    # the largest shape context creation admits (l = 3, Bgbit = 10): step 1 carries -Bg/2 in all six rows against key words 0x7FFF8000 -- both limbs of
    # every key word at 2^15, negated where the phased copy's rotation wraps -- and every limb sum of that CMux is 2l N 2^(Bgbit-1) 2^15
    import thfhe
    l, Bgbit = 3, 10
    kw = dict(O.PARAM_SETS["SK-128"], n=4, l=l, Bgbit=Bgbit)
    p = O.make_params(**kw)
    K = O.SKKeys(p, 0x7F3, 2.0**-25, 2.0**-15)
    bk, x, mu, step = B.sk_case(p, K.bk, True)
    orc = O.Oracle(p, bk, K.ksk)
    assert B.sk_reached(orc, p, bk, x, mu, step) == B.bound(2 * l, p.N, Bgbit)
    ref = np.tile(orc.bootstrap_wo_keyswitch(x, mu), (9, 1))
    xs = np.tile(x, (9, 1))
    ck = thfhe.CloudKey(thfhe.make_params(**kw), bk, K.ksk, device=0)
    try:
        for shape in RING:
            twice(ck, shape, l, 9, lambda: ck.bootstrap_wo_keyswitch(xs, mu), ref)
    finally:
        ck.close()


def test_one_context_split_over_both_key_arrays(O):
    # The launch rule cuts whole rounds of 2 048 jobs for the eight-wave kernel before anything else, so the smallest batch that one context runs on
    # all three kernels is 2 048 + r; with both thresholds at 6 and r = 12 it is ring8 (2 048) | ring4 (6) | cooperative (6).  Few DISTINCT samples:
    # a dozen, repeated, so that each of them runs on the phased array (both ring shapes) and on the plain one (cooperative) inside ONE call and all
    # copies must agree with the oracle.  n = 8: every sample carries the seven rotation amounts around the phase's wrap, in a rotated order.
    p, orc, ck = setup(O, 0x7D0, n=8)
    try:
        D = 12
        xs = words(np.random.default_rng(0x7D1), D, p.n + 1)
        for j in range(D):
            for t, abar in enumerate(WRAP_AMOUNTS):
                i = (j + t) % p.n
                xs[j, i] = np.array(abar << 21, np.uint32).astype(np.int32)
                assert O.lib().oracle_modswitch(int(xs[j, i]), p.N) % (2 * p.N) == abar
        ref = np.stack(pmap(lambda x: orc.bootstrap_wo_keyswitch(x, MU), xs))
        _, coop, ring4, _ = BY_ID["split"]
        assert (coop, ring4) == (6, 6)
        idx = np.concatenate([np.arange(2048) % D, np.arange(6), np.arange(6)])   # ring8: all twelve; ring4 and cooperative: samples 0 .. 5 each
        with thresholds(ck, coop, ring4):
            # the pieces by the rule's own answers: the whole batch starts on the eight-wave kernel, its remainder of 12 on the four-wave kernel,
            # and what that remainder leaves (6 <= the cooperative threshold) on the cooperative one
            assert ck.rotation_kernel_name(2048 + 12) == BY_ID["ring8"][3].format(l=p.l)
            assert ck.rotation_kernel_name(12) == BY_ID["ring4"][3].format(l=p.l)
            assert ck.rotation_kernel_name(6) == BY_ID["coop"][3].format(l=p.l)
            first, second = (ck.bootstrap_wo_keyswitch(xs[idx], MU) for _ in range(2))
        assert first.tobytes() == second.tobytes(), differing(first, second)
        assert np.array_equal(first, ref[idx]), differing(first, ref[idx])
        # and each kernel alone on the twelve samples
        for shape in ("ring8", "ring4", "coop"):
            _, c, r4, name = BY_ID[shape]
            with thresholds(ck, c, r4):
                assert ck.rotation_kernel_name(D) == name.format(l=p.l)
                a, b = (ck.bootstrap_wo_keyswitch(xs, MU) for _ in range(2))
            assert a.tobytes() == b.tobytes(), (shape, differing(a, b))
            assert np.array_equal(a, ref), (shape, differing(a, ref))
    finally:
        ck.close()
