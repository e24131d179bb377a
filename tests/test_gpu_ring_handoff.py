"""The ring kernel's key hand-off (torus-fhe_amd/csrc/thfhe_ring_schedule.h) on the MI355X (pytest -m gpu): three
barriers per digit row, the row's fourth chunk lent a slot by transpose buffer 0.  Both ring shapes (eight and four waves), every output word
against the oracle, and every launch repeated on the same inputs: the two outputs must be the same bytes -- a hand-off race shows as a
run-to-run difference before it shows as a wrong word.  The host replay of the schedule is tests/test_ring_schedule.py.

SK-128 with a short mask (n = 4 or 8, the recipe of test_gpu_fold_ring.py) keeps an oracle rotation at milliseconds; at n <= 3 the prologue,
the end-of-stream clamp and the last row's borrowed chunk all lie within the first few chunks of the stream."""
import numpy as np
import pytest

import lut_reference as R
import mv_lut_reference as MV
import tree_lut_reference as TR
from support import KERNELS, differing, pmap, thresholds, words

pytestmark = pytest.mark.gpu

RING = [k for k in KERNELS if k[0] in ("ring8", "ring4")]   # W = 8 and W = 4
MU = 1 << 29


def setup(O, seed, **over):
    """(params, oracle, CloudKey) of SK-128 with the given fields replaced, random keys"""
    import thfhe
    kw = dict(O.PARAM_SETS["SK-128"], **over)
    p = O.make_params(**kw)
    K = O.SKKeys(p, seed, 2.0**-25, 2.0**-15)
    return p, O.Oracle(p, K.bk, K.ksk), thfhe.CloudKey(thfhe.make_params(**kw), K.bk, K.ksk, device=0)


def twice_on_both_shapes(ck, l, jobs, launch, ref):
    """launch() on the eight- and the four-wave ring, twice each: byte-identical outputs, every word equal to ref"""
    for _, coop, ring4, name in RING:
        with thresholds(ck, coop, ring4):
            assert ck.rotation_kernel_name(jobs) == name.format(l=l)
            first, second = launch(), launch()
            assert first.tobytes() == second.tobytes(), (name, jobs, "two launches differ at", differing(first, second))
            assert np.array_equal(first, ref), (name, jobs, differing(first, ref))


# l = 2 and 3 with the digit sizes test_gpu_fold_ring.py gives them; l = 1 and 4 (not in that file) with the Bgbit = 8 of support.SHAPES
@pytest.mark.parametrize("l, Bgbit", [(1, 8), (2, 10), (3, 7), (3, 10), (4, 8)], ids=["l1-Bg8", "l2-Bg10", "l3-Bg7", "l3-Bg10", "l4-Bg8"])
def test_job_counts(O, l, Bgbit):
    # 1, 7: one partly filled workgroup (waves without a job still bring their slices); 8: full; 9 and 17: a last workgroup holding one job
    p, orc, ck = setup(O, 0x4A0 + 16 * l + Bgbit, n=4, l=l, Bgbit=Bgbit)
    try:
        xs = words(np.random.default_rng(0x4B0 + l), 17, p.n + 1)
        ref = np.stack(pmap(lambda x: orc.bootstrap_wo_keyswitch(x, MU), xs))
        for jobs in (1, 7, 8, 9, 17):
            twice_on_both_shapes(ck, l, jobs, lambda: ck.bootstrap_wo_keyswitch(xs[:jobs], MU), ref[:jobs])
    finally:
        ck.close()


def test_zero_mask_words_beside_working_neighbours(O):
    # n = 8, one eight-wave workgroup (two four-wave ones): job j skips CMux j (and job 1 also CMux 5 .. 7, job 4 also CMux 0 .. 2) while its
    # neighbours work at that index; job 6 skips every CMux.  A skipping wave keeps issuing its slices and keeps every barrier.
    p, orc, ck = setup(O, 0x4C0, n=8)
    try:
        xs = words(np.random.default_rng(0x4C1), 8, p.n + 1)
        zero = {j: {j} for j in range(8)}
        zero[1] |= {5, 6, 7}
        zero[4] |= {0, 1, 2}
        zero[6] = set(range(p.n))
        for j in range(8):
            for i in range(p.n):
                bar = O.lib().oracle_modswitch(int(xs[j, i]), p.N) % (2 * p.N)
                if i in zero[j]:
                    xs[j, i] = 0
                elif bar == 0:
                    xs[j, i] = 1 << 21        # mod-switches to 1
                assert (O.lib().oracle_modswitch(int(xs[j, i]), p.N) % (2 * p.N) == 0) == (i in zero[j])
        ref = np.stack(pmap(lambda x: orc.bootstrap_wo_keyswitch(x, MU), xs))
        twice_on_both_shapes(ck, p.l, 8, lambda: ck.bootstrap_wo_keyswitch(xs, MU), ref)
    finally:
        ck.close()


@pytest.mark.parametrize("n", [1, 2, 3])      # n = 1 is the smallest mask a context accepts
def test_short_key_streams(O, n):
    # 9 jobs: a full workgroup and a single job; the stream is 24 n chunks long
    p, orc, ck = setup(O, 0x4D0 + n, n=n)
    try:
        xs = words(np.random.default_rng(0x4D8 + n), 9, p.n + 1)
        ref = np.stack(pmap(lambda x: orc.bootstrap_wo_keyswitch(x, MU), xs))
        twice_on_both_shapes(ck, p.l, 9, lambda: ck.bootstrap_wo_keyswitch(xs, MU), ref)
    finally:
        ck.close()


@pytest.fixture(scope="module")
def lut_env(O):
    p, orc, ck = setup(O, 0x4E0, n=4)
    yield p, orc, ck, words(np.random.default_rng(0x4E1), 9, p.n + 1)
    ck.close()


def test_lut_instantiation_theta4(lut_env):
    p, orc, ck, xs = lut_env
    tv = words(np.random.default_rng(0x4E2), p.N)
    ref = np.stack(pmap(lambda x: R.lut_bootstrap(orc, [x], (1,), 0, tv, 4, keyswitch=False), xs))
    twice_on_both_shapes(ck, p.l, len(xs), lambda: ck.lut_bootstrap_wo_keyswitch(tv, xs, theta=4), ref)


def test_encrypted_table_instantiation(lut_env):
    p, orc, ck, xs = lut_env
    rng = np.random.default_rng(0x4E3)
    tv_a, tv_b = words(rng, 3, p.N), words(rng, 3, p.N)
    idx = (np.arange(len(xs)) % 3).astype(np.int32)
    ref = np.stack(pmap(lambda g: TR.lut_enc(orc, [xs[g]], (1,), 0, tv_a[idx[g]], tv_b[idx[g]], 2, keyswitch=False), range(len(xs))))
    twice_on_both_shapes(ck, p.l, len(xs), lambda: ck.lut_bootstrap_enc_wo_keyswitch(tv_a, tv_b, xs, theta=2, lut_index=idx), ref)


def test_multi_value_instantiation(lut_env):
    p, orc, ck, xs = lut_env
    rng = np.random.default_rng(0x4E4)
    tv0 = words(rng, p.N)
    factors = words(rng, 2, 9, 16)            # two tables of q = 9 outputs, p = 16 taps
    idx = (np.arange(len(xs)) % 2).astype(np.int32)
    accs = pmap(lambda x: MV.rotate(orc, R.prologue([x], (1,), 0), tv0), xs)
    ref = np.stack([MV.combine(acc, factors[t], p.N) for acc, t in zip(accs, idx)])
    twice_on_both_shapes(ck, p.l, len(xs), lambda: ck.mv_lut_bootstrap_wo_keyswitch(factors, xs, tv0=tv0, table_index=idx), ref)
