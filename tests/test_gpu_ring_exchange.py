"""The ring kernel's lane exchange of variant "x"  on the MI355X (pytest -m gpu).  Past the forward exchange a lane stands
for the position nu = lane_nu(lane): it reads the key at nu, takes the roots of nu, and after the inverse's unmasked exchange (flipped names on the
lanes with bit 3 set) updates the accumulator coefficients nu + 64 m.  A wrong lane map, sign or root shows in every output word, so the cases are
the kernel's instantiations and paths, small: every gadget depth at n = 1, 2, 3, 5 on both ring shapes at every job count that leaves waves idle,
a zero mask word beside working neighbours, the three lookup-table instantiations at n = 3, and the crafted CMux with every limb sum at the
exactness bound.  Every output word against the exact oracle, every launch twice on the same inputs with byte-equal outputs."""
import numpy as np
import pytest

import bound_inputs as B
import lut_reference as R
import mv_lut_reference as MV
import tree_lut_reference as TR
from support import KERNELS, differing, pmap, thresholds, words

pytestmark = pytest.mark.gpu

RING = {k[0]: k for k in KERNELS if k[0] in ("ring8", "ring4")}
JOBS = {"ring8": (1, 7, 8, 9, 17), "ring4": (1, 3, 4, 5)}
MU = 1 << 29


def setup(O, seed, **over):
    """(params, oracle, CloudKey) of SK-128 with the given fields replaced, random keys"""
    import thfhe
    kw = dict(O.PARAM_SETS["SK-128"], **over)
    p = O.make_params(**kw)
    K = O.SKKeys(p, seed, 2.0**-25, 2.0**-15)
    return p, O.Oracle(p, K.bk, K.ksk), thfhe.CloudKey(thfhe.make_params(**kw), K.bk, K.ksk, device=0)


def twice(ck, shape, l, jobs, launch, ref):
    """launch() on the forced shape, twice: byte-identical outputs, every word equal to ref"""
    _, coop, ring4, name = RING[shape]
    with thresholds(ck, coop, ring4):
        assert ck.rotation_kernel_name(jobs) == name.format(l=l)
        first, second = launch(), launch()
        assert first.tobytes() == second.tobytes(), (shape, jobs, "two launches differ at", differing(first, second))
        assert np.array_equal(first, ref), (shape, jobs, differing(first, ref))


@pytest.mark.parametrize("n", [1, 2, 3, 5])
@pytest.mark.parametrize("l, Bgbit", [(1, 8), (2, 10), (3, 7), (4, 8)], ids=["l1", "l2", "l3", "l4"])
def test_depths_lengths_and_job_counts(O, l, Bgbit, n):
    p, orc, ck = setup(O, 0x6A00 + 16 * l + n, n=n, l=l, Bgbit=Bgbit)
    try:
        xs = words(np.random.default_rng(0x6B00 + 16 * l + n), 17, p.n + 1)
        ref = np.stack(pmap(lambda x: orc.bootstrap_wo_keyswitch(x, MU), xs))
        for shape, counts in JOBS.items():
            for jobs in counts:
                twice(ck, shape, l, jobs, lambda: ck.bootstrap_wo_keyswitch(xs[:jobs], MU), ref[:jobs])
    finally:
        ck.close()


def test_zero_mask_word_beside_working_neighbours(O):
    # n = 3, 9 jobs: job j skips CMux j mod 3 while the other waves of its workgroup transform and multiply there; job 4 skips every CMux
    p, orc, ck = setup(O, 0x6C0, n=3)
    try:
        xs = words(np.random.default_rng(0x6C1), 9, p.n + 1)
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
    p, orc, ck = setup(O, 0x6E0, n=3)
    yield p, orc, ck, words(np.random.default_rng(0x6E1), 9, p.n + 1)
    ck.close()


def test_lut_instantiation_theta4_n3(lut_env):
    p, orc, ck, xs = lut_env
    tv = words(np.random.default_rng(0x6E2), p.N)
    ref = np.stack(pmap(lambda x: R.lut_bootstrap(orc, [x], (1,), 0, tv, 4, keyswitch=False), xs))
    for shape in RING:
        twice(ck, shape, p.l, len(xs), lambda: ck.lut_bootstrap_wo_keyswitch(tv, xs, theta=4), ref)


def test_encrypted_table_instantiation_n3(lut_env):
    p, orc, ck, xs = lut_env
    rng = np.random.default_rng(0x6E3)
    tv_a, tv_b = words(rng, 2, p.N), words(rng, 2, p.N)      # any TLWE sample is a valid start: mask and body both rotate
    idx = (np.arange(len(xs)) % 2).astype(np.int32)
    ref = np.stack(pmap(lambda g: TR.lut_enc(orc, [xs[g]], (1,), 0, tv_a[idx[g]], tv_b[idx[g]], 2, keyswitch=False), range(len(xs))))
    for shape in RING:
        twice(ck, shape, p.l, len(xs), lambda: ck.lut_bootstrap_enc_wo_keyswitch(tv_a, tv_b, xs, theta=2, lut_index=idx), ref)


def test_multi_value_instantiation_n3(lut_env):
    p, orc, ck, xs = lut_env
    rng = np.random.default_rng(0x6E4)
    tv0 = words(rng, p.N)
    factors = words(rng, 2, 9, 16)            # two tables of q = 9 outputs, p = 16 taps
    idx = (np.arange(len(xs)) % 2).astype(np.int32)
    accs = pmap(lambda x: MV.rotate(orc, R.prologue([x], (1,), 0), tv0), xs)
    ref = np.stack([MV.combine(acc, factors[t], p.N) for acc, t in zip(accs, idx)])
    for shape in RING:
        twice(ck, shape, p.l, len(xs), lambda: ck.mv_lut_bootstrap_wo_keyswitch(factors, xs, tv0=tv0, table_index=idx), ref)


def test_both_shapes_at_the_bound(O):
    # the largest shape context creation admits (l = 3, Bgbit = 10): step 1 carries -Bg/2 in all six rows against key words 0x7FFF8000, every limb
    # sum of that CMux is 2l N 2^(Bgbit-1) 2^15; 9 rotations = a full eight-wave workgroup + one wave, two four-wave workgroups + one wave
    import thfhe
    l, Bgbit = 3, 10
    kw = dict(O.PARAM_SETS["SK-128"], n=4, l=l, Bgbit=Bgbit)
    p = O.make_params(**kw)
    K = O.SKKeys(p, 0x6F3, 2.0**-25, 2.0**-15)
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
