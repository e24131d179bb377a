"""The ring kernel's folded transforms (variant "f") on the MI355X (pytest -m gpu): both ring shapes, gate and LUT
instantiations, every output word against the oracle -- at the exactness bound (crafted inputs of tests/bound_inputs.py) and on random keys with
the mask words that take the CMux loop's special paths.  Each case asserts the kernel that ran."""
import numpy as np
import pytest

import bound_inputs as B
import lut_reference as R
from support import KERNELS, differing, thresholds, words

pytestmark = pytest.mark.gpu

RING = [k for k in KERNELS if k[0] in ("ring8", "ring4")]   # W = 8 and W = 4


@pytest.mark.parametrize("l, Bgbit", [(2, 10), (3, 7), (3, 10)], ids=["l2-Bg10", "l3-Bg7", "l3-Bg10"])
def test_ring_shapes_at_the_bound(O, l, Bgbit):
    # step 0 copies the body into the mask, step 1 carries -Bg/2 in all 2l rows against key words 0x7FFF8000: every limb sum of that CMux is
    # 2l N 2^(Bgbit-1) 2^15; 12 rotations = one full eight-wave workgroup + half of one, three four-wave workgroups
    import thfhe
    kw = dict(O.PARAM_SETS["SK-128"], n=4, l=l, Bgbit=Bgbit)
    p = O.make_params(**kw)
    K = O.SKKeys(p, 0xF0 + l, 2.0**-25, 2.0**-15)
    bk, x, mu, step = B.sk_case(p, K.bk, True)
    orc = O.Oracle(p, bk, K.ksk)
    assert B.sk_reached(orc, p, bk, x, mu, step) == B.bound(2 * l, p.N, Bgbit)
    ref = orc.bootstrap_wo_keyswitch(x, mu)
    tv = np.full(p.N, mu, np.int32)
    ref_lut = R.lut_bootstrap(orc, [x], (1,), 0, tv, 4, keyswitch=False)
    xs = np.tile(x, (12, 1))
    ck = thfhe.CloudKey(thfhe.make_params(**kw), bk, K.ksk, device=0)
    try:
        for _, coop, ring4, name in RING:
            with thresholds(ck, coop, ring4):
                assert ck.rotation_kernel_name(len(xs)) == name.format(l=l)
                got = ck.bootstrap_wo_keyswitch(xs, mu)
                assert np.array_equal(got, np.tile(ref, (12, 1))), (name, differing(got, np.tile(ref, (12, 1))))
                u = ck.lut_bootstrap_wo_keyswitch(tv, xs, theta=4)     # the LUT instantiation of the same loop, four outputs per rotation
                for g in range(len(xs)):
                    assert np.array_equal(u[g], ref_lut), (name, g)
    finally:
        ck.close()


def test_random_keys_and_the_special_mask_words(O):
    # n = 8, 9 jobs: one full eight-wave workgroup plus one wave with seven idle partners (four-wave shape: 4 + 4 + 1).  Mask words forced to the
    # mod-switched values 0 (skipped CMux), 1 (smallest rotation), 1024 (X^N = -1) and 2047 (largest rotation) in some jobs, random elsewhere.
    import thfhe
    kw = dict(O.PARAM_SETS["SK-128"], n=8)
    p = O.make_params(**kw)
    K = O.SKKeys(p, 0xF8, 2.0**-25, 2.0**-15)
    orc = O.Oracle(p, K.bk, K.ksk)
    xs = words(np.random.default_rng(0xF9), 9, p.n + 1)
    forced = {0: 0, 1: 1 << 21, 1024: -2**31, 2047: -(1 << 21)}     # word -> its value mod-switched to Z_2N
    for job, col, want in [(0, 0, 0), (0, 3, 1), (1, 1, 1024), (1, 7, 2047), (3, 0, 1), (3, 1, 0), (3, 2, 0), (5, 4, 2047), (8, 0, 1024), (8, 5, 0), (8, 7, 1)]:
        xs[job, col] = forced[want]
        assert O.lib().oracle_modswitch(int(xs[job, col]), p.N) % (2 * p.N) == want
    xs[6, :p.n] = 0                                                   # a job whose every CMux is skipped
    mu = 1 << 29
    ref = np.stack([orc.bootstrap_wo_keyswitch(x, mu) for x in xs])
    ck = thfhe.CloudKey(thfhe.make_params(**kw), K.bk, K.ksk, device=0)
    try:
        for _, coop, ring4, name in RING:
            with thresholds(ck, coop, ring4):
                assert ck.rotation_kernel_name(len(xs)) == name.format(l=p.l)
                got = ck.bootstrap_wo_keyswitch(xs, mu)
                assert np.array_equal(got, ref), (name, differing(got, ref))
    finally:
        ck.close()
