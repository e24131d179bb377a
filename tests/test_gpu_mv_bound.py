"""The multi-value instantiations of the blind rotations on the MI355X at the exactness bound of DESIGN.md section 3 (pytest -m gpu).

launch_rotations<kLutMv> compiles the CMux loop of sk_blind_rotate_ring_kernel<L, 5, 8, kLutMv>, of the four-wave ring shape and of
sk_blind_rotate_coop_kernel<L, 1, kLutMv> once more for every L; test_gpu_mv_lut_shapes.py drives them with random words only, 5 - 8 bits
below the bound.  Here the crafted bootstrap of tests/bound_inputs.py (sk_case, unchanged: kLutMv starts like kLut, and with tv0 = mu
everywhere, one input of weight 1 and bias 0 its rotation is the gate's) puts the extreme digit in all 2l rows of one CMux against a key
whose every word has both limbs at magnitude 2^15: the limb sum at coefficient N - 1 is 2l N 2^(Bgbit-1) 2^15 itself (half of it at l = 4,
Bgbit = 8, where l Bgbit = 32 leaves the single-key recipe the l body rows).  Each case asserts the sum it reached, the kernel that ran and
every word of all 12 x q records against the model's combination of the oracle's accumulator.  The inputs are not valid ciphertexts; the
contract is word equality.

Output 0 of every factor table is a single unit tap (bound_inputs.mv_factors): its record is minus one plain extraction, so it carries every
coefficient of the accumulator's mask column -- the peak at coefficient N - 1 is observed there -- bit for bit; of the body the records
carry the coefficients at the tap positions.  tests/test_bound_inputs.py::test_multi_value_records_see_one_lsb checks both on the CPU."""
import numpy as np
import pytest

import bound_inputs as B
import lut_reference as R
import mv_lut_reference as MV
from support import KERNELS, differing
from test_bound_inputs import MV_IDS, MV_PQ, MV_SHAPES, MV_TABLES

pytestmark = pytest.mark.gpu

BATCH = 12      # identical samples: more than one workgroup of either ring shape, and both launches of the split case; every one compared
# the table of every sample: both tables in either launch of the split case (6 + 6), and the two launches differ
TABLE_INDEX = np.array([0, 1, 1, 0, 1, 0, 1, 1, 0, 0, 1, 0], np.int32)


@pytest.mark.parametrize("l, Bgbit, full", MV_SHAPES, ids=MV_IDS)
def test_multi_value_at_the_bound(O, l, Bgbit, full):
    import thfhe
    assert not np.array_equal(TABLE_INDEX[:6], TABLE_INDEX[6:]) and set(TABLE_INDEX[:6]) == set(TABLE_INDEX[6:]) == {0, 1}
    kw = dict(O.PARAM_SETS["SK-128"], n=4, l=l, Bgbit=Bgbit)
    p = O.make_params(**kw)
    N = p.N
    K = O.SKKeys(p, 0xB0 + l, 2.0**-25, 2.0**-15)
    bk, x, mu, step = B.sk_case(p, K.bk, full)
    orc = O.Oracle(p, bk, K.ksk)
    assert B.sk_reached(orc, p, bk, x, mu, step) == B.bound(2 * l, N, Bgbit) // (1 if full else 2)
    tv0 = np.full(N, mu, np.int32)
    acc = MV.rotate(orc, R.prologue([x], (1,), 0), tv0)            # the oracle's CMux chain
    assert np.array_equal(R.extract_at(acc, 0, N), orc.bootstrap_wo_keyswitch(x, mu))
    cases = []
    for pt, q in MV_PQ:
        w = B.mv_factors(np.random.default_rng(0xF0 + pt), MV_TABLES, q, pt)
        by_table = np.stack([MV.combine(acc, w[t], N) for t in range(MV_TABLES)])
        assert not np.array_equal(by_table[0], by_table[1])
        cases.append((pt, q, w, by_table))
    xs = np.tile(x, (BATCH, 1))
    ck = thfhe.CloudKey(thfhe.make_params(**kw), bk, K.ksk, device=0)
    try:
        for kid, coop, ring4, name in KERNELS:
            ck.set_coop_threshold(coop)
            ck.set_ring4_threshold(ring4)
            assert ck.rotation_kernel_name(BATCH) == name.format(l=l)
            for pt, q, w, by_table in cases:
                ref = by_table[TABLE_INDEX]
                u = ck.mv_lut_bootstrap_wo_keyswitch(w, xs, tv0=tv0, table_index=TABLE_INDEX)
                assert u.shape == (BATCH, q, N + 1)
                assert np.array_equal(u, ref), (kid, pt, q, differing(u, ref))
        # the key-switched call once per shape (the kernel case left selected: the split)
        pt, q, w, by_table = cases[1]
        ks = np.stack([orc.keyswitch(r) for r in by_table.reshape(-1, N + 1)]).reshape(MV_TABLES, q, -1)[TABLE_INDEX]
        got = ck.mv_lut_bootstrap(w, xs, tv0=tv0, table_index=TABLE_INDEX)
        assert np.array_equal(got, ks), differing(got, ks)
    finally:
        ck.close()
