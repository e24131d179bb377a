"""The leveled kernels of the 64-bit ring of degree 2048 at the proven bound of their FP64 transforms (DESIGN.md sections 3 and 4.26): the quantity
thfhe_mk_ctx_create checks, 2 l parts N 2^(part bits - 1) 2^15 <= 2^37.  The crafted inputs of tests/mk_lhe_cases.py put every digit part at its
extreme and set words with limbs of magnitude 2^15 against them: the limb sums reach 137 036 300 288 = 0.997 x 2^37 (asserted, with Python integers,
in tests/test_mk_lhe_host.py, which also shows that one flipped bit of a limb sum changes a compared word).  Word equality with the model, for
mk_lhe_cmux2k_kernel, for mk_lhe_rotate2k_kernel, and for a rotation step that follows a crafted step."""
import numpy as np
import pytest

import mk_lhe_cases as CS
import mk_lhe_reference as M
from support import differing

pytestmark = pytest.mark.gpu
N, L, BGBIT = CS.N, CS.L, CS.BGBIT


@pytest.fixture(scope="module")
def ck():
    import thfhe
    p, K, orc = CS.keys()
    c = thfhe.MKCloudKey(thfhe.make_params(**CS.KW), K.bk, K.ksk, device=0)
    yield c
    c.close()


def test_cmux_at_the_bound(ck):
    w, d1, d0 = CS.bound_cmux_case()
    want = M.cmux(CS.model_set(w, 1), 0, 0, d1, d0)
    with ck.tgsw_set(w, 1) as ts:
        got_a, got_b = ck.lhe_cmux(ts, 0, d1[0], d1[1], d0[0], d0[1])
    assert np.array_equal(got_a[0], want[0]) and np.array_equal(got_b[0], want[1]), (differing(got_a[0], want[0]), differing(got_b[0], want[1]))


def test_tree_level_at_the_bound(ck):
    """The same CMux as a tree level of a lookup: d1 = table polynomial 1, d0 = polynomial 0 (zero), on an encrypted table."""
    w, d1, d0 = CS.bound_cmux_case()
    tab_a, tab_b = np.stack([d0[0], d1[0]]), np.stack([d0[1], d1[1]])
    want = M.lookup_wo_keyswitch(CS.model_set(w, 1), 0, 1, 0, 4, tab_a, tab_b)
    with ck.tgsw_set(w, 1) as ts:
        got = ck.lhe_lookup_wo_keyswitch(ts, tab_b, d_tree=1, d_rot=0, theta=4, tab_a=tab_a)
    assert np.array_equal(got[0], want), differing(got[0], want)


@pytest.mark.parametrize("follow", ["crafted", "random"])
def test_rotation_at_the_bound_and_the_step_after(ck, follow):
    """(0, 2) on the table whose first rotation step has the crafted difference on both polynomials; bit 1 then rotates what the crafted step
    left -- by a set of the same extreme words, or by random words."""
    w, _, _ = CS.bound_cmux_case()
    nxt = w if follow == "crafted" else CS.words64(np.random.default_rng(9), 1, 1, 4, L, N)
    words = np.concatenate([w, nxt], axis=1)
    tab = CS.bound_rot_table(512)
    want = M.lookup_wo_keyswitch(CS.model_set(words, 2), 0, 0, 2, 4, tab, tab)
    with ck.tgsw_set(words, 2) as ts:
        got = ck.lhe_lookup_wo_keyswitch(ts, tab, d_tree=0, d_rot=2, theta=4, tab_a=tab)
    assert np.array_equal(got[0], want), differing(got[0], want)
