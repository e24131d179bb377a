"""rotation_kernel_name is the library's own answer: under every threshold setting the shape sweeps use (support.KERNELS) a live context
reports the kernel that the frozen rules of tests/test_launch_plan.py name, on both sides of every branch of the single-key plan and of the
multi-key pair threshold.  The contexts hold zero keys of a few LWE words; nothing is bootstrapped.  CPU twin: tests/test_launch_plan.py."""
import ctypes as C

import numpy as np
import pytest

import support as S
from test_launch_plan import mk_name, sk_name

pytestmark = pytest.mark.gpu


def test_single_key_context_reports_the_plan_under_every_threshold_setting():
    import thfhe
    p = thfhe.make_params("SK-128", n=8)
    ck = thfhe.CloudKey(p, np.zeros(p.n * 2 * p.l * 2 * p.N, np.int32), np.zeros(p.N * p.ks_t * ((1 << p.ks_basebit) - 1) * (p.n + 1), np.int32), device=0)
    try:
        rotations = (5, 12, 1024, 1100, 2048, 2049)
        assert [ck.rotation_kernel_name(r) for r in rotations] == [sk_name(p.l, r, S.DEFAULT_COOP, S.DEFAULT_RING4) for r in rotations]
        for kid, coop, ring4, below_2048 in S.KERNELS:
            with S.thresholds(ck, coop, ring4):
                for r in rotations:
                    assert ck.rotation_kernel_name(r) == sk_name(p.l, r, coop, ring4), (kid, r)
                assert ck.rotation_kernel_name(5 if kid != "split" else 12) == below_2048.format(l=p.l)
            assert ck.rotation_kernel_name(5) == "sk_blind_rotate_coop_kernel<3>"   # the defaults are back
        with pytest.raises(thfhe.ThfheError, match="too short"):
            thfhe._check(thfhe.lib().thfhe_rotation_kernel_name(ck.h, 5, C.create_string_buffer(8), 8))
    finally:
        ck.close()


def test_multi_key_context_reports_the_pair_threshold_it_was_given():
    import thfhe
    p = thfhe.make_params("MK2", n=8)
    ck = thfhe.MKCloudKey(p, np.zeros(p.parties * p.n * 4 * p.l * p.N, np.int64),
                          np.zeros(p.parties * p.N * p.ks_t * ((1 << p.ks_basebit) - 1) * (p.n + 1), np.int32), device=0)
    try:
        assert [ck.rotation_kernel_name(r) for r in (4, 300)] == ["mk_blind_rotate_coop_kernel<2>", "mk_blind_rotate_pair_kernel<2>"]
        for thr in (0, 4, 299, 300, 1 << 20):
            ck.set_pair_threshold(thr)
            for r in (4, 300):
                assert ck.rotation_kernel_name(r) == mk_name(p.N, p.l, p.Bgbit, r, thr), (thr, r)
    finally:
        ck.close()
