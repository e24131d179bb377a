"""ks_plain_kernel on its own (pytest -m gpu): every compiled row width, the rows that exactly fill their padding, the single key's nsplit
tiers, the digit shapes up to t basebit = 31, and the batches of 192 samples and more that stay on it.  Cases and checks: tests/ks_cases.py."""
import numpy as np
import pytest

import ks_cases as KC

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("c", KC.family("plain"), ids=lambda c: c.id)
def test_plain(c):
    KC.check_case(c)


def test_refused_shapes_leave_the_process_working():
    """n = 1408 and t basebit = 32 are refused when the context is made, with the documented errors; a context made afterwards works"""
    import thfhe

    def make(n, t, bb):
        p = thfhe.make_params(n=n, N=1024, k=1, l=1, Bgbit=8, ks_t=t, ks_basebit=bb, torus_bits=32, parties=1)
        return thfhe.CloudKey(p, np.zeros((n, 2, 2, 1024), np.int32), np.zeros((1024, t, (1 << bb) - 1, n + 1), np.int32), device=0)

    with pytest.raises(thfhe.ThfheError, match="need 1 <= n <= 1407"):
        make(1408, 1, 1)
    for t, bb in ((32, 1), (16, 2), (8, 4)):
        with pytest.raises(thfhe.ThfheError, match="bad key-switch parameters"):
            make(4, t, bb)
    c = KC._c("after-refusal", "plain", "sk", 1407, 1, 1, {3: "plain"})
    KC.check_case(c)
