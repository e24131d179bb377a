"""ks_staged_kernel on its own (pytest -m gpu): all seven instances on the single key with t = 5 (stages straddle coordinates, no planes), the
512-word rows with t = 1 .. 7, the threshold of 192 samples, a ragged last workgroup of 32, and the single key's span of 128 coordinates from
2 048 samples on.  The multi-key spans run in test_gpu_ks_layouts.py.  Cases and checks: tests/ks_cases.py."""
import pytest

import ks_cases as KC

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("c", KC.family("staged"), ids=lambda c: c.id)
def test_staged(c):
    assert any(KC.case_route(c, count)[0] == "staged" for count in c.counts)
    KC.check_case(c)
