"""The key switch in the other engines' layouts (pytest -m gpu): 3-gen (one mask for all parties; N = 1024 / 2048 / 4096, party blocks off the
16-byte alignment, the nsplit tiers and the two mask slices that fill sA), KMS (one mask per party) and the packing key (rows of 2N words,
b inside the row, LWE dimensions at the coordinate padding's edge).  Cases and checks: tests/ks_cases.py."""
import pytest

import ks_cases as KC

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("c", KC.family("layouts"), ids=lambda c: c.id)
def test_layout(c):
    KC.check_case(c)
