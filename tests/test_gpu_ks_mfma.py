"""sk_keyswitch_mfma_kernel on its own (pytest -m gpu): t = 4 and 8 at 4 .. 44 word tiles, rows that fill their padding, a last tile that holds
just the b column, the threshold of 512 samples and ragged last tiles of 256 and 32; and the MUX combine (rot_per_gate = 2) through gates()
on the plain, staged and matrix-core kernels.  Cases and checks: tests/ks_cases.py."""
import numpy as np
import pytest

import ks_cases as KC
from support import differing

pytestmark = pytest.mark.gpu

MUX_PIECE = 24   # gates per call of the piecewise comparison: the plain kernel with nsplit = 16


@pytest.mark.parametrize("c", KC.family("mfma"), ids=lambda c: c.id)
def test_mfma(c):
    assert any(KC.case_route(c, count)[0] == "mfma" for count in c.counts)
    KC.check_case(c)


@pytest.mark.parametrize("c", KC.family("mux"), ids=lambda c: c.id)
def test_mux(O, c):
    """random records through gates(MUX): two rotations per gate, the key switch of u1 + u2 + (0, 2^29).  Real keys: with a zero bootstrapping
    key the extracted masks would be zero."""
    import thfhe
    kw = dict(n=c.n, N=1024, k=1, l=1, Bgbit=8, ks_t=c.t, ks_basebit=c.basebit, torus_bits=32, parties=1)
    p = O.make_params(**kw)
    K = O.SKKeys(p, 0x4D55 + c.t, 2.0**-25, 2.0**-15)
    orc = O.Oracle(p, K.bk, K.ksk)
    ck = thfhe.CloudKey(thfhe.make_params(**kw), K.bk, K.ksk, device=0)
    try:
        for count in c.counts:
            rt = KC.case_route(c, count)
            assert rt[0] == c.counts[count] and KC.case_route(c, MUX_PIECE)[0] == "plain"
            x, y, z = (KC.random_words(np.random.default_rng(7 * count + q), (count, c.n + 1)) for q in range(3))
            got = ck.gates(O.MUX, x, y, z)
            assert got.shape == (count, c.n + 1)
            assert np.array_equal(ck.gates(O.MUX, x, y, z), got), (c.id, count, "second call differs")
            s = sorted({0, 1, 31, 32, count // 2, 32 * ((count - 1) // 32), 256 * ((count - 1) // 256), count - 2, count - 1} & set(range(count)))
            ref = orc.gates(O.MUX, x[s], y[s], z[s])
            assert np.array_equal(got[s], ref), (c.id, count, rt, [[s[g], w] for g, w in differing(got[s], ref)])
            if count > MUX_PIECE:
                other = np.concatenate([ck.gates(O.MUX, x[q:q + MUX_PIECE], y[q:q + MUX_PIECE], z[q:q + MUX_PIECE]) for q in range(0, count, MUX_PIECE)])
                assert np.array_equal(got, other), (c.id, count, rt, differing(got, other))
    finally:
        ck.close()
