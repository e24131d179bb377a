"""The LWE -> TLWE packing key switch on the host: keygen.gen_pack_key against its definition, and the exact
phase property of the operation (the model in pack_reference.py) with a noiseless key."""
import numpy as np
import pytest

import pack_reference as PR

N = 1024


def _keys(rng, n):
    return rng.integers(0, 2, n).astype(np.int32), rng.integers(0, 2, N).astype(np.int32)


@pytest.mark.parametrize("t,basebit", [(8, 2), (4, 2), (5, 3)])
def test_gen_pack_key_rows_decrypt_to_the_gadget(t, basebit):
    from thfhe import keygen
    rng = np.random.default_rng(t * 10 + basebit)
    n, sigma = 12, 2.0**-25
    s, z = _keys(rng, n)
    pk = keygen.gen_pack_key(rng, s, z, t, basebit, sigma)
    R = (1 << basebit) - 1
    assert pk.shape == (n, t, R, 2, N) and pk.dtype == np.int32
    ph = PR.tlwe_phase(pk[..., 0, :].reshape(-1, N), pk[..., 1, :].reshape(-1, N), z).reshape(n, t, R, N).astype(np.int64)
    j, p, v = np.meshgrid(np.arange(n), np.arange(t), np.arange(1, R + 1), indexing="ij")
    msg = np.zeros((n, t, R, N), np.int64)
    msg[..., 0] = (v * s[j].astype(np.int64)) << (32 - (p + 1) * basebit)
    err = PR.torus(PR.wrap32(ph - msg))
    assert np.abs(err).max() <= 6 * sigma
    assert 0.9 * sigma < err.std() < 1.1 * sigma          # Gaussian on all N coefficients of every row
    assert len(np.unique(pk[..., 0, :])) > 0.99 * pk[..., 0, :].size   # alpha uniform


@pytest.mark.parametrize("m", [1, 7, 1024])
def test_noiseless_packing_adds_exactly_the_rounding(m):
    from thfhe import keygen
    rng = np.random.default_rng(m)
    n, t, basebit = 16, 8, 2
    s, z = _keys(rng, n)
    pk = keygen.gen_pack_key(rng, s, z, t, basebit, 0.0)
    count = m if m > 1 else 3                      # m = 1: three outputs of one sample each
    lwe = rng.integers(-2**31, 2**31, size=(count, n + 1), dtype=np.int64).astype(np.int32)
    lwe[0, :n] = -1
    if count > 2:
        lwe[1, :n], lwe[2, :n] = 2**31 - 1, -2**31
    a, b = PR.pack(lwe, pk, t, basebit, m)
    assert a.shape == b.shape == (-(-count // m), N)
    ph = PR.tlwe_phase(a, b, z).astype(np.int64)
    lph = PR.lwe_phase(lwe, s).astype(np.int64)
    rnd = -((PR.rounded(lwe[:, :n], t, basebit) - (lwe[:, :n].astype(np.int64) & PR.M32)) * s).sum(axis=1)
    for g in range(a.shape[0]):
        k = min(m, count - g * m)
        want = np.zeros(N, np.int64)
        want[:k] = lph[g * m:g * m + k] + rnd[g * m:g * m + k]
        assert np.array_equal(PR.wrap32(ph[g]), PR.wrap32(want)), g
