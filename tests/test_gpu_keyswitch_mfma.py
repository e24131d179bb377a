"""The key switch on the matrix cores (sk_keyswitch_mfma_kernel, pytest -m gpu): from 512 gates on, the shapes it takes (2-bit digits,
t = 4 or 8, rows of 512 / 640 / 1152 words) run as an int8 GEMM.  Every output word must equal the older kernels' result on the same inputs
(cut into batches below the threshold) and the CPU oracle on sampled rows."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MFMA_MIN_GATES = 512   # kKsMfmaMinSamples (thfhe_keyswitch.h)
SMALL = 200            # batches of this size stay on ks_staged_kernel


def _inputs(p, batch, seed):
    rng = np.random.default_rng(seed)
    u = rng.integers(-2**31, 2**31, (batch, p.N + 1), dtype=np.int64).astype(np.int32)
    u[0, :] = 0                      # every digit zero but the rounding offset's carry
    u[1, :] = -1                     # all digits 3
    u[2, :] = 2**31 - 1
    u[-1, :] = -2**31
    return u


def _in_pieces(ck, u):
    return np.concatenate([ck.keyswitch(u[q:q + SMALL]) for q in range(0, len(u), SMALL)])


def _check(ck, orc, p, batch, seed):
    u = _inputs(p, batch, seed)
    got = ck.keyswitch(u)
    assert got.shape == (batch, p.n + 1)
    ref = _in_pieces(ck, u)
    bad = np.nonzero((got != ref).any(axis=1))[0]
    assert bad.size == 0, (batch, bad[:8])
    for g in sorted(set([0, 1, 2, 3, batch // 2, batch - 2, batch - 1] + list(range(5, batch, 397)))):
        assert np.array_equal(got[g], orc.keyswitch(u[g])), (batch, g)


def _ctx(O, name, **kw):
    import thfhe
    p = O.make_params(name, **kw)
    s = O.SIGMAS[name]
    K = O.SKKeys(p, 0x4D46, s["bk"], s["ks"])
    return p, K, O.Oracle(p, K.bk, K.ksk), thfhe.CloudKey(thfhe.make_params(name, **kw), K.bk, K.ksk, device=0)


def test_sk128_at_and_around_the_threshold(O, sk128):
    import thfhe
    p, K, orc = sk128
    ck = thfhe.CloudKey(thfhe.make_params("SK-128"), K.bk, K.ksk, device=0)
    for batch, seed in ((4096, 1), (MFMA_MIN_GATES - 1, 2), (MFMA_MIN_GATES, 3), (MFMA_MIN_GATES + 1, 4), (2051, 5), (4353, 6)):
        _check(ck, orc, p, batch, seed)
    ck.close()


@pytest.mark.parametrize("name,kw", [("SK-128", dict(ks_t=4)), ("SK-80", {}), ("SK-lib", {})])
def test_other_shapes(O, name, kw):
    p, K, orc, ck = _ctx(O, name, **kw)
    for batch, seed in ((4096, 11), (MFMA_MIN_GATES + 3, 12)):
        _check(ck, orc, p, batch, seed)
    ck.close()


def test_mux_and_nand_batches(O, sk128):
    """the two-rotation input of the MUX epilogue ((0, 2^29) + u1 + u2) and a 4 096-gate NAND batch through the new kernel"""
    import thfhe
    p, K, orc = sk128
    ck = thfhe.CloudKey(thfhe.make_params("SK-128"), K.bk, K.ksk, device=0)
    lwe = O.SIGMAS["SK-128"]["lwe"]
    rng = np.random.default_rng(21)
    B = 600
    bits = rng.integers(0, 2, (3, B))
    cx, cy, cz = (K.encrypt_bits(bits[q], lwe, 400 + q) for q in range(3))
    got = thfhe.gate_mux(ck, cx, cy, cz)
    assert np.array_equal(K.decrypt_bits(got), np.where(bits[0] == 1, bits[1], bits[2]).astype(bool))
    ref = np.concatenate([thfhe.gate_mux(ck, cx[q:q + SMALL], cy[q:q + SMALL], cz[q:q + SMALL]) for q in range(0, B, SMALL)])
    assert np.array_equal(got, ref)
    s = [0, 1, 299, 598, 599]
    assert np.array_equal(got[s], orc.gates(O.MUX, cx[s], cy[s], cz[s]))

    B = 4096
    a, b = rng.integers(0, 2, (2, B))
    ca, cb = K.encrypt_bits(a, lwe, 500), K.encrypt_bits(b, lwe, 501)
    got = ck.gates(O.NAND, ca, cb)
    assert np.array_equal(K.decrypt_bits(got), ~(a.astype(bool) & b.astype(bool)))
    s = [0, 1, 1000, 2047, 2048, 4095]
    assert np.array_equal(got[s], orc.gates(O.NAND, ca[s], cb[s]))
    ck.close()
