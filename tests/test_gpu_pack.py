"""The LWE -> TLWE packing key switch on the GPU (pytest -m gpu): thfhe_pack_lwe word for word against the
numpy model (pack_reference.py) on both sides of its kernel threshold, the reference's Convert flow (src/Convert.cpp:29-33,86-114)
with one packed sample for a 32-bit result, the noise of 1 024 slots against its prediction, the SK-lib comparison with the per-bit
TLweFromLwe path, and the error paths."""
import ctypes as C

import numpy as np
import pytest

import pack_reference as PR

pytestmark = pytest.mark.gpu

N = 1024
PACK_MFMA_MIN = 8     # kPackMfmaMinSamples (thfhe_threshold.hip): below, the plain kernel
ADVERSARIAL = {0: 0, 1: -1, 2: 2**31 - 1, 3: -2**31, 30: -1, 31: 2**31 - 1, 1023: 0, 1024: -2**31, 4095: -1}


def _lwe(rng, count, n):
    x = rng.integers(-2**31, 2**31, size=(count, n + 1), dtype=np.int64).astype(np.int32)
    for r, w in ADVERSARIAL.items():
        if r < count:
            x[r, :n] = w
    return x


def additive_shares(rng, key, t):
    """as test_threshold.additive_shares: finalDecrypt computes b - partial_0 + sum_{i>=1} partial_i, so key = s_0 - s_1 - ... - s_{t-1}."""
    others = [rng.integers(-3, 4, N).astype(np.int32) for _ in range(t - 1)]
    return [key.astype(np.int32) + sum(others, np.zeros(N, np.int32))] + others


def threshold_decrypt(T, ctx, a, b, z, rng, parties=3):
    shares = additive_shares(rng, z, parties)
    noises = [np.trunc(rng.standard_normal(a.shape) * 2.0**-20 * 2.0**32).astype(np.int32) for _ in range(parties)]
    parts = np.stack([T.PartialDecrypt(ctx, shares[i], a, noises[i]) for i in range(parties)])
    return T.finalDecrypt(ctx, b, parts, want_result=True)


@pytest.fixture(scope="module")
def ctx():
    from thfhe import threshold as T
    c = T.PolyContext(0)
    yield c
    c.close()


@pytest.mark.parametrize("name", ["SK-128", "SK-80", "SK-lib"])
def test_pack_equals_the_model_word_for_word(ctx, name):
    import thfhe
    from thfhe import keygen
    from thfhe import threshold as T
    p = thfhe.make_params(name)
    rng = np.random.default_rng(p.n)
    s, z = rng.integers(0, 2, p.n).astype(np.int32), rng.integers(0, 2, N).astype(np.int32)
    pk = keygen.gen_pack_key(rng, s, z, p.ks_t, p.ks_basebit, thfhe.SIGMAS[name]["bk"])
    ctx.set_pack_key(pk, p.ks_t, p.ks_basebit)
    lwe = _lwe(rng, 4096, p.n)
    Tm = PR.per_sample(lwe, pk, p.ks_t, p.ks_basebit)     # a prefix of the samples is the model of a smaller batch
    for count in (1, PACK_MFMA_MIN - 1, PACK_MFMA_MIN, 31, 32, 1024, 1025, 4096):
        x = lwe[:count].copy()
        x[-1, :p.n] = -2**31                             # the batch's last mask extreme too
        Tx = np.concatenate([Tm[:count - 1], PR.per_sample(x[-1:], pk, p.ks_t, p.ks_basebit)])
        for slots in (1, 32, 1024):
            a, b = T.PackLwe(ctx, x, slots)
            ra, rb = PR.rotate_sum(Tx, slots, N)
            assert a.shape == ra.shape == (-(-count // slots), N)
            assert np.array_equal(a, ra) and np.array_equal(b, rb), (name, count, slots)


@pytest.mark.parametrize("n,t,basebit,counts", [(100, 4, 2, (1, 7, 8, 300)), (40, 5, 3, (1, 64)), (1, 16, 2, (33,))])
def test_pack_other_shapes_equal_the_model(ctx, n, t, basebit, counts):
    # t = 4 on the matrix cores, 3-bit digits on the plain kernel only, a dimension far below its padding (n = 1 -> 128)
    from thfhe import keygen
    from thfhe import threshold as T
    rng = np.random.default_rng(n * 100 + t)
    s, z = rng.integers(0, 2, n).astype(np.int32), rng.integers(0, 2, N).astype(np.int32)
    pk = keygen.gen_pack_key(rng, s, z, t, basebit, 2.0**-25)
    ctx.set_pack_key(pk, t, basebit)
    for count in counts:
        x = _lwe(rng, count, n)
        for slots in (1, 7, 1024):
            a, b = T.PackLwe(ctx, x, slots)
            ra, rb = PR.pack(x, pk, t, basebit, slots)
            assert np.array_equal(a, ra) and np.array_equal(b, rb), (n, t, basebit, count, slots)


@pytest.fixture(scope="module")
def sk128_pack(ctx):
    import thfhe
    from thfhe import keygen
    p = thfhe.make_params("SK-128")
    K = keygen.SecretKeySet(p, seed=0x9AC0001)
    ck = thfhe.CloudKey(p, K.bk, K.ksk, device=0)
    rng = np.random.default_rng(0x9AC0002)
    z = rng.integers(0, 2, N).astype(np.int32)
    sigma = thfhe.SIGMAS["SK-128"]["bk"]
    pk = keygen.gen_pack_key(rng, K.lwe_key, z, p.ks_t, p.ks_basebit, sigma)
    yield p, K, ck, z, pk, sigma
    ck.close()


def test_convert_flow_32_bits_in_one_partial_decryption(ctx, sk128_pack):
    # src/Convert.cpp:29-33,86-114: a 32-bit AND of two encrypted words, then ONE packed sample per party instead of 32
    import thfhe
    from thfhe import threshold as T
    p, K, ck, z, pk, sigma = sk128_pack
    ctx.set_pack_key(pk, p.ks_t, p.ks_basebit)
    msg1, msg2 = 0xDEADBEEF, 0x7F3A05C6
    bits1 = np.array([(msg1 >> i) & 1 for i in range(32)])
    bits2 = np.array([(msg2 >> i) & 1 for i in range(32)])
    out = thfhe.gate_and(ck, K.encrypt(bits1, 1), K.encrypt(bits2, 2))
    a, b = T.PackLwe(ctx, out, slots=32)
    assert a.shape == b.shape == (1, N)
    bits, res = threshold_decrypt(T, ctx, a, b, z, np.random.default_rng(5))
    got = T.packed_bits(res, 32, slots=32)
    assert sum(int(v) << i for i, v in enumerate(got)) == msg1 & msg2


def test_4096_gate_outputs_1024_per_sample_noise(ctx, sk128_pack):
    import thfhe
    from thfhe import threshold as T
    p, K, ck, z, pk, sigma = sk128_pack
    ctx.set_pack_key(pk, p.ks_t, p.ks_basebit)
    rng = np.random.default_rng(11)
    x, y = rng.integers(0, 2, 4096), rng.integers(0, 2, 4096)
    want = (x & y).astype(bool)
    out = thfhe.gate_and(ck, K.encrypt(x, 3), K.encrypt(y, 4))
    a, b = T.PackLwe(ctx, out, slots=1024)
    assert a.shape == (4, N)
    ph = PR.tlwe_phase(a, b, z).reshape(-1)
    assert np.array_equal(ph > 0, want)
    err = PR.torus(PR.wrap32(ph.astype(np.int64) - PR.lwe_phase(out, K.lwe_key).astype(np.int64)))
    pred = PR.predicted_sigma(1024, p.n, p.ks_t, p.ks_basebit, int(K.lwe_key.sum()), sigma)
    assert 0.5 * pred <= err.std() <= 1.5 * pred, (err.std(), pred)
    assert np.abs(PR.torus(ph) - np.where(want, 0.125, -0.125)).max() < 1.0 / 16
    bits, res = threshold_decrypt(T, ctx, a, b, z, rng)
    assert np.array_equal(T.packed_bits(res, 4096, 1024), want)


def test_sk_lib_packed_equals_per_bit_conversion(ctx):
    import thfhe
    from thfhe import keygen
    from thfhe import threshold as T
    p = thfhe.make_params("SK-lib")
    K = keygen.SecretKeySet(p, seed=0x9AC0003)
    ck = thfhe.CloudKey(p, K.bk, K.ksk, device=0)
    rng = np.random.default_rng(12)
    x, y = rng.integers(0, 2, 100), rng.integers(0, 2, 100)
    out = thfhe.gate_nand(ck, K.encrypt(x, 5), K.encrypt(y, 6))
    ck.close()
    s = K.lwe_key   # TLweFromLwe's ring key is the LWE key itself (n = N); the packing key switches s -> s
    ta, tb = T.TLweFromLwe(ctx, out)
    per_bit, _ = threshold_decrypt(T, ctx, ta, tb, s, np.random.default_rng(7))
    ctx.set_pack_key(keygen.gen_pack_key(rng, s, s, p.ks_t, p.ks_basebit, thfhe.SIGMAS["SK-lib"]["bk"]), p.ks_t, p.ks_basebit)
    a, b = T.PackLwe(ctx, out, slots=64)
    assert a.shape == (2, N)
    _, res = threshold_decrypt(T, ctx, a, b, s, np.random.default_rng(8))
    packed = T.packed_bits(res, 100, 64)
    assert np.array_equal(packed, per_bit)
    assert np.array_equal(packed, ~(x.astype(bool) & y.astype(bool)))


def test_pack_error_paths_leave_the_context_working():
    import thfhe
    from thfhe import keygen
    from thfhe import threshold as T
    L = thfhe.lib()
    ctx = T.PolyContext(0)
    z32 = np.zeros(64, np.int32)
    p32 = z32.ctypes.data_as(C.POINTER(C.c_int32))
    # no key yet: the C entry point and the Python layer both refuse
    assert L.thfhe_pack_lwe(ctx.h, p32, 1, 1, p32, p32) == -1 and b"no packing key" in L.thfhe_last_error()
    with pytest.raises(thfhe.ThfheError):
        T.PackLwe(ctx, np.zeros((1, 11), np.int32))
    # key arguments, checked before the key is read
    assert L.thfhe_pack_key_set(ctx.h, p32, 0, 8, 2) == -1
    assert L.thfhe_pack_key_set(ctx.h, p32, 10, 0, 2) == -1
    assert L.thfhe_pack_key_set(ctx.h, p32, 10, 17, 2) == -1
    assert L.thfhe_pack_key_set(ctx.h, p32, 10, 8, 0) == -1
    assert L.thfhe_pack_key_set(ctx.h, p32, 10, 2, 5) == -2
    assert L.thfhe_pack_key_set(ctx.h, p32, 2049, 8, 2) == -2
    assert L.thfhe_pack_key_set(None, p32, 10, 8, 2) == -1 and L.thfhe_pack_key_set(ctx.h, None, 10, 8, 2) == -1
    rng = np.random.default_rng(13)
    n = 10
    s, z = rng.integers(0, 2, n).astype(np.int32), rng.integers(0, 2, N).astype(np.int32)
    pk2 = keygen.gen_pack_key(rng, s, z, 8, 2, 2.0**-25)
    pk3 = keygen.gen_pack_key(rng, s, z, 5, 3, 2.0**-25)
    ctx.set_pack_key(pk2, 8, 2)
    x = _lwe(rng, 70, n)
    for slots in (0, -1, N + 1):
        with pytest.raises(thfhe.ThfheError):
            T.PackLwe(ctx, x, slots)
    assert L.thfhe_pack_lwe(ctx.h, p32, 1, 1, None, p32) == -1
    with pytest.raises(ValueError):
        ctx.set_pack_key(pk2[:, :, :2], 8, 2)
    a, b = T.PackLwe(ctx, x, 32)
    ra, rb = PR.pack(x, pk2, 8, 2, 32)
    assert np.array_equal(a, ra) and np.array_equal(b, rb)
    # a refused key leaves the earlier one; a new key replaces it, planes included (3-bit digits have none: the plain kernel at 70)
    assert L.thfhe_pack_key_set(ctx.h, pk3.ctypes.data_as(C.POINTER(C.c_int32)), n, 5, 5) == -2
    a, b = T.PackLwe(ctx, x, 32)
    assert np.array_equal(a, ra) and np.array_equal(b, rb)
    ctx.set_pack_key(pk3, 5, 3)
    a, b = T.PackLwe(ctx, x, 32)
    ra, rb = PR.pack(x, pk3, 5, 3, 32)
    assert np.array_equal(a, ra) and np.array_equal(b, rb)
    assert T.PackLwe(ctx, x[:0], 32)[0].shape == (0, N)
    ctx.close()
