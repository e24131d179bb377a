"""Leveled table lookup without a GPU: the model of lhe_reference.py decrypts every address of a small table under real
keys, the layout helpers of thfhe.lut agree with the model's, SecretKeySet.tgsw_encrypt is the bootstrapping key's code path, every host check of
the C entry points answers before a context is looked at, and noiseless TGSW samples select exactly the addressed entry."""
import ctypes as C

import numpy as np
import pytest

import lhe_reference as LR
import lut_reference as R
from support import words

N = 1024


@pytest.fixture(scope="module")
def small():
    """n = 16 key set of the product's key generator (its TGSW encryption is what a client runs), the oracle on its tables"""
    import oracle_lib as O
    import thfhe
    from thfhe import keygen
    kw = dict(thfhe.PARAM_SETS["SK-128"], n=16)
    K = keygen.SecretKeySet(thfhe.make_params(**kw), seed=77)
    p = O.make_params(**kw)
    return p, K, O.Oracle(p, K.bk, K.ksk)


def test_model_decrypts_every_address_of_a_2_plus_2_table(small):
    from thfhe import lut
    p, K, orc = small
    d_tree, d_rot, theta, p_out = 2, 2, 2, 8
    rng = np.random.default_rng(5)
    f = rng.integers(0, p_out, (theta, 16))
    tab_b = lut.lhe_table(f, d_tree, d_rot, theta, encode=lambda v: lut.encode(v, p_out))
    tab_a, tab_eb = lut.encrypt_table(K.rlwe_key, tab_b, 2.0**-25, rng)
    addr = np.arange(16)
    Cs = K.tgsw_encrypt(lut.lhe_address_bits(addr, 4), seed=9).reshape(16, 4, 2 * p.l, 2, N)
    for a in addr:
        for ta, tb in ((None, tab_b), (tab_a, tab_eb)):
            u = LR.lookup(orc, Cs[a], ta, tb, d_tree, d_rot, theta, keyswitch=False)
            assert np.array_equal(lut.decode(K.ring_phase(u), p_out), f[:, a]), a
            ks = np.stack([orc.keyswitch(r) for r in u])
            assert np.array_equal(lut.decode(K.phase(ks), p_out), f[:, a]), a


@pytest.mark.parametrize("shape", [(0, 1, 1), (1, 0, 1), (2, 3, 4), (6, 2, 1), (0, 10, 1), (3, 8, 4), (6, 10, 1)])
def test_table_layout_and_address_bits(shape):
    from thfhe import lut
    d_tree, d_rot, theta = shape
    rng = np.random.default_rng(sum(shape))
    F = words(rng, theta, 1 << (d_tree + d_rot))
    tab = lut.lhe_table(F, d_tree, d_rot, theta)
    assert tab.shape == (1 << d_tree, N) and np.array_equal(tab, LR.table_polys(F, d_tree, d_rot))
    box = N >> d_rot
    e = int(rng.integers(0, F.shape[1]))
    for j in range(theta):
        assert tab[e >> d_rot, (e & ((1 << d_rot) - 1)) * box + j] == F[j, e]
    d = d_tree + d_rot
    addr = rng.integers(0, 1 << d, 9)
    bits = lut.lhe_address_bits(addr, d)
    assert bits.shape == (9 * d,) and np.array_equal(bits.reshape(9, d), LR.address_bits(addr, d))
    assert np.array_equal((bits.reshape(9, d) << np.arange(d)).sum(axis=1), addr)


def test_layout_helpers_reject_bad_arguments():
    from thfhe import lut
    with pytest.raises(ValueError):
        lut.lhe_table(np.zeros((1, 2)), 7, 0)
    with pytest.raises(ValueError):
        lut.lhe_table(np.zeros((4, 1024)), 0, 10, 4)       # theta 4 > box 1
    with pytest.raises(ValueError):
        lut.lhe_table(np.zeros((1, 5)), 1, 1)
    with pytest.raises(ValueError):
        lut.lhe_address_bits([16], 4)
    with pytest.raises(ValueError):
        lut.lhe_address_bits([0], 17)


def test_tgsw_encrypt_of_the_lwe_key_reproduces_bk(small):
    p, K, orc = small
    rng = np.random.default_rng(77)
    assert np.array_equal(rng.integers(0, 2, p.n).astype(np.int32), K.lwe_key)     # the generator state at which __init__ encrypts the key
    assert np.array_equal(rng.integers(0, 2, p.N).astype(np.int32), K.rlwe_key)
    assert np.array_equal(K._tgsw_encrypt(rng, K.lwe_key), K.bk)
    one = K.tgsw_encrypt([1, 0], seed=3)
    assert one.shape == (2, 2 * p.l, 2, N) and np.array_equal(one, K.tgsw_encrypt([1, 0], seed=3))
    # rows decrypt to bit * gadget on coefficient 0 of their own polynomial (mask rows: -z times it), noise below 2^-20
    ph = K.tlwe_phase(one[:, :, 0, :], one[:, :, 1, :]).astype(np.int64)
    for lv in range(p.l):
        g = 1 << (32 - (lv + 1) * p.Bgbit)
        want = np.zeros(N, np.int64)
        want[0] = g
        assert np.abs(ph[1, p.l + lv]).max() < 1 << 12
        assert np.abs(((ph[0, p.l + lv] - want + 2**31) % 2**32) - 2**31).max() < 1 << 12


def test_trivial_tgsw_samples_select_exactly_the_addressed_entry(small):
    p, K, orc = small
    d_tree, d_rot, theta = 2, 3, 4
    rng = np.random.default_rng(11)
    unit = 1 << (32 - p.l * p.Bgbit)                    # words the decomposition represents exactly
    F = R.to_i32(rng.integers(0, 1 << (p.l * p.Bgbit), (theta, 32)) * unit)
    tab = LR.table_polys(F, d_tree, d_rot)
    for a in (0, 1, 7, 8, 21, 31):
        Cs = LR.trivial_tgsw(p, LR.address_bits([a], 5)[0])
        u = LR.lookup_wo_keyswitch(p, Cs, None, tab, d_tree, d_rot, theta)
        assert not u[:, :N].any() and np.array_equal(u[:, N], F[:, a]), a


def _err(L):
    return L.thfhe_last_error().decode()


def test_every_host_check_answers_without_a_context():
    import thfhe
    L = thfhe.lib()
    i32p = C.POINTER(C.c_int32)
    buf = np.zeros(4 * N, np.int32)
    b = buf.ctypes.data_as(i32p)
    h = C.c_void_p()
    INV = -1
    # thfhe_tgsw_set_create
    assert L.thfhe_tgsw_set_create(None, None, 1, 1, C.byref(h)) == INV and "null argument" in _err(L)
    assert L.thfhe_tgsw_set_create(None, b, 1, 1, None) == INV and "null argument" in _err(L)
    for d in (0, -1, 17):
        assert L.thfhe_tgsw_set_create(None, b, 1, d, C.byref(h)) == INV and "d must be" in _err(L)
    for count in (0, (1 << 24) + 1):
        assert L.thfhe_tgsw_set_create(None, b, count, 4, C.byref(h)) == INV and "count must be" in _err(L)
    assert L.thfhe_tgsw_set_create(None, b, 1, 16, C.byref(h)) == INV and "null ctx" in _err(L) and not h.value
    L.thfhe_tgsw_set_destroy(None)
    # thfhe_lhe_cmux
    for hole in range(6):
        args = [b] * 6
        args[hole] = None
        assert L.thfhe_lhe_cmux(None, None, 0, *args, 1) == INV and "null argument" in _err(L)
    for bit in (-1, 16):
        assert L.thfhe_lhe_cmux(None, None, bit, b, b, b, b, b, b, 1) == INV and "bit must be" in _err(L)
    assert L.thfhe_lhe_cmux(None, None, 0, b, b, b, b, b, b, 1) == INV and "null tgsw set" in _err(L)
    # thfhe_lhe_lookup and _wo_keyswitch
    idx = np.array([0, 3], np.int32).ctypes.data_as(i32p)
    for fn in (L.thfhe_lhe_lookup, L.thfhe_lhe_lookup_wo_keyswitch):
        call = lambda d_tree=1, d_rot=1, theta=1, tab_b=b, n_tables=1, index=None, out=b, count=2: \
            fn(None, None, 0, count, d_tree, d_rot, theta, None, tab_b, n_tables, index, out)
        assert call(tab_b=None) == INV and "null argument" in _err(L)
        assert call(out=None) == INV and "null argument" in _err(L)
        for v in (-1, 7):
            assert call(d_tree=v) == INV and "d_tree" in _err(L)
        for v in (-1, 11):
            assert call(d_rot=v) == INV and "d_rot" in _err(L)
        for v in (0, 3, 8):
            assert call(theta=v) == INV and "theta must be 1, 2 or 4" in _err(L)
        assert call(d_rot=9, theta=4) == INV and "box" in _err(L)
        assert call(d_rot=10, theta=2) == INV and "box" in _err(L)
        assert call(n_tables=0) == INV and "n_tables" in _err(L)
        assert call(d_tree=6, n_tables=4097) == INV and "n_tables" in _err(L)
        assert call(n_tables=3, index=idx) == INV and "table_index out of range" in _err(L)
        assert call() == INV and "null tgsw set" in _err(L)
        assert call(count=0) == INV and "null tgsw set" in _err(L)
