"""Leveled scatter without a GPU: the model of scatter_reference.py against the plain model circuits.lhe_scatter_plain on
noiseless samples, write-then-read through lhe_reference.lookup_wo_keyswitch, the demux identity out0 + out1 = x, the helpers of thfhe.lut and
thfhe.circuits, every host check of the two C entry points with a NULL context, and a 16-sample histogram under real keys on the n = 16 set."""
import ctypes as C

import numpy as np
import pytest

import lhe_reference as LR
import lut_reference as R
import scatter_reference as SR
from support import words

N = 1024


def exact_words(rng, p, *shape):
    """words the decomposition represents exactly: multiples of 2^(32 - l Bgbit)"""
    bits = p.l * p.Bgbit
    return R.to_i32(rng.integers(0, 1 << bits, shape, dtype=np.int64) << (32 - bits))


@pytest.mark.parametrize("cfg", [(0, 3), (3, 0), (2, 2)], ids=lambda c: "tree%d-rot%d" % c)
def test_noiseless_model_equals_the_plain_model_on_every_address(sk_small, cfg):
    from thfhe import circuits
    p, K, orc = sk_small
    d_tree, d_rot = cfg
    d = d_tree + d_rot
    box = N >> d_rot
    rng = np.random.default_rng(10 * d_tree + d_rot)
    v = np.zeros((2, N), np.int32)
    v[:, :min(box, 4)] = exact_words(rng, p, 2, min(box, 4))
    for addr in range(1 << d):
        Cs = LR.trivial_tgsw(p, LR.address_bits([addr], d)[0])
        tab = SR.scatter(p, Cs[None], SR.trivial(v[addr & 1]), d_tree, d_rot)
        assert tab.shape == (1, 1 << d_tree, 2 * N) and not tab[..., :N].any()
        want = circuits.lhe_scatter_plain([addr], v[addr & 1], d_tree, d_rot)
        assert np.array_equal(tab[..., N:], want), addr
        # ... and the plain model is the layout of lut.lhe_table
        assert want[0, addr >> d_rot, (addr & ((1 << d_rot) - 1)) * box] == v[addr & 1][0] and np.count_nonzero(want) == np.count_nonzero(v[addr & 1])


def test_plain_model_sums_indices_and_tables():
    from thfhe import circuits, lut
    rng = np.random.default_rng(3)
    d_tree, d_rot = 2, 3
    addr = np.array([5, 5, 31, 0, 17, 5])
    f = rng.integers(1, 1000, (3, 2))
    vals = lut.lhe_value(f)
    vi, ti = np.array([0, 1, 2, 2, 1, 0]), np.array([0, 0, 2, 0, 2, 2])
    tab = circuits.lhe_scatter_plain(addr, vals, d_tree, d_rot, val_index=vi, n_tables=3, table_index=ti)
    assert tab.shape == (3, 4, N) and not tab[1].any()
    want = np.zeros((3, 2, 32), np.int64)
    for a, v, t in zip(addr, vi, ti):
        want[t, :, a] += f[v]
    for t in range(3):
        assert np.array_equal(lut.lhe_table_entries(tab[t], d_tree, d_rot, theta=2), want[t])
        assert np.array_equal(tab[t], lut.lhe_table(want[t], d_tree, d_rot, theta=2))
    # one value for every sample; one value per sample
    assert np.array_equal(circuits.lhe_scatter_plain(addr, vals[1], d_tree, d_rot), circuits.lhe_scatter_plain(addr, vals, d_tree, d_rot, val_index=[1] * 6))
    assert np.array_equal(circuits.lhe_scatter_plain(addr[:3], vals, d_tree, d_rot), circuits.lhe_scatter_plain(addr[:3], vals, d_tree, d_rot, val_index=[0, 1, 2]))
    # the shift is negacyclic: a value that reaches past N comes back negated (documented spill, unchecked by the library)
    top = np.zeros(N, np.int64)
    top[N - 1] = 7
    assert circuits.lhe_scatter_plain([1], top, 0, 1)[0, 0, N // 2 - 1] == -7
    with pytest.raises(ValueError):
        circuits.lhe_scatter_plain([32], vals[0], d_tree, d_rot)
    with pytest.raises(ValueError):
        circuits.lhe_scatter_plain([0, 1], vals, d_tree, d_rot)      # three values for two addresses, no index


def test_write_then_read_returns_the_value_at_its_address_only(sk_small):
    p, K, orc = sk_small
    d_tree, d_rot = 2, 2
    rng = np.random.default_rng(21)
    v = np.zeros(N, np.int32)
    v[:2] = exact_words(rng, p, 2)
    for addr in (0, 6, 15):
        tab = SR.scatter(p, LR.trivial_tgsw(p, LR.address_bits([addr], 4)[0])[None], SR.trivial(v), d_tree, d_rot)[0]
        for other in range(16):
            u = LR.lookup_wo_keyswitch(p, LR.trivial_tgsw(p, LR.address_bits([other], 4)[0]), tab[:, :N], tab[:, N:], d_tree, d_rot, 2)
            assert not u[:, :N].any()
            assert np.array_equal(u[:, N], v[:2] if other == addr else [0, 0]), (addr, other)


def test_children_sum_to_the_input_word_for_word(sk_small):
    p, K, orc = sk_small
    rng = np.random.default_rng(22)
    for _ in range(2):
        Cw, x = words(rng, 2 * p.l, 2, N), words(rng, 2 * N)
        c0, c1 = SR.demux(p, Cw, x)
        assert np.array_equal(LR._add(c0, c1), x)
        assert np.array_equal(c1, LR.extern_mul(p, Cw, x))
    leaves = SR.scatter_wo_reduce(p, words(rng, 3, 2 * p.l, 2, N), x, 2, 1)
    assert leaves.shape == (4, 2 * N)
    assert np.array_equal(SR.rotate_chain_up(p, None, x, 0), x)      # d_rot = 0: the chain is the identity


def test_value_and_entry_helpers():
    from thfhe import lut
    v = lut.lhe_value([3, -1, 5])
    assert v.shape == (N,) and v.dtype == np.int32 and v[:3].tolist() == [3, -1, 5] and not v[3:].any()
    v = lut.lhe_value([[1, 2], [3, 0]], encode=lambda m: lut.encode(m, 8))
    assert v.shape == (2, N) and np.array_equal(v[:, :2], lut.encode([[1, 2], [3, 0]], 8)) and not v[:, 2:].any()
    assert lut.lhe_value(7).tolist() == [7] + [0] * (N - 1)
    for bad in (np.zeros((1, 1, 1)), np.zeros(N + 1), np.zeros((2, 0))):
        with pytest.raises(ValueError):
            lut.lhe_value(bad)
    rng = np.random.default_rng(1)
    for d_tree, d_rot, theta in [(0, 10, 1), (6, 0, 4), (2, 4, 2)]:
        F = words(rng, theta, 1 << (d_tree + d_rot))
        assert np.array_equal(lut.lhe_table_entries(lut.lhe_table(F, d_tree, d_rot, theta), d_tree, d_rot, theta), F)
    with pytest.raises(ValueError):
        lut.lhe_table_entries(np.zeros((1, N)), 0, 10, theta=2)


class ModelKey:
    """a stand-in for CloudKey whose lhe_scatter answers from the model: circuits.lhe_histogram runs on it without a device"""
    def __init__(self, p, Cs):
        import thfhe
        self.p, self.Cs, self.params = p, Cs, thfhe.make_params(**dict(thfhe.PARAM_SETS["SK-128"], n=p.n))

    def lhe_scatter(self, tset, val_b, *, d_tree, d_rot, **kw):
        assert tset is self.Cs and not kw
        tab = SR.scatter(self.p, self.Cs, SR.trivial(val_b), d_tree, d_rot)
        return tab[..., :N], tab[..., N:]


@pytest.fixture(scope="module")
def small():
    """the n = 16 set of sk_small's parameters under the product's key generator: its TGSW encryption is what a client runs"""
    import oracle_lib as O
    import thfhe
    from thfhe import keygen
    kw = dict(thfhe.PARAM_SETS["SK-128"], n=16)
    return O.make_params(**kw), keygen.SecretKeySet(thfhe.make_params(**kw), seed=77)


def test_model_decrypts_every_slot_of_a_16_sample_histogram(small):
    from thfhe import circuits, lut
    p, K = small
    d_tree, d_rot, p_out = 2, 2, 8
    rng = np.random.default_rng(31)
    addr = np.concatenate([[3, 3, 3, 3, 3, 0, 15], rng.integers(0, 16, 9)])
    counts = np.bincount(addr, minlength=16)
    assert counts.max() < p_out and (counts == 0).any()
    Cs = K.tgsw_encrypt(lut.lhe_address_bits(addr, 4), seed=32).reshape(16, 4, 2 * p.l, 2, N)
    tab_a, tab_b = circuits.lhe_histogram(ModelKey(p, Cs), Cs, p_out, d_tree, d_rot)
    assert tab_a.shape == tab_b.shape == (1, 4, N)
    ph = K.tlwe_phase(tab_a[0], tab_b[0])
    assert np.array_equal(lut.decode(lut.lhe_table_entries(ph, d_tree, d_rot)[0], p_out), counts)
    # every other coefficient of the table encrypts zero
    want = circuits.lhe_scatter_plain(addr, lut.lhe_value([1], encode=lambda v: lut.encode(v, p_out)), d_tree, d_rot)[0]
    err = (ph.astype(np.int64) - want + 2**31) % 2**32 - 2**31
    assert np.abs(err).max() < 2**32 // (4 * p_out)


def _err(L):
    return L.thfhe_last_error().decode()


def test_every_host_check_answers_without_a_context():
    import thfhe
    L = thfhe.lib()
    i32p = C.POINTER(C.c_int32)
    buf = np.zeros(4 * N, np.int32)
    b = buf.ctypes.data_as(i32p)
    INV = -1
    # thfhe_lhe_demux: x_a may be NULL (trivial samples), the other five may not
    for hole in range(1, 6):
        args = [b] * 6
        args[hole] = None
        assert L.thfhe_lhe_demux(None, None, 0, *args, 1) == INV and "null argument" in _err(L)
    for bit in (-1, 16):
        assert L.thfhe_lhe_demux(None, None, bit, b, b, b, b, b, b, 1) == INV and "bit must be" in _err(L)
    assert L.thfhe_lhe_demux(None, None, 0, b, b, b, b, b, b, 1) == INV and "null tgsw set" in _err(L)
    assert L.thfhe_lhe_demux(None, None, 0, None, b, b, b, b, b, 0) == INV and "null tgsw set" in _err(L)
    # thfhe_lhe_scatter, in the documented order
    bad = np.array([0, 3], np.int32).ctypes.data_as(i32p)
    ok = np.array([0, 1], np.int32).ctypes.data_as(i32p)

    def call(d_tree=1, d_rot=1, val_a=None, val_b=b, n_vals=1, val_index=None, n_tables=1, table_index=None, tab_a=b, tab_b=b, count=2):
        return L.thfhe_lhe_scatter(None, None, 0, count, d_tree, d_rot, val_a, val_b, n_vals, val_index, n_tables, table_index, tab_a, tab_b)
    for hole in ("val_b", "tab_a", "tab_b"):
        assert call(**{hole: None}) == INV and "null argument" in _err(L)
    for v in (-1, 7):
        assert call(d_tree=v) == INV and "d_tree" in _err(L)
    for v in (-1, 11):
        assert call(d_rot=v) == INV and "d_rot" in _err(L)
    assert call(n_tables=0) == INV and "n_tables" in _err(L)
    assert call(d_tree=6, n_tables=4097) == INV and "n_tables" in _err(L)
    for v in (0, -1, (1 << 24) + 1):
        assert call(n_vals=v) == INV and "n_vals" in _err(L)
    assert call(n_vals=3, val_index=bad) == INV and "val_index out of range" in _err(L)
    assert call(n_vals=3) == INV and "n_vals must be 1 or count" in _err(L)          # no index: one value, or one per sample
    assert call(n_vals=3, count=0) == INV and "n_vals must be 1 or count" in _err(L)
    assert call(n_tables=3, table_index=bad) == INV and "table_index out of range" in _err(L)
    # a range error comes before an index error of the later argument, and both before the set
    assert call(d_tree=7, n_vals=3, val_index=bad) == INV and "d_tree" in _err(L)
    assert call(n_vals=2, val_index=bad, n_tables=3, table_index=bad) == INV and "val_index" in _err(L)
    for kw in (dict(), dict(n_vals=2), dict(n_vals=2, val_index=ok, n_tables=2, table_index=ok), dict(count=0)):
        assert call(**kw) == INV and "null tgsw set" in _err(L)
    assert not buf.any()
