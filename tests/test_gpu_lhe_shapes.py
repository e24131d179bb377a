"""Leveled table lookup on every parameter shape (pytest -m gpu): the seven shapes of support.py -- l = 1 .. 4
and the Bgbit of each -- on sk_lhe_cmux_kernel and sk_lhe_rotate_kernel, every word against the model composed from the CPU oracle's exact
pieces (lhe_reference.py).

  (1) 11 samples with random-word TGSW samples and random-word tables, encrypted and public: thfhe_lhe_cmux, and thfhe_lhe_lookup with and without
      the key switch at (d_tree, d_rot, theta) = (0, 1, 1), (1, 0, 1), (2, 3, 4), (6, 2, 1), (0, 10, 1); a per-sample table index over 3 tables;
      a call cut into slices against the unsliced call; the same at d_tree = 0 -- (0, 3, 4) and (0, 10, 1) --, where the rotation kernel itself
      picks the sample's table;
  (2) noiseless TGSW samples with a zero mask on ALL 1 024 addresses at (0, 10) and all 4 096 at (2, 10), against numpy alone: table words that
      the decomposition represents exactly come out exactly.  The 4 096 addresses go through four sets of 1 024 samples (a set of 4 096 x 12 bits
      is 2.4 .. 3.2 GB of host words at l = 3, 4), each read in two calls, the second with a non-zero `first`.

The inputs of (1) are random words, not valid ciphertexts; the contract is word equality."""
import numpy as np
import pytest

import lhe_reference as LR
import lut_reference as R
from support import N, SHAPES, differing, pmap, shape_env, shape_id, words

pytestmark = pytest.mark.gpu

CONFIGS = [(0, 1, 1), (1, 0, 1), (2, 3, 4), (6, 2, 1), (0, 10, 1)]
COUNT = 11


@pytest.fixture(scope="module")
def env(O):
    yield from shape_env(O)


_cache = {}


def case(p, orc, shape, cfg, n_tables=1):
    """inputs and model outputs of one (shape, config): TGSW words, tables, index, (wo, ks) for the encrypted and the public table"""
    key = (shape, cfg, n_tables)
    if key not in _cache:
        d_tree, d_rot, theta = cfg
        d = d_tree + d_rot
        rng = np.random.default_rng(1000 * SHAPES.index(shape) + 100 * d_tree + 10 * d_rot + theta + n_tables)
        Cs = words(rng, COUNT, d, 2 * p.l, 2, N)
        tab_a, tab_b = words(rng, n_tables, 1 << d_tree, N), words(rng, n_tables, 1 << d_tree, N)
        idx = rng.permutation(np.arange(COUNT) % n_tables).astype(np.int32)
        ref = {}
        for kind in ("enc", "pub"):
            wo = np.stack(pmap(lambda s: LR.lookup_wo_keyswitch(p, Cs[s], tab_a[idx[s]] if kind == "enc" else None, tab_b[idx[s]], d_tree, d_rot, theta),
                               range(COUNT)))
            ks = np.stack(pmap(orc.keyswitch, wo.reshape(-1, N + 1))).reshape(COUNT, theta, -1)
            ref[kind] = (wo, ks)
        _cache[key] = (Cs, tab_a, tab_b, idx, ref)
    return _cache[key]


@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_cmux_every_word(env, shape):
    p, K, orc, ck = env(shape)
    rng = np.random.default_rng(50 + SHAPES.index(shape))
    d = 3
    Cs = words(rng, COUNT, d, 2 * p.l, 2, N)
    d1, d0 = words(rng, COUNT, 2 * N), words(rng, COUNT, 2 * N)
    with ck.tgsw_set(Cs, d) as ts:
        assert (ts.count, ts.d) == (COUNT, d)
        for bit in (0, 2):
            ref = np.stack(pmap(lambda s: LR.cmux(p, Cs[s][bit], d1[s], d0[s]), range(COUNT)))
            a, b = ck.lhe_cmux(ts, bit, d1[:, :N], d1[:, N:], d0[:, :N], d0[:, N:])
            got = np.concatenate([a, b], axis=1)
            assert np.array_equal(got, ref), (bit, differing(got, ref))


@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: "tree%d-rot%d-theta%d" % c)
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_lookup_every_word(env, shape, cfg):
    p, K, orc, ck = env(shape)
    d_tree, d_rot, theta = cfg
    Cs, tab_a, tab_b, idx, ref = case(p, orc, shape, cfg)
    kw = dict(d_tree=d_tree, d_rot=d_rot, theta=theta)
    with ck.tgsw_set(Cs, d_tree + d_rot) as ts:
        for kind in ("enc", "pub"):
            ta = tab_a if kind == "enc" else None
            u = ck.lhe_lookup_wo_keyswitch(ts, tab_b, tab_a=ta, **kw)
            assert u.shape == (COUNT, theta, N + 1)
            assert np.array_equal(u, ref[kind][0]), (kind, differing(u, ref[kind][0]))
            got = ck.lhe_lookup(ts, tab_b, tab_a=ta, **kw)
            assert got.shape == (COUNT, theta, p.n + 1)
            assert np.array_equal(got, ref[kind][1]), (kind, differing(got, ref[kind][1]))


@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_per_sample_table_index_and_slices(env, shape):
    p, K, orc, ck = env(shape)
    cfg = (2, 3, 4)
    Cs, tab_a, tab_b, idx, ref = case(p, orc, shape, cfg, n_tables=3)
    assert len(set(idx.tolist())) == 3
    kw = dict(d_tree=2, d_rot=3, theta=4, table_index=idx)
    with ck.tgsw_set(Cs, 5) as ts:
        whole = {}
        for kind in ("enc", "pub"):
            ta = tab_a if kind == "enc" else None
            whole[kind] = ck.lhe_lookup(ts, tab_b, tab_a=ta, **kw)
            assert np.array_equal(whole[kind], ref[kind][1]), (kind, differing(whole[kind], ref[kind][1]))
            u = ck.lhe_lookup_wo_keyswitch(ts, tab_b, tab_a=ta, **kw)
            assert np.array_equal(u, ref[kind][0]), (kind, differing(u, ref[kind][0]))
            # a window of the set: first != 0, the index array follows the window
            win = ck.lhe_lookup(ts, tab_b, tab_a=ta, d_tree=2, d_rot=3, theta=4, table_index=idx[4:9], first=4, count=5)
            assert np.array_equal(win, ref[kind][1][4:9]), kind
        try:
            ck.set_tree_slice(6)      # 2 TLWE of workspace per sample: slices of 3 samples, the call crosses three boundaries
            for kind in ("enc", "pub"):
                got = ck.lhe_lookup(ts, tab_b, tab_a=tab_a if kind == "enc" else None, **kw)
                assert np.array_equal(got, whole[kind]), (kind, differing(got, whole[kind]))
        finally:
            ck.set_tree_slice(65536)


@pytest.mark.parametrize("cfg", [(0, 3, 4), (0, 10, 1)], ids=lambda c: "tree%d-rot%d-theta%d" % c)
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_flat_rotation_with_per_sample_table_index(env, shape, cfg):
    # d_tree = 0 with a per-sample table index: no tree level runs, so sk_lhe_rotate_kernel itself starts sample s from table table_index[s]
    # (LheRotArgs.src_idx, src_stride = 1024 words, from the uploaded tables directly) -- the one dispatch path of lhe_lookup the cases above
    # do not enter.  At d_tree = 0 a slice holds tree_slice samples, so set_tree_slice(3) cuts the 11 samples into 3 + 3 + 3 + 2 and the index
    # slice is uploaded anew for each.
    p, K, orc, ck = env(shape)
    d_tree, d_rot, theta = cfg
    Cs, tab_a, tab_b, idx, ref = case(p, orc, shape, cfg, n_tables=3)
    assert tab_b.shape == (3, 1, N) and sorted(set(idx.tolist())) == [0, 1, 2] and len(set(idx[4:9].tolist())) > 1
    kw = dict(d_tree=d_tree, d_rot=d_rot, theta=theta)
    with ck.tgsw_set(Cs, d_rot) as ts:
        whole = {}
        for kind in ("enc", "pub"):
            ta = tab_a if kind == "enc" else None
            u = ck.lhe_lookup_wo_keyswitch(ts, tab_b, tab_a=ta, table_index=idx, **kw)
            assert u.shape == (COUNT, theta, N + 1)
            assert np.array_equal(u, ref[kind][0]), (kind, differing(u, ref[kind][0]))
            whole[kind] = ck.lhe_lookup(ts, tab_b, tab_a=ta, table_index=idx, **kw)
            assert whole[kind].shape == (COUNT, theta, p.n + 1)
            assert np.array_equal(whole[kind], ref[kind][1]), (kind, differing(whole[kind], ref[kind][1]))
            # a window of the set: first != 0, the index array follows the window
            win = ck.lhe_lookup_wo_keyswitch(ts, tab_b, tab_a=ta, table_index=idx[4:9], first=4, count=5, **kw)
            assert np.array_equal(win, ref[kind][0][4:9]), (kind, differing(win, ref[kind][0][4:9]))
            win = ck.lhe_lookup(ts, tab_b, tab_a=ta, table_index=idx[4:9], first=4, count=5, **kw)
            assert np.array_equal(win, ref[kind][1][4:9]), (kind, differing(win, ref[kind][1][4:9]))
        try:
            ck.set_tree_slice(3)
            for kind in ("enc", "pub"):
                ta = tab_a if kind == "enc" else None
                got = ck.lhe_lookup(ts, tab_b, tab_a=ta, table_index=idx, **kw)
                assert np.array_equal(got, whole[kind]), (kind, differing(got, whole[kind]))
                u = ck.lhe_lookup_wo_keyswitch(ts, tab_b, tab_a=ta, table_index=idx, **kw)
                assert np.array_equal(u, ref[kind][0]), (kind, differing(u, ref[kind][0]))
        finally:
            ck.set_tree_slice(65536)


def exact_words(rng, p, *shape):
    """words the decomposition represents exactly: multiples of 2^(32 - l Bgbit)"""
    bits = p.l * p.Bgbit
    return R.to_i32(rng.integers(0, 1 << bits, shape, dtype=np.int64) << (32 - bits))


@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_trivial_samples_on_all_1024_addresses(env, shape):
    p, K, orc, ck = env(shape)
    rng = np.random.default_rng(70 + SHAPES.index(shape))
    tab = exact_words(rng, p, 1, N)                              # (0, 10): box = 1, entry e at coefficient e
    addr = rng.permutation(1024)
    with ck.tgsw_set(LR.trivial_tgsw(p, LR.address_bits(addr, 10)), 10) as ts:
        u = np.concatenate([ck.lhe_lookup_wo_keyswitch(ts, tab, d_tree=0, d_rot=10, first=0, count=300),
                            ck.lhe_lookup_wo_keyswitch(ts, tab, d_tree=0, d_rot=10, first=300, count=724)])
    assert u.shape == (1024, 1, N + 1)
    assert not u[:, 0, :N].any()
    bad = np.flatnonzero(u[:, 0, N] != tab[0][addr])
    assert bad.size == 0, ("addresses", addr[bad[:8]].tolist())


@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_trivial_samples_on_all_4096_addresses(env, shape):
    p, K, orc, ck = env(shape)
    rng = np.random.default_rng(90 + SHAPES.index(shape))
    tab_a, tab_b = exact_words(rng, p, 4, N), exact_words(rng, p, 4, N)   # (2, 10): an encrypted table, so the mask is rotated too
    addr = rng.permutation(4096)
    want = np.empty((4096, N + 1), np.int32)
    for e in range(4096):
        acc = np.concatenate([R.monomial(tab_a[e >> 10], -(e & 1023), N), R.monomial(tab_b[e >> 10], -(e & 1023), N)])
        want[e] = R.extract_at(acc, 0, N)
    for q in range(4):
        part = addr[1024 * q:1024 * (q + 1)]
        with ck.tgsw_set(LR.trivial_tgsw(p, LR.address_bits(part, 12)), 12) as ts:
            u = np.concatenate([ck.lhe_lookup_wo_keyswitch(ts, tab_b, tab_a=tab_a, d_tree=2, d_rot=10, first=0, count=512),
                                ck.lhe_lookup_wo_keyswitch(ts, tab_b, tab_a=tab_a, d_tree=2, d_rot=10, first=512, count=512)])
        bad = np.flatnonzero((u[:, 0] != want[part]).any(axis=1))
        assert bad.size == 0, ("addresses", part[bad[:8]].tolist())
