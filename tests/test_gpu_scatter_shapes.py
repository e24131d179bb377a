"""Leveled scatter on every parameter shape (pytest -m gpu): the seven shapes of support.py -- l = 1 .. 4 and the Bgbit of
each -- on sk_lhe_demux_kernel, sk_lhe_scatter_rotate_kernel and sk_lhe_scatter_sum_kernel, every word against the model composed from the CPU
oracle's exact pieces (scatter_reference.py on lhe_reference.py).

  (1) thfhe_lhe_demux on 5 samples with random-word TGSW samples and random-word x, encrypted and trivial (the PUB kernel);
  (2) thfhe_lhe_scatter on 11 samples at (d_tree, d_rot) = (0, 2), (2, 0), (3, 2), (1, 10) -- rotation only, tree only (the first level reads the
      values, PUB when they are trivial), both, and box = 1 with the largest shift N - 1 --, encrypted and trivial values: one value per sample,
      a val_index over 3 values, a table_index over 3 tables of which one receives nothing, a call cut into slices of 4 samples, a window;
  (3) (6, 0) on the shape of SK-128 with 2 samples: the deepest tree, the in-place slots at full depth;
  (4) noiseless TGSW samples with a zero mask and exactly representable values on every address of d = 4, against numpy alone.

The inputs of (1) - (3) are random words, not valid ciphertexts; the contract is word equality."""
import numpy as np
import pytest

import lhe_reference as LR
import lut_reference as R
import scatter_reference as SR
from support import N, SHAPES, differing, pmap, shape_env, shape_id, words

pytestmark = pytest.mark.gpu

CONFIGS = [(0, 2), (2, 0), (3, 2), (1, 10)]
COUNT = 11


@pytest.fixture(scope="module")
def env(O):
    yield from shape_env(O)


@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_demux_every_word(env, shape):
    p, K, orc, ck = env(shape)
    rng = np.random.default_rng(150 + SHAPES.index(shape))
    d, count = 3, 5
    Cs, x = words(rng, count, d, 2 * p.l, 2, N), words(rng, count, 2 * N)
    with ck.tgsw_set(Cs, d) as ts:
        for bit in (0, 2):
            for kind, xs in (("enc", x), ("pub", SR.trivial(x[:, N:]))):
                ref = pmap(lambda s: SR.demux(p, Cs[s][bit], xs[s]), range(count))
                ref0, ref1 = np.stack([r[0] for r in ref]), np.stack([r[1] for r in ref])
                o0a, o0b, o1a, o1b = ck.lhe_demux(ts, bit, xs[:, N:], x_a=xs[:, :N] if kind == "enc" else None)
                got0, got1 = np.concatenate([o0a, o0b], axis=1), np.concatenate([o1a, o1b], axis=1)
                assert np.array_equal(got1, ref1), (bit, kind, differing(got1, ref1))
                assert np.array_equal(got0, ref0), (bit, kind, differing(got0, ref0))
                assert np.array_equal(LR._add(got0, got1), xs)


_cache = {}


def case(p, shape, cfg, count=COUNT):
    """inputs and model leaves of one (shape, config): TGSW words, 3 values, the value and table index, leaves[kind] int32[count][2^d_tree][2N]"""
    key = (shape, cfg, count)
    if key not in _cache:
        d_tree, d_rot = cfg
        d = d_tree + d_rot
        rng = np.random.default_rng(2000 * SHAPES.index(shape) + 100 * d_tree + d_rot)
        Cs = words(rng, count, d, 2 * p.l, 2, N)
        vals = words(rng, 3, 2 * N)
        vidx = ((np.arange(count) + 1) % 3).astype(np.int32)
        tidx = (2 * (np.arange(count) % 2)).astype(np.int32)     # tables 0 and 2: table 1 receives nothing
        leaves = {"enc": np.stack(pmap(lambda s: SR.scatter_wo_reduce(p, Cs[s], vals[vidx[s]], d_tree, d_rot), range(count))),
                  "pub": np.stack(pmap(lambda s: SR.scatter_wo_reduce(p, Cs[s], SR.trivial(vals[vidx[s]][N:]), d_tree, d_rot), range(count)))}
        _cache[key] = (Cs, vals, vidx, tidx, leaves)
    return _cache[key]


def summed(leaves, tidx=None, n_tables=1):
    tab = np.zeros((n_tables,) + leaves.shape[1:], np.int64)
    for s in range(leaves.shape[0]):
        tab[0 if tidx is None else tidx[s]] += leaves[s]
    return tab.astype(np.uint32).view(np.int32)


def check(got, ref, what):
    tab = np.concatenate(got, axis=2)
    assert tab.shape == ref.shape, what
    assert np.array_equal(tab, ref), (what, differing(tab, ref))


@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: "tree%d-rot%d" % c)
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_scatter_every_word(env, shape, cfg):
    p, K, orc, ck = env(shape)
    d_tree, d_rot = cfg
    Cs, vals, vidx, tidx, leaves = case(p, shape, cfg)
    assert sorted(set(vidx.tolist())) == [0, 1, 2] and sorted(set(tidx.tolist())) == [0, 2] and len(set(tidx[4:9].tolist())) == 2
    kw = dict(d_tree=d_tree, d_rot=d_rot)
    with ck.tgsw_set(Cs, d_tree + d_rot) as ts:
        for kind in ("enc", "pub"):
            va, vb = (vals[:, :N], vals[:, N:]) if kind == "enc" else (None, vals[:, N:])
            one, three = summed(leaves[kind]), summed(leaves[kind], tidx, 3)
            assert not three[1].any()
            # one value per sample (n_vals == count, no index), one table
            check(ck.lhe_scatter(ts, vb[vidx], val_a=None if va is None else va[vidx], **kw), one, (kind, "value per sample"))
            # 3 values through val_index, 3 tables through table_index
            whole = ck.lhe_scatter(ts, vb, val_a=va, val_index=vidx, n_tables=3, table_index=tidx, **kw)
            check(whole, three, (kind, "indices"))
            # a window of the set: first != 0, the index arrays follow the window
            win = ck.lhe_scatter(ts, vb, val_a=va, val_index=vidx[4:9], n_tables=3, table_index=tidx[4:9], first=4, count=5, **kw)
            check(win, summed(leaves[kind][4:9], tidx[4:9], 3), (kind, "window"))
            try:
                ck.set_tree_slice(4 << d_tree)      # 2^d_tree TLWE of workspace per sample: slices of 4 + 4 + 3 samples
                cut = ck.lhe_scatter(ts, vb, val_a=va, val_index=vidx, n_tables=3, table_index=tidx, **kw)
                assert np.array_equal(cut[0], whole[0]) and np.array_equal(cut[1], whole[1]), (kind, "slices")
                check(ck.lhe_scatter(ts, vb[vidx], val_a=None if va is None else va[vidx], **kw), one, (kind, "value per sample, slices"))
            finally:
                ck.set_tree_slice(65536)


def test_deepest_tree_on_the_shape_of_sk128(env):
    shape = SHAPES[2]
    assert shape[1:3] == (3, 7)      # l, Bgbit of SK-128
    p, K, orc, ck = env(shape)
    Cs, vals, vidx, tidx, leaves = case(p, shape, (6, 0), count=2)
    with ck.tgsw_set(Cs, 6) as ts:
        for kind in ("enc", "pub"):
            got = ck.lhe_scatter(ts, vals[:, N:], val_a=vals[:, :N] if kind == "enc" else None, val_index=vidx, d_tree=6, d_rot=0)
            check(got, summed(leaves[kind]), kind)
            try:
                ck.set_tree_slice(1)      # below one sample's workspace: slices of one sample
                cut = ck.lhe_scatter(ts, vals[:, N:], val_a=vals[:, :N] if kind == "enc" else None, val_index=vidx, d_tree=6, d_rot=0)
                assert np.array_equal(cut[0], got[0]) and np.array_equal(cut[1], got[1]), kind
            finally:
                ck.set_tree_slice(65536)


@pytest.mark.parametrize("cfg", [(2, 2), (0, 4), (4, 0)], ids=lambda c: "tree%d-rot%d" % c)
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_noiseless_samples_on_every_address_of_d4(env, shape, cfg):
    p, K, orc, ck = env(shape)
    d_tree, d_rot = cfg
    box = N >> d_rot
    rng = np.random.default_rng(170 + SHAPES.index(shape))
    bits = p.l * p.Bgbit
    f = R.to_i32(rng.integers(1, 1 << bits, 3, dtype=np.int64) << (32 - bits))      # words the decomposition represents exactly
    v = np.zeros((1, N), np.int32)
    v[0, :3] = f
    addr = rng.permutation(16)
    with ck.tgsw_set(LR.trivial_tgsw(p, LR.address_bits(addr, 4)), 4) as ts:
        # one value for all (n_vals = 1), a table of its own for every sample: table s holds f at address addr[s] and nothing else
        tab_a, tab_b = ck.lhe_scatter(ts, v, d_tree=d_tree, d_rot=d_rot, n_tables=16, table_index=np.arange(16))
        assert tab_a.shape == tab_b.shape == (16, 1 << d_tree, N) and not tab_a.any()
        want = np.zeros((16, 1 << d_tree, N), np.int32)
        for s, a in enumerate(addr):
            want[s, a >> d_rot, (a & ((1 << d_rot) - 1)) * box:][:3] = f
        assert np.array_equal(tab_b, want), differing(tab_b, want)
        # all into one table: every entry holds f; as an encrypted value with a zero mask the same words come out
        one_a, one_b = ck.lhe_scatter(ts, v, val_a=np.zeros_like(v), d_tree=d_tree, d_rot=d_rot)
        assert not one_a.any() and np.array_equal(one_b[0], want.astype(np.int64).sum(axis=0).astype(np.uint32).view(np.int32))
