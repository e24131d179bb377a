"""tests/support.py itself (no GPU): the word generator draws what the expressions it replaced drew, the index helper keeps its promise, the
kernel-name and shape tables hold what the sweeps rely on, and importing the module does not load the engine."""
import os
import subprocess
import sys

import numpy as np

import support as S


def test_words_draws_what_both_legacy_expressions_drew():
    got = S.words(np.random.default_rng(7), 3, 5)
    assert got.dtype == np.int32 and got.shape == (3, 5)
    assert np.array_equal(got, np.random.default_rng(7).integers(-2**31, 2**31, size=(3, 5), dtype=np.int64).astype(np.int32))
    assert np.array_equal(got, np.random.default_rng(7).integers(-2**31, 2**31, (3, 5)).astype(np.int32))
    # the stream is consumed identically: the draws that follow agree too
    a, b = np.random.default_rng(7), np.random.default_rng(7)
    S.words(a, 3, 5)
    b.integers(-2**31, 2**31, (3, 5))
    assert np.array_equal(S.words(a, 4), b.integers(-2**31, 2**31, 4).astype(np.int32))
    assert S.words(np.random.default_rng(7), 1024).shape == (1024,)


def test_spread_index_uses_every_table_and_differs_between_the_split_launches():
    # the split case runs jobs 0 .. 5 on the four-wave ring and jobs 6 .. 10 in a second launch; both callers assert
    # not array_equal(idx[:5], idx[6:]): the second launch's five indices, in order, are not the first five of the first launch
    idx = S.spread_index(np.random.default_rng(0), 11, 3)
    assert idx.dtype == np.int32 and sorted(set(idx.tolist())) == [0, 1, 2]
    assert sorted(idx.tolist()) == sorted((np.arange(11) % 3).tolist())
    assert not np.array_equal(idx[:5], idx[6:])
    for seed in range(20):
        assert set(S.spread_index(np.random.default_rng(seed), 11, 4).tolist()) == {0, 1, 2, 3}


def test_kernel_table_formats_for_every_l():
    assert len({k[0] for k in S.KERNELS}) == len(S.KERNELS) == 4
    for _, coop, ring4, name in S.KERNELS:
        assert coop >= 0 and ring4 >= 0
        for l in (1, 2, 3, 4):
            assert "<%d" % l in name.format(l=l)
    assert (S.DEFAULT_COOP, S.DEFAULT_RING4) == (768, 1024)


def test_shapes_cover_what_the_sweeps_rely_on():
    assert len(S.SHAPES) == 7 and {s[1] for s in S.SHAPES} == {1, 2, 3, 4}
    assert any(s[0] == 1 for s in S.SHAPES) and any(s[0] % 4 for s in S.SHAPES if s[0] > 1)
    assert [s[1] for s in S.SHAPES[:4]] == [1, 2, 3, 4]           # test_gpu_tree_mvk takes this prefix
    assert len({S.shape_id(s) for s in S.SHAPES}) == 7 and S.shape_id(S.SHAPES[0]) == "n24-l1-Bg8-ks8x2"


def test_importing_support_does_not_load_the_engine():
    here = os.path.dirname(os.path.abspath(__file__))
    pkg = os.path.join(os.path.dirname(here), "torus-fhe_amd")
    code = "import sys; sys.path[:0] = [%r, %r]; import support; assert 'thfhe' not in sys.modules; print('ok')" % (here, pkg)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, check=True)
    assert out.stdout.strip() == "ok"
