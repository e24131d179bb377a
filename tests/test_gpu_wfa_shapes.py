"""Layered automata on every decomposition length (pytest -m gpu): sk_lhe_wfa_step_kernel<l, PUB> and the extract kernel at
(l, Bgbit) = (1, 8), (2, 10), (3, 7), (4, 8) -- the first four shapes of support.py -- on 3 samples of random words, every output word against the
model built from the CPU oracle's exact pieces (wfa_reference.py).  The inputs are random words, not valid ciphertexts; the contract is word
equality.

The automaton of `general` has 5 states and 4 steps over two sets of different d (2 and 3 bits): steps 0 and 2 read the same bit; layers 0, 2
and 3 move the states by a permutation per bit value, layer 1 has two copy states and a state three others move to (it is no permutation).  Its
last three steps alone, on step bits that again read one bit twice (steps 0 and 2 of the three), are the odd-step-count case: the layer buffers
alternate, so a wrong parity shows at one of the two counts."""
import numpy as np
import pytest

import wfa_reference as WR
from support import N, SHAPES, differing, shape_env, shape_id, words

pytestmark = pytest.mark.gpu

WFA_SHAPES = SHAPES[:4]
COUNT, STATES = 3, 5
TRANS = np.array([
    [[1, 2], [2, 3], [3, 4], [4, 0], [0, 1]],      # a permutation per bit value
    [[0, 1], [2, 2], [3, 1], [4, 1], [1, 1]],      # state 1: target of states 0, 2, 3 on bit 1 (and of 4); states 1 and 4 are copies
    [[4, 3], [3, 2], [2, 1], [1, 0], [0, 4]],      # another permutation
    [[0, 4], [1, 3], [2, 0], [3, 1], [4, 2]],      # reads the finals
], np.int32)
STEP_BIT = np.array([16 * 1 + 2, 16 * 0 + 1, 16 * 1 + 2, 16 * 0 + 0], np.int32)   # sets 1, 0, 1, 0; bit 2 of set 1 twice
STEP_BIT3 = np.array([16 * 0 + 1, 16 * 1 + 0, 16 * 0 + 1], np.int32)              # the 3-step case: bit 1 of set 0 twice
START = np.array([3, 0, 3], np.int32)
IDX = np.array([1, 0, 1], np.int32)


@pytest.fixture(scope="module")
def env(O):
    yield from shape_env(O)


_cache = {}


def general(p, orc, shape, n_steps=4):
    """inputs and model outputs (theta = 4; theta 1 and 2 are its first records): per kind "enc" / "pub" (wo, ks), with the table index IDX"""
    key = (shape, n_steps)
    if key not in _cache:
        rng = np.random.default_rng(7000 + 10 * WFA_SHAPES.index(shape) + n_steps)
        sets = [words(rng, COUNT, d, 2 * p.l, 2, N) for d in (2, 3)]
        fin_a, fin_b = words(rng, 2, STATES, N), words(rng, 2, STATES, N)
        tr, sb = TRANS[4 - n_steps:], STEP_BIT if n_steps == 4 else STEP_BIT3
        ref = {kind: WR.batch(p, orc, sets, tr, sb, fin_a if kind == "enc" else None, fin_b, 4, START, IDX) for kind in ("enc", "pub")}
        _cache[key] = (sets, fin_a, fin_b, tr, sb, ref)
    return _cache[key]


class opened:
    """the TgswSets of a case"""
    def __init__(self, ck, sets):
        self.ck, self.sets = ck, sets

    def __enter__(self):
        self.ts = [self.ck.tgsw_set(C, C.shape[1]) for C in self.sets]
        return self.ts

    def __exit__(self, *exc):
        for t in self.ts:
            t.close()


def same(got, ref, what):
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.array_equal(got, ref), (what, differing(got, ref))


@pytest.mark.parametrize("n_steps", [4, 3])
@pytest.mark.parametrize("shape", WFA_SHAPES, ids=shape_id)
def test_general_automaton_every_word(env, shape, n_steps):
    # two sets of different d, a bit read twice, copy states, fan-in 3, permutation layers, even and odd step counts, public and encrypted finals
    # with a per-sample table, theta 1 / 2 / 4 with n_out = 3 (two outputs share a start state)
    p, K, orc, ck = env(shape)
    sets, fin_a, fin_b, tr, sb, ref = general(p, orc, shape, n_steps)
    with opened(ck, sets) as ts:
        for kind in ("enc", "pub"):
            fa = fin_a if kind == "enc" else None
            for theta in (4, 2, 1):
                u = ck.lhe_wfa_wo_keyswitch(ts, tr, sb, fin_b, START, theta=theta, fin_a=fa, table_index=IDX)
                same(u, ref[kind][0][:, :, :theta], (kind, theta, "wo"))
                got = ck.lhe_wfa(ts, tr, sb, fin_b, START, theta=theta, fin_a=fa, table_index=IDX)
                same(got, ref[kind][1][:, :, :theta], (kind, theta, "ks"))
            assert np.array_equal(ref[kind][0][:, 0], ref[kind][0][:, 2])     # outputs 0 and 2 start in one state


@pytest.mark.parametrize("shape", WFA_SHAPES, ids=shape_id)
def test_chunks_window_and_slices_give_the_same_words(env, shape):
    p, K, orc, ck = env(shape)
    sets, fin_a, fin_b, tr, sb, ref = general(p, orc, shape)
    kw = dict(theta=2, fin_a=fin_a, table_index=IDX)
    want = ref["enc"][1][:, :, :2]
    with opened(ck, sets) as ts:
        try:
            for g in (1, 2, 5, 0):            # 5 states in chunks of 2: a ragged last chunk; 0: automatic
                ck.set_wfa_chunk(g)
                same(ck.lhe_wfa(ts, tr, sb, fin_b, START, **kw), want, ("chunk", g))
        finally:
            ck.set_wfa_chunk(0)
        # a window of the sets: first != 0, the index array follows the window
        win = ck.lhe_wfa(ts, tr, sb, fin_b, START, theta=2, fin_a=fin_a, table_index=IDX[1:], first=1, count=2)
        same(win, want[1:], "window")
        same(ck.lhe_wfa_wo_keyswitch(ts, tr, sb, fin_b, START, theta=2, table_index=IDX[1:2], first=1, count=1), ref["pub"][0][1:2, :, :2], "window pub")
        try:
            ck.set_tree_slice(10)             # two layers of 5 TLWE per sample: slices of one sample, the call crosses three of them
            same(ck.lhe_wfa(ts, tr, sb, fin_b, START, **kw), want, "slices by layers")
            ck.set_tree_slice(6)              # ... and by output records: 3 outputs x theta 2 per sample
            same(ck.lhe_wfa(ts, tr, sb, fin_b, START, **kw), want, "slices by records")
        finally:
            ck.set_tree_slice(65536)


@pytest.mark.parametrize("shape", WFA_SHAPES, ids=shape_id)
def test_one_state_one_step_and_a_step_of_copies(env, shape):
    import lut_reference as R
    p, K, orc, ck = env(shape)
    rng = np.random.default_rng(7100 + WFA_SHAPES.index(shape))
    sets = [words(rng, 2, 1, 2 * p.l, 2, N)]
    fin_a, fin_b = words(rng, 1, STATES, N), words(rng, 1, STATES, N)
    with opened(ck, sets) as ts:
        # n_states = 1, n_steps = 1: the only transition is 0 -> 0 on both bit values
        one = np.zeros((1, 1, 2), np.int32)
        u = ck.lhe_wfa_wo_keyswitch(ts, one, [0], fin_b[:, :1], [0], theta=2, fin_a=fin_a[:, :1])
        want = np.stack([R.extract_at(np.concatenate([fin_a[0, 0], fin_b[0, 0]]), j, N) for j in range(2)])
        same(u, np.broadcast_to(want, (2, 1, 2, N + 1)), "1 x 1")
        # one step whose d0 and d1 are one state for every state: the finals come back unchanged (here permuted), encrypted and public
        perm = np.array([2, 0, 4, 1, 3])
        tr = np.stack([perm, perm], axis=1)[None].astype(np.int32)
        start = np.arange(STATES, dtype=np.int32)
        for fa in (fin_a, None):
            u = ck.lhe_wfa_wo_keyswitch(ts, tr, [0], fin_b, start, theta=4, fin_a=fa)
            za = np.zeros(N, np.int32)
            want = np.stack([np.stack([R.extract_at(np.concatenate([za if fa is None else fa[0, q], fin_b[0, q]]), j, N) for j in range(4)]) for q in perm])
            same(u, np.broadcast_to(want, (2, STATES, 4, N + 1)), ("copies", fa is None))
            ref = WR.batch(p, orc, sets, tr, [0], fa, fin_b, 4, start)[0]
            same(u, ref, ("copies, model", fa is None))


def test_the_checks_that_look_at_the_sets(env):
    import thfhe
    shape = WFA_SHAPES[0]
    p, K, orc, ck = env(shape)
    sets, fin_a, fin_b, tr, sb, ref = general(p, orc, shape)
    other = env(WFA_SHAPES[1])[3]
    with opened(ck, sets) as ts, opened(ck, [sets[0][:2]]) as short:
        call = lambda t=ts, step_bit=sb, **kw: ck.lhe_wfa(t, tr, step_bit, fin_b, START, **kw)
        for bad in (16 * 2 + 0, 16 * 0 + 2, 16 * 1 + 3, -1):         # set 2 of 2; bit 2 of a 2-bit set; bit 3 of a 3-bit set
            with pytest.raises(thfhe.ThfheError, match="step_bit"):
                call(step_bit=np.array([bad, 1, 18, 0], np.int32))
        with pytest.raises(thfhe.ThfheError, match="one count and one context"):
            call(t=[short[0], ts[1]], count=2)
        with pytest.raises(thfhe.ThfheError, match="not all in the set"):
            call(first=2, count=2)
        with pytest.raises(thfhe.ThfheError, match="another context"):
            other.lhe_wfa(ts, tr, sb, fin_b, START)
        assert call(first=3, count=0).shape == (0, 3, 1, p.n + 1)
