"""sk_lhe_wfa_step_kernel<L, PUB> on the MI355X at the exactness bound of DESIGN.md section 3, and at its structural limits (pytest -m gpu).

The step kernel calls the lhe_cmux_step of sk_lhe_cmux_kernel from other surroundings: at l <= 3 the spectra stay in registers across all the
states of a chunk, at l = 4 every state requests them again, and the lane index and roots are rebuilt per state behind an empty asm -- eight
separate compilations of the CMux.  test_gpu_wfa_shapes.py and test_gpu_wfa.py drive them with random words and real keys, 5 - 8 bits below
the bound, never at (l, Bgbit) = (3, 10), never above 5 states.  Here (bound_inputs.wfa_case) every non-copy state of the crafted step is the
CMux of lhe_cmux_case: every TGSW word extreme_key_word, d1 - d0 = digit_word in mask and body, so all 2l rows carry the extreme digit and the
limb sum at coefficient N - 1 is 2l N 2^(Bgbit-1) 2^15 exactly; with public finals (bodies alone) the l-row sum.  "random d0": the same
difference out of random operands (w + T, w), a w of its own for every pair of states.  12 identical samples, every one compared; each case
asserts the sum it reached; every output word against the model built from the CPU oracle's exact pieces (wfa_reference.py).  The inputs are
not valid ciphertexts; the contract is word equality.

The records (theta = 4, start = every state) carry every coefficient of a state's mask column -- the peak at N - 1 is observed there -- and
coefficients 0 .. 3 of its body; tests/test_bound_inputs.py::test_automaton_records_see_one_lsb checks that on the CPU.

The instantiation that runs is not reported by the library; it follows from the call: l from the context, PUB = true exactly for the step that
reads public finals (fin_a None), false for every step that reads a layer."""
import numpy as np
import pytest

import bound_inputs as B
import wfa_reference as WR
from support import differing, words
from test_bound_inputs import LHE_SHAPES, WFA_KINDS
from test_gpu_exactness_bound import LHE_IDS, _Lhe

pytestmark = pytest.mark.gpu

BATCH, THETA = 12, 4
START = np.arange(B.WFA_STATES, dtype=np.int32)


def _same_as(got, ref, what):
    """every sample of got (leading axis) equals the one model record set"""
    assert got.shape[1:] == ref.shape, (what, got.shape, ref.shape)
    for g in range(got.shape[0]):
        assert np.array_equal(got[g], ref), (what, g, np.argwhere(got[g] != ref)[:8].tolist())


def _reached(p, C, trans, fa, fb):
    """the limb sum of every non-copy state of a step that reads the finals (fa None: zero masks)"""
    from test_bound_inputs import _wfa_diff
    return {B.lhe_reached(p, C, _wfa_diff(fa, fb, t0, t1)) for t0, t1 in trans.tolist() if t0 != t1}


def _run_bound_case(O, l, Bgbit, name, chunks):
    E = _Lhe(O, l, Bgbit)
    try:
        p, N = E.p, E.p.N
        Cs = B.wfa_bound_bits(p)
        trans, step_bit = B.wfa_bound_automata(p)[name]
        crafted = trans[-1] if name != "reads-a-layer" else trans[0]      # the step whose CMuxes are at the bound
        assert sum(t0 != t1 for t0, t1 in crafted.tolist()) == 4
        with E.ck.tgsw_set(np.tile(Cs, (BATCH, 1, 1, 1, 1)), 2) as ts:
            for kind, variant in WFA_KINDS:
                fa, fb = B.wfa_bound_finals(p, kind, variant, 0xA0 + l)
                # in "reads-a-layer" the step below copies the finals, so the crafted step sees the same operands in the layer buffer
                assert _reached(p, Cs[0], crafted, fa, fb) == {B.bound(2 * l if kind == "enc" else l, N, Bgbit)}
                ref = WR.wfa_wo_keyswitch(p, [Cs], trans, step_bit, fa, fb, THETA, START)
                try:
                    for g in chunks:
                        E.ck.set_wfa_chunk(g)
                        u = E.ck.lhe_wfa_wo_keyswitch([ts], trans, step_bit, fb, START, theta=THETA, fin_a=fa)
                        assert u.shape == (BATCH, B.WFA_STATES, THETA, N + 1)
                        _same_as(u, ref, (name, kind, variant, "chunk", g))
                finally:
                    E.ck.set_wfa_chunk(0)
    finally:
        E.close()


@pytest.mark.parametrize("l, Bgbit", LHE_SHAPES, ids=LHE_IDS)
def test_wfa_step_at_the_bound(O, l, Bgbit):
    # (a) one step, 5 states, 4 of them at the bound.  Chunk 1: one state per workgroup.  Chunk 5: one workgroup walks all the states, so states
    # 1 .. 3 run their CMux at the bound on held spectra (l <= 3) or re-requested ones (l = 4), after a state that left its operands in LDS.
    # Chunk 2: a ragged last chunk.  PUB = true for the public finals, false for the encrypted ones.
    _run_bound_case(O, l, Bgbit, "one-step", (1, 5, 2))


@pytest.mark.parametrize("l, Bgbit", LHE_SHAPES, ids=LHE_IDS)
def test_wfa_bound_step_reads_a_layer(O, l, Bgbit):
    # (b) two steps, the lower one all copies of the finals: the crafted step is the non-final layer, reads the layer buffer (other strides, the
    # masks next to the bodies) and is the PUB = false instantiation whatever the finals are -- with public finals on a zero mask, the l-row sum.
    # Chunk 0 is one state per workgroup on 12 samples; chunk 5 walks the layer in one workgroup.
    _run_bound_case(O, l, Bgbit, "reads-a-layer", (0, 5))


@pytest.mark.parametrize("l, Bgbit", LHE_SHAPES, ids=LHE_IDS)
def test_wfa_bound_step_then_a_random_step(O, l, Bgbit):
    # (c) the crafted step on the finals, then a step on a second bit with random TGSW words whose every CMux has a state the crafted step wrote
    # as d0: the low bits of what the crafted step stored reach the outputs
    _run_bound_case(O, l, Bgbit, "then-random", (0, 5))


# ---- (d) the structural limits, random words, one shape ----------------------------------------------------------------------------------------
MAX_STATES = MAX_OUT = MAX_SETS = 64       # kWfaMaxStates, kWfaMaxOut, kWfaMaxSets of thfhe_lhe.h


def _max_automaton(rng):
    """3 steps over 64 states: random transitions, states 5 and 40 the target of nine more states each (fan-in), every eighth state a copy, and
    all 64 states started from in a random order"""
    trans = rng.integers(0, MAX_STATES, (3, MAX_STATES, 2)).astype(np.int32)
    trans[:, 1:10, 0] = 5
    trans[:, 20:29, 1] = 40
    trans[:, ::8, 1] = trans[:, ::8, 0]
    return trans, rng.permutation(MAX_STATES).astype(np.int32)


def test_wfa_at_its_structural_limits(O):
    # n_states = 64, n_out = 64, theta = 1, 3 steps (so both layer buffers are read and written), 2 samples with a table each, at chunk 0
    # (automatic: one state per workgroup here), 64 (one workgroup walks the whole layer) and 7 (ten chunks, the last of one state); then the same
    # words as 64 sets of d = 1, the three bits in sets 63, 0 and 31 and random words in the others: the same records.  The model: 3 x 64 x 2 exact
    # CMuxes less the copies.
    l, Bgbit = 3, 7
    E = _Lhe(O, l, Bgbit)
    try:
        p, N = E.p, E.p.N
        rng = np.random.default_rng(0x64F)
        trans, start = _max_automaton(rng)
        assert (trans[:, :, 0] == trans[:, :, 1]).sum() >= 24 and (trans[:, :, 0] != trans[:, :, 1]).sum() >= 150
        W = words(rng, 2, 3, 2 * l, 2, N)                      # [sample][bit]
        fin_a, fin_b = words(rng, 2, MAX_STATES, N), words(rng, 2, MAX_STATES, N)
        idx = np.array([1, 0], np.int32)
        step_bit = np.array([2, 0, 1], np.int32)
        wo, ks = WR.batch(p, E.orc, [W], trans, step_bit, fin_a, fin_b, 1, start, idx)
        assert wo.shape == (2, MAX_OUT, 1, N + 1)
        kw = dict(theta=1, fin_a=fin_a, table_index=idx)
        with E.ck.tgsw_set(W, 3) as ts:
            try:
                for g in (0, 64, 7):
                    E.ck.set_wfa_chunk(g)
                    u = E.ck.lhe_wfa_wo_keyswitch([ts], trans, step_bit, fin_b, start, **kw)
                    assert np.array_equal(u, wo), ("chunk", g, differing(u, wo))
            finally:
                E.ck.set_wfa_chunk(0)
            got = E.ck.lhe_wfa([ts], trans, step_bit, fin_b, start, **kw)
            assert np.array_equal(got, ks), differing(got, ks)
        place = {63: 2, 0: 0, 31: 1}                           # set -> the bit of W it holds
        many = [W[:, place[i]][:, None] if i in place else words(rng, 2, 1, 2 * l, 2, N) for i in range(MAX_SETS)]
        step_sets = np.array([16 * 63, 16 * 0, 16 * 31], np.int32)
        opened = []
        try:
            for C in many:
                opened.append(E.ck.tgsw_set(C, 1))
            u = E.ck.lhe_wfa_wo_keyswitch(opened, trans, step_sets, fin_b, start, **kw)
            assert np.array_equal(u, wo), ("64 sets", differing(u, wo))
        finally:
            for t in opened:
                t.close()
    finally:
        E.close()
