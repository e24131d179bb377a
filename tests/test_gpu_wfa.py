"""Layered automata under real keys (pytest -m gpu): SK-128 at full size, wfa_less_than(8) and wfa_equal(8) on the 8
operand pairs of wfa_cases.py -- equal operands, operands that differ in the top bit only and in the bottom bit only.  Every output word is
compared with the model (wfa_reference.py), every output must decrypt at modulus 8, before and after the key switch, and the standard deviation
of phase - encode over the 32 ring-key outputs must lie inside [0.5, 2] x sqrt(non-copy steps on the path) sigma_1 (the band of section 4.15, for
the bias reason given there).  tests/test_wfa_host.py runs the same cases on the CPU model: it decrypts all of them at ratio 1.71.  A one-step
automaton equals thfhe_lhe_cmux word for word."""
import numpy as np
import pytest

import lut_reference as R
import wfa_cases
from support import N, differing, words

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ck(O):
    import thfhe
    S = wfa_cases.keys(O)
    c = thfhe.CloudKey(S.tp, S.K.bk, S.K.ksk, device=0)
    yield c
    c.close()


def run(ck, c):
    trans, step_bit, fin, start = c["aut"]
    ts = [ck.tgsw_set(C, C.shape[1]) for C in c["sets"]]
    try:
        return (ck.lhe_wfa_wo_keyswitch(ts, trans, step_bit, c["fin_b"], start, theta=wfa_cases.THETA),
                ck.lhe_wfa(ts, trans, step_bit, c["fin_b"], start, theta=wfa_cases.THETA))
    finally:
        for t in ts:
            t.close()


@pytest.mark.parametrize("which", ["less_than", "equal"])
def test_sk128_comparison_of_8_bit_operands(O, ck, which):
    from thfhe import lut
    S, c = wfa_cases.keys(O), wfa_cases.case(O, which)
    want = c["want"]
    wo, ks = run(ck, c)
    assert np.array_equal(wo, c["wo"]), differing(wo, c["wo"])
    assert np.array_equal(ks, c["ks"]), differing(ks, c["ks"])
    assert np.array_equal(lut.decode(S.K.ring_phase(wo).reshape(want.shape), wfa_cases.P_OUT), want)
    assert np.array_equal(lut.decode(S.K.phase(ks).reshape(want.shape), wfa_cases.P_OUT), want)
    f = want[:, 0, 0].astype(bool)
    assert np.array_equal(f, wfa_cases.A < wfa_cases.B if which == "less_than" else wfa_cases.A == wfa_cases.B)


def test_sk128_noise_inside_the_band(O, ck):
    S = wfa_cases.keys(O)
    cases = [wfa_cases.case(O, w) for w in ("less_than", "equal")]
    wo = np.concatenate([run(ck, c)[0] for c in cases])
    std = wfa_cases.noise(S, wo, np.concatenate([c["want"] for c in cases]))
    pred = wfa_cases.predicted(S, cases)
    print(f"\nwfa noise SK-128: measured std {std:.3e} over {wo.shape[0] * wo.shape[2]} outputs, predicted {pred:.3e}, ratio {std / pred:.2f}")
    assert 0.5 * pred <= std <= 2 * pred


def test_one_step_automaton_equals_lhe_cmux(O, ck):
    S = wfa_cases.keys(O)
    rng = np.random.default_rng(4700)
    count, d = 4, 2
    Cs = words(rng, count, d, 2 * S.p.l, 2, N)
    d1, d0 = words(rng, count, 2 * N), words(rng, count, 2 * N)
    fin = np.stack([d0, d1], axis=1)                                   # table s = (state 0: d0[s], state 1: d1[s])
    trans = np.array([[[0, 1], [1, 0]]], np.int32)                     # V_0[0] = d0 + C (.) (d1 - d0); V_0[1] swaps the operands
    with ck.tgsw_set(Cs, d) as ts:
        a, b = ck.lhe_cmux(ts, 1, d1[:, :N], d1[:, N:], d0[:, :N], d0[:, N:])
        a2, b2 = ck.lhe_cmux(ts, 1, d0[:, :N], d0[:, N:], d1[:, :N], d1[:, N:])
        u = ck.lhe_wfa_wo_keyswitch([ts], trans, [1], fin[:, :, N:], [0, 1], theta=4, fin_a=fin[:, :, :N], table_index=np.arange(count))
    for s in range(count):
        for o, (ma, mb) in enumerate(((a, b), (a2, b2))):
            want = np.stack([R.extract_at(np.concatenate([ma[s], mb[s]]), j, N) for j in range(4)])
            assert np.array_equal(u[s, o], want), (s, o)
