"""Reference of circuit bootstrapping in one-rotation mode (include/thfhe_hip.h: thfhe_circuit_bootstrap_mode, thfhe_cb_stage_a with
THFHE_CB_ONE_ROTATION) -- TEST INFRASTRUCTURE ONLY.  Stage A is the many-LUT bootstrap of mk_lut_reference.py (the CPU
oracle's pieces) on the record itself with the l constants mu_j interleaved in ONE Torus64 test vector, coefficients 0 .. l-1 extracted and the
body offsets added; stage B is cb_reference.private_keyswitch.  Nothing here imports the product's kernels.

`models(O, name)` holds, once per process, what the tests of the real-key cases (cb_cases.case) share: the stage-A records of both modes, the
one-rotation rows of the whole pool, and the lookup and comparison of the case on those rows."""
import numpy as np

import cb_cases as CC
import cb_reference as CB
import lhe_reference as LR
import mk_lut_reference as ML
import wfa_reference as WR
from support import N, pmap


def theta(l):
    """the smallest power of two >= l; the engines' theta stops at 4"""
    assert 1 <= l <= 4
    return 1 if l == 1 else (2 if l == 2 else 4)


def test_vector(l, Bgbit, D):
    """int64[D]: mu_j = 2^(63 - (j+1) Bgbit) at every coefficient q = j mod theta for j < l, zero in the unused slots"""
    th = theta(l)
    slot = np.array([1 << (63 - (j + 1) * Bgbit) if j < l else 0 for j in range(th)], np.int64)
    return slot[np.arange(D) % th]


test_vector.__test__ = False   # a helper, not a test, wherever it is imported


def stage_a_one(orc2, recs, l, Bgbit):
    """lwe2 int32[len(recs)][l][D+1] from gate-encoded records: ONE rotation per record (weight 1, bias 0, the mod-switch rounded to multiples of
    theta), record j the extraction at coefficient j, + 2^(31 - (j+1) Bgbit) on the body"""
    recs = np.asarray(recs, np.int32)
    th, tv = theta(l), test_vector(l, Bgbit, orc2.params.N)
    off = np.array([1 << (31 - (j + 1) * Bgbit) for j in range(l)], np.int64)

    def one(r):
        u = ML.lut_wo_keyswitch(orc2, recs[r], tv, th)[:l].astype(np.int64)
        u[:, -1] += off
        return u.astype(np.uint32).view(np.int32)
    return np.stack(pmap(one, range(recs.shape[0])))


def circuit_bootstrap_one(orc2, key, recs, l, Bgbit, t, basebit):
    """rows int32[len(recs)][2l][2][N]: private_keyswitch o stage_a_one"""
    return CB.private_keyswitch(key, stage_a_one(orc2, recs, l, Bgbit), l, t, basebit)


def lwe2_errors(z2, lwe2, bits, l, Bgbit):
    """phase - m g_j of every stage-A record under the level-2 ring key, int64[len(bits)][l], g_j = 2^(32 - (j+1) Bgbit)"""
    lwe2 = np.asarray(lwe2, np.int32).astype(np.int64)
    ph = lwe2[:, :, -1] - (lwe2[:, :, :-1] * np.asarray(z2, np.int64)[None, None, :]).sum(axis=2)
    g = np.array([1 << (32 - (j + 1) * Bgbit) for j in range(l)], np.int64)
    return CB.centred(ph - np.asarray(bits, np.int64).reshape(-1, 1) * g[None, :])


_made = {}


def models(O, name, device=None):
    """dict for the case cb_cases.case(O, name): lwe2_one / lwe2 (stage A in one-rotation / per-level mode, every record of the pool), rows (the
    one-rotation TGSW rows of the pool), lookup (the case's (1, 2) lookup on them) and, on SK-128, wfa (the comparison).  The lookup and the
    comparison have decoded by the time this returns."""
    if name in _made:
        return _made[name]
    from thfhe import lut
    S, c = CC.keys(O, name, device), CC.case(O, name, device)
    l, Bgbit = S.tp.l, S.tp.Bgbit
    lwe2_one = stage_a_one(S.orc2, c["recs"], l, Bgbit)
    rows = CB.private_keyswitch(S.pks, lwe2_one, l, CC.T, CC.BASEBIT)
    m = dict(lwe2_one=lwe2_one, lwe2=CB.stage_a(S.orc2, c["recs"], l, Bgbit), rows=rows)
    Cs = rows[:24].reshape(8, 3, 2 * l, 2, N)
    m["lookup"] = np.stack(pmap(lambda s: LR.lookup(S.orc, Cs[s], None, c["tab"], 1, 2, 1), range(8)))
    assert np.array_equal(lut.decode(S.K.phase(m["lookup"]).reshape(8), CC.P_OUT), c["table"][CC.ADDR]), "the model itself must decode every lookup"
    if name == "SK-128":
        trans, step_bit, fin_b, start = c["aut"]
        Cw = rows[24:].reshape(4, 6, 2 * l, 2, N)
        m["wfa"] = np.stack(pmap(lambda s: WR.wfa(S.orc, [Cw[s]], trans, step_bit, None, fin_b, 1, start), range(4)))
        assert np.array_equal(lut.decode(S.K.phase(m["wfa"]).reshape(4), CC.P_OUT), c["equal"]), "the model itself must decode every comparison"
    # one slice boundary read back with a 2-entry table at d_tree = 0, d_rot = 1
    m["table2"] = np.array([5, 2])
    m["tab2"] = lut.lhe_table(m["table2"], 0, 1, 1, encode=lambda v: lut.encode(v, CC.P_OUT))
    _made[name] = m
    return m
