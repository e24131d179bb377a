"""Leveled nodes in the gate-DAG executor on the named parameter sets (pytest -m gpu): real keys, real TGSW samples.  The cases
and the model's wires come from tests/dag_lhe_cases.py, which the model-only noise test of tests/test_dag_lhe_host.py shares: every wire of the
device run equals the model word for word, every output decrypts, and the gathered wires carry sqrt(2) sigma_ks within [0.5, 1.5] x."""
import numpy as np
import pytest

import dag_lhe_cases as DC
from support import differing

pytestmark = pytest.mark.gpu


class Device:
    """the CloudKey, packing context and TgswSets of a case"""
    def __init__(self, S, sets):
        import thfhe
        from thfhe import threshold as T
        self.ck = thfhe.CloudKey(S.tp, S.K.bk, S.K.ksk, device=0)
        self.pc = T.PolyContext(0)
        self.pc.set_pack_key(S.pk, S.p.ks_t, S.p.ks_basebit)
        self.ts = [self.ck.tgsw_set(C, C.shape[1]) for C in sets]

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for t in self.ts:
            t.close()
        self.pc.close()
        self.ck.close()


def same(got, ref, what):
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.array_equal(got, ref), (what, differing(got, ref))


def test_sk128_array_read_and_mux_max(O):
    from thfhe import circuits as CI
    c, m = DC.array_read(O), DC.mux_max(O)
    S, q = c["S"], np.arange(8)
    with Device(S, c["sets"]) as D:
        # lhe_array_read over 8 computed bits at all 8 addresses as 8 instances (and over 16 at the odd addresses)
        got = CI.evaluate_batch(D.ck, c["cir"], c["x"], pack=D.pc, tgsw_sets=D.ts)
        same(got, c["ref"], "array read")
        for name, wire, addr in (("(1, 2)", c["read8"], c["a8"]), ("(1, 3)", c["read16"], c["a16"])):
            want = c["want"][q, addr]
            assert np.array_equal(S.K.decrypt(got[:, wire]), want), name
            std = DC.noise_std(S, got[:, wire], want)
            print(f"\ngathered wires, SK-128 {name}: measured std {std:.3e} over 8 outputs (GPU == CPU model word for word), sqrt(2) sigma_ks = "
                  f"{DC.SIGMA_GATHER:.1e}, ratio {std / DC.SIGMA_GATHER:.2f}")
            assert 0.5 * DC.SIGMA_GATHER <= std <= 1.5 * DC.SIGMA_GATHER, (name, std)
        # wfa_mux_max at width 8 on 8 pairs, on the same key with its own sets
        ts = [D.ck.tgsw_set(C, C.shape[1]) for C in m["sets"]]
        try:
            got = CI.evaluate_batch(D.ck, m["cir"], m["x"], tgsw_sets=ts)       # no GATHER: no packing context
        finally:
            for t in ts:
                t.close()
        same(got, m["ref"], "mux max")
        val = (S.K.decrypt(got[:, m["out"]]).reshape(8, 8) << np.arange(7, -1, -1)).sum(axis=1)
        assert np.array_equal(val, np.maximum(m["A"], m["B"])), (val, m["A"], m["B"])


@pytest.mark.parametrize("name", ["SK-80", "SK-lib"])
def test_other_named_sets_at_the_smallest_shape(O, name):
    from thfhe import circuits as CI
    c = DC.smallest(O, name)
    with Device(c["S"], c["sets"]) as D:
        got = CI.evaluate_batch(D.ck, c["cir"], c["x"], pack=D.pc, tgsw_sets=D.ts)
    same(got, c["ref"], name)
    assert np.array_equal(c["S"].K.decrypt(got[:, c["out"]]), c["want"])
