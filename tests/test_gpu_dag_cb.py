"""Circuit-bootstrap nodes in the gate-DAG executor on the MI355X (pytest -m gpu): real keys at n = 16 with the level-2
context and the private key at full D = 2048 (tests/dag_cb_cases.py, whose builders have the CPU model decode every case before the device is
asked).  No tolerance anywhere: every wire and every TGSW word of a run equals the model, the level-by-level yardstick of flat calls
(circuits.evaluate_levels) and the flat thfhe_circuit_bootstrap of the same wires, word for word."""
import numpy as np
import pytest

import cb_cases as CC
import dag_cb_cases as DC
from support import differing

pytestmark = pytest.mark.gpu


class Dev:
    """the gate context with the private key, the level-2 context and the packing context of a named set"""
    def __init__(self, O, name):
        import thfhe
        from thfhe import threshold as T
        self.S = S = DC.keys(O, name, device=0)
        self.ck = thfhe.CloudKey(S.tp, S.K.bk, S.K.ksk, device=0)
        self.ck2 = thfhe.MKCloudKey(S.tp2, S.K2.bk, S.K2.ksk, device=0)
        self.ck.cb_key_set(self.ck2, S.pks, CC.T, CC.BASEBIT)
        self.pc = T.PolyContext(0)
        self.pc.set_pack_key(S.pk, S.p.ks_t, S.p.ks_basebit)

    def run(self, c, one_rotation=False, words=True, **kw):
        """(wires int32[instances][n_wires][n+1], stats, the rows of every computed set) of a case's circuit on its inputs"""
        cir = c["cir"]
        fam = dict(cir.lhe_families(), **cir.cb_families())
        r = self.ck.dag_run_cb_batch(c["x"], cir.nodes(), one_rotation=one_rotation, return_words=words, pack=self.pc, **fam, **kw)
        return (np.concatenate([c["x"], r[0]], axis=1),) + tuple(r[1:])

    def close(self):
        self.pc.close()
        self.ck.close()
        self.ck2.close()


@pytest.fixture(scope="module")
def sk128(O):
    d = Dev(O, "SK-128")
    yield d
    d.close()


def same(got, ref, what):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.array_equal(got, ref), (what, differing(got, ref))


def check_lookup(D, c, one_rotation):
    from thfhe import circuits as CI
    S, cir = D.S, c["cir"]
    got, st, words = D.run(c, one_rotation)
    same(got, c["ref"], "every wire equals the model")
    same(words[0], c["rows"][0], "every TGSW word equals the model")
    d = len(cir.cb_specs[0])
    assert st["levels"] == 4 and st["level2_rotations"] == got.shape[0] * d * (1 if one_rotation else S.tp.l)
    # ... and the yardstick of flat calls in a row, instance by instance; evaluate_batch is the same run through the circuit front end
    for q in range(got.shape[0]):
        same(got[q], CI.evaluate_levels(D.ck, cir, c["x"][q], one_rotation=one_rotation), f"evaluate_levels, instance {q}")
    same(CI.evaluate_batch(D.ck, cir, c["x"], one_rotation=one_rotation), got, "evaluate_batch")
    assert np.array_equal(S.K.decrypt(got[:, c["out"]]), c["want"].astype(bool))
    assert np.array_equal(S.K.decrypt(got[:, c["nand"]]), ~(c["want"].astype(bool) & c["k"].astype(bool)))


@pytest.mark.parametrize("one_rotation", [False, True], ids=["per level", "one rotation"])
def test_lookup_at_a_computed_address(O, sk128, one_rotation):
    check_lookup(sk128, DC.lookup(O, one_rotation=one_rotation, device=0), one_rotation)


def test_sk80_at_the_smallest_shape(O):
    D = Dev(O, "SK-80")
    try:
        check_lookup(D, DC.lookup(O, "SK-80", d=1, d_tree=0, count=2, device=0), False)
    finally:
        D.close()


def test_array_read_at_a_computed_index(O, sk128):
    from thfhe import circuits as CI
    c = DC.array_read(O, device=0)
    S, cir = sk128.S, c["cir"]
    got, st, words = sk128.run(c)
    same(got, c["ref"], "every wire equals the model")
    same(words[0], c["rows"][0], "every TGSW word equals the model")
    own = cir.n_inputs + next(iter(cir.cb_rows))
    same(got[:, own], c["x"][:, c["index"][0]], "the CB node's own wire is a copy of bit 0's, here an input")
    assert np.array_equal(S.K.decrypt(got[:, c["out"]]), c["want"])
    # the same GATHER on a client set made of the returned words: the circuit without the CB node, the set given by the caller
    twin = CI.Circuit()
    x = twin.inputs(8)
    twin.gates = [g for g in cir.gates[:cir.n_wires() - 8 - 2]]          # everything before the CB node and the GATHER
    out = CI.lhe_array_read(twin, c["g"], 0, 1, 2)
    with sk128.ck.tgsw_set(words[0], 3) as ts:
        ref = CI.evaluate_batch(sk128.ck, twin, c["x"], out_wires=[out], pack=sk128.pc, tgsw_sets=[ts])
    same(got[:, c["out"]], ref[:, 0], "the GATHER on a client set of the same words")


def test_mux_max_on_one_computed_set(O, sk128):
    c = DC.mux_max(O, device=0)
    S = sk128.S
    got, st, words = sk128.run(c)
    same(got, c["ref"], "every wire equals the model")
    same(words[0], c["rows"][0], "every TGSW word equals the model")
    count, width = c["A"].shape[0], 3
    val = (S.K.decrypt(got[:, c["out"]]).reshape(count, width) << np.arange(width - 1, -1, -1)).sum(axis=1)
    assert np.array_equal(val, np.maximum(c["A"], c["B"])) and c["A"][0] == c["B"][0]


@pytest.mark.parametrize("dag_slice", [1, 5, 28672])
def test_three_sets_two_of_them_on_one_level(O, sk128, dag_slice):
    # 7 instances in slices of 1, of 5 + 2 (a short last slice: the node-major bases base[node] S change with S) and in one
    c = DC.three_sets(O, device=0)
    S, cir, ck = sk128.S, c["cir"], sk128.ck
    ck.set_dag_slice(dag_slice)
    try:
        got, st, words = sk128.run(c)
    finally:
        ck.set_dag_slice(28672)
    same(got, c["ref"], "every wire equals the model")
    assert st["levels"] == 6 and st["level2_rotations"] == 7 * 7 * S.tp.l
    for k, wires in enumerate(cir.cb_specs):
        same(words[k], c["rows"][k], f"set {k}: every word equals the model")
        tset, flat = ck.circuit_bootstrap(got[:, wires].reshape(-1, got.shape[-1]), len(wires), return_words=True)
        tset.close()
        same(words[k].reshape(flat.shape), flat, f"set {k}: every word equals the flat circuit_bootstrap of the same wires")
    assert np.array_equal(S.K.decrypt(got[:, c["outs"]]).reshape(7, 3), c["plain"][:, c["outs"]])


@pytest.mark.parametrize("one_rotation", [False, True], ids=["per level", "one rotation"])
def test_the_bit_slice_boundary(O, sk128, one_rotation):
    from thfhe import lut
    c = DC.slice_boundary(O, one_rotation, device=0)
    S = sk128.S
    assert c["x"].shape[0] * 3 == CC.SLICE_BITS + 1                      # slices of 682 + 1 instances
    got, st, words = sk128.run(c, one_rotation, out_wires=[c["out"]])
    w = words[0].reshape(c["rows"].shape)
    for b0 in range(0, w.shape[0], 256):
        same(w[b0:b0 + 256], c["rows"][b0:b0 + 256], f"bits {b0} .. {b0 + 255}")
    look = got[:, -1][DC.SLICE_READ]
    same(look, c["ref"], "the lookups of samples 0 and 680 .. 682")
    assert np.array_equal(lut.decode(S.K.phase(look), CC.P_OUT), c["want"])


def test_a_narrower_group_with_the_larger_slice_on_fresh_contexts(O):
    # levels of sum d = 3 and 2 at 1 024 instances: slices of 682 x 3 = 2 046 bits and of 1 024 x 2 = 2 048 bits.  Fresh contexts, so that no
    # earlier call has grown the slice workspace: it is what THIS run reserved.
    c = DC.two_levels(O, device=0)
    D = Dev(O, "SK-128")
    try:
        got, st, words = D.run(c, out_wires=c["wires"])
        assert st["levels"] == 2 and st["launches"] == 3 and st["level2_rotations"] == c["x"].shape[0] * 5 * D.S.tp.l
        same(got[:, -2:], c["nand"], "the NAND wires equal the model")
        for k in (0, 1):
            for q0 in range(0, words[k].shape[0], 128):
                same(words[k][q0:q0 + 128], c["rows"][k][q0:q0 + 128], f"set {k}, instances {q0} .. {q0 + 127}: every word equals the model")
        flat_set, flat = D.ck.circuit_bootstrap(got[:, -2:].reshape(-1, got.shape[-1]), 2, return_words=True)
        flat_set.close()
        same(words[1].reshape(flat.shape), flat, "set 1: every word equals the flat circuit_bootstrap of the same wires")
    finally:
        D.close()


def test_lifetime_of_the_computed_sets_and_the_lent_stream(O, sk128):
    import thfhe
    from thfhe import circuits as CI
    c, a = DC.lookup(O, device=0), DC.array_read(O, device=0)
    ck = sk128.ck
    first = sk128.run(c)
    # a plain leveled run on a client set between two CB runs: the gate context's stream is its own again
    twin = CI.Circuit()
    x = twin.inputs(8)
    twin.gates = [g for g in a["cir"].gates[:a["cir"].n_wires() - 8 - 2]]
    out = CI.lhe_array_read(twin, a["g"], 0, 1, 2)
    rows = a["rows"][0]
    with ck.tgsw_set(rows, 3) as ts:
        mid = CI.evaluate_batch(ck, twin, a["x"], out_wires=[out], pack=sk128.pc, tgsw_sets=[ts])
    same(mid[:, 0], a["ref"][:, a["out"]], "the leveled entry between two CB runs")
    again = sk128.run(c)
    same(again[0], first[0], "the same wires again")
    same(again[2][0], first[2][0], "the same words again")
    ck.dag_cb_release()
    ck.dag_cb_release()                                                  # nothing left to free: not an error
    with pytest.raises(thfhe.ThfheError):                                # a refused run: no level-2 context of the right shape
        ck.dag_run_cb_batch(c["x"], c["cir"].nodes(), level2=_Null(), pack=sk128.pc, **dict(c["cir"].lhe_families(), **c["cir"].cb_families()))
    after = sk128.run(c)
    same(after[0], first[0], "the same wires after the release")
    same(after[2][0], first[2][0], "the same words after the release")
    same(first[0], c["ref"], "... the model's")


class _Null:
    h = None
