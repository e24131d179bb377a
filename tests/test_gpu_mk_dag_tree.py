"""Encrypted-table, tree and multi-value tree nodes in the 3-gen gate-DAG executor on the MI355X (pytest -m gpu): the
circuit gate -> LUT -> TREE (p = 4 x 4, theta_lo = 2) -> TREE_MV (k = 2) -> LUT_ENC -> NAND on two input wires, two instances, on MK2 (n = 30) and
MK4-N2048 (n = 10, two parties): every wire of thfhe_mk_dag_run_tree_batch equal to evaluate_levels (the flat multi-key calls level by level) and to
the model composed from the CPU oracle's pieces; the same with one node per launch and one sample per tree slice; the plan's figures; and the
context check -- a D = P n packing key with a TREE row is refused, a plan without trees runs with no key.  Tables and the packing key are random
words: only word equality is asserted."""
import numpy as np
import pytest

import mk_lut_reference as R
import mk_pack_reference as MP
import mk_tree_mv_reference as TM
from support import differing

pytestmark = pytest.mark.gpu

T_PK, BASEBIT = 2, 1      # the D = N packing key's digits


def _circuit(p, rng):
    import thfhe
    from thfhe import circuits as CIR
    N = p.N
    tv = rng.integers(-2**63, 2**63, N, dtype=np.int64)
    rows = rng.integers(-2**63, 2**63, (2, N), dtype=np.int64)                 # p_hi = 4, theta_lo = 2: R = 2 rows
    tv0 = rng.integers(-2**63, 2**63, N, dtype=np.int64)
    w = rng.integers(-3, 4, (2, 4, 4)).astype(np.int32)                         # k = 2, p_hi = 4, p_lo = 4
    ea, eb = rng.integers(-2**63, 2**63, (2, N), dtype=np.int64)
    ob = int(rng.integers(-2**63, 2**63, dtype=np.int64))
    par = dict(tv=tv, rows=rows, tv0=tv0, w=w, ea=ea, eb=eb, ob=ob, lo_w=(3,), lo_b=1234567, hi_w=(-5,), hi_b=-7654321)
    cir = CIR.Circuit()
    a, b = cir.inputs(2)
    g = cir.gate(thfhe.NAND, a, b)
    l = cir.lut(cir.table(tv), [g])[0]
    t = cir.tree(cir.tree_rows(rows), [l], [a], 4, lo_weights=par["lo_w"], hi_weights=par["hi_w"], lo_bias=par["lo_b"], hi_bias=par["hi_b"], theta1=2)
    m = cir.tree_mv(cir.mv_base(tv0), w, [t], [b], lo_weights=par["lo_w"], hi_weights=par["hi_w"], lo_bias=par["lo_b"], hi_bias=par["hi_b"], out_bias=ob)
    z = cir.lut_enc(cir.enc_table(ea, eb), [m[0]])[0]
    f = cir.gate(thfhe.NAND, z, m[1])
    assert (g, l, t, m, z, f) == (2, 3, 4, [5, 6], 7, 8)
    return cir, par


def _model(O, orc, pk, par, x):
    """one instance, wire by wire, from the oracle's pieces"""
    v = [x[0], x[1]]
    v.append(orc.gates(O.NAND, x[0:1], x[1:2])[0])
    v.append(R.lut_bootstrap(orc, [v[2]], (1,), 0, par["tv"], 1)[0])
    v.append(MP.tree(orc, pk, T_PK, BASEBIT, par["rows"], [v[3]], [v[0]], 4, par["lo_w"], par["lo_b"], 2, par["hi_w"], par["hi_b"]))
    v.extend(TM.tree_mvk(orc, pk, T_PK, BASEBIT, par["tv0"], par["w"], [v[4]], [v[1]], par["lo_w"], par["lo_b"], par["hi_w"], par["hi_b"], par["ob"]))
    v.append(MP.lut_bootstrap_enc(orc, [v[5]], (1,), 0, par["ea"], par["eb"], 1)[0])
    v.append(orc.gates(O.NAND, v[7][None], v[6][None])[0])
    return np.stack(v)


@pytest.mark.parametrize("name,over", [("MK2", dict(n=30)), ("MK4-N2048", dict(n=10, parties=2))])
def test_chain_equals_the_flat_calls_and_the_model(O, name, over):
    import thfhe
    from thfhe import circuits as CIR
    p = O.make_params(name, **over)
    s = O.SIGMAS[name]
    K = O.MKKeys(p, 67, s["bk"], s["ks"])
    orc = O.MKOracle(p, K.bk, K.ksk)
    ck = thfhe.MKCloudKey(thfhe.make_params(**p.as_dict()), K.bk, K.ksk, device=0)
    try:
        rng = np.random.default_rng(p.N + 7)
        Q = 2
        x = np.stack([R.encrypt_words(K, rng.integers(-2**31, 2**31, 2), s["lwe"], 80 + i) for i in range(Q)])   # [instance][wire][words]
        cir, par = _circuit(p, rng)
        pk = rng.integers(-2**63, 2**63, (p.N, T_PK, (1 << BASEBIT) - 1, 2, p.N), dtype=np.int64)

        # a plan without trees runs with no packing key; with a TREE row the context is asked for the D = N key
        plain = CIR.Circuit()
        pa, pb = plain.inputs(2)
        pz = plain.lut_enc(plain.enc_table(par["ea"], par["eb"]), [plain.gate(thfhe.NAND, pa, pb)])[0]
        no_key = CIR.evaluate_batch(ck, plain, x)
        for i in range(Q):
            nand = orc.gates(O.NAND, x[i, 0:1], x[i, 1:2])[0]
            assert np.array_equal(no_key[i, 2], nand) and np.array_equal(no_key[i, pz], MP.lut_bootstrap_enc(orc, [nand], (1,), 0, par["ea"], par["eb"], 1)[0])
        with pytest.raises(thfhe.ThfheError, match="no packing key"):
            CIR.evaluate_batch(ck, cir, x)
        ck.pack_key_set(rng.integers(-2**63, 2**63, (p.parties * p.n, 2, 3, 2, p.N), dtype=np.int64), 2, 2)
        with pytest.raises(thfhe.ThfheError, match="D = N"):
            CIR.evaluate_batch(ck, cir, x)
        assert np.array_equal(CIR.evaluate_batch(ck, plain, x), no_key)          # ... which a plan without trees does not need
        ck.pack_key_set(pk, T_PK, BASEBIT)

        st = {}
        wires = CIR.evaluate_batch(ck, cir, x, stats=st)
        assert wires.shape == (Q, 9, p.parties * p.n + 1)
        # six levels; launches 1 + 1 + 2 + 2 + 1 + 1; rotations per instance 1 + 1 + (R + 1) + (1 + k) + 1 + 1 = 10
        assert (st["levels"], st["launches"], st["rotations"], st["widest_level"], st["instances"]) == (6, 8, 10 * Q, Q, Q)
        for i in range(Q):
            levels = CIR.evaluate_levels(ck, cir, x[i])
            assert np.array_equal(wires[i], levels), (name, i, differing(wires[i], levels))
            ref = _model(O, orc, pk, par, x[i])
            assert np.array_equal(wires[i], ref), (name, i, differing(wires[i], ref))
        assert np.array_equal(CIR.evaluate(ck, cir, x[1]), wires[1])
        sel = CIR.evaluate_batch(ck, cir, x, out_wires=[8, 4, 6])
        assert np.array_equal(sel, wires[:, [8, 4, 6]])
        try:   # one node per launch and one sample per tree slice (k p_hi = 8 candidates; the TREE's 4 fit twice: tree_slice 4 is one TREE node)
            ck.set_dag_slice(1)
            assert np.array_equal(CIR.evaluate_batch(ck, cir, x), wires), (name, "dag_slice 1")
            ck.set_dag_slice(8192)
            ck.set_tree_slice(8)
            assert np.array_equal(CIR.evaluate_batch(ck, cir, x), wires), (name, "tree_slice 8")
            ck.set_tree_slice(4)
            assert np.array_equal(CIR.evaluate_batch(ck, cir, x), wires), (name, "tree_slice 4")
        finally:
            ck.set_dag_slice(8192)
            ck.set_tree_slice(16384)
        # the older entries refuse the rows, a SELECT row is refused by the new one, and the context stays usable
        with pytest.raises(thfhe.ThfheError, match="opcode not defined"):
            mvs, bases, words = cir.mv_families()
            ck.dag_run_mv_batch(x, cir.nodes(), cir.specs, np.stack(cir.tables), mvs, bases, words, [par["ob"]])
        with pytest.raises(thfhe.ThfheError, match="SELECT"):
            ck.dag_run_tree_batch(x, np.array([[17, 0, -1, -1, 0, 0]], np.int32), trees=cir.tree_specs)
        assert np.array_equal(CIR.evaluate_batch(ck, cir, x), wires)
    finally:
        ck.close()
