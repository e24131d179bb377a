"""Multi-value nodes in the 3-gen gate-DAG executor on the MI355X (pytest -m gpu): a circuit of two input wires -- an MV
node with p = 4 and q = 3, a NAND of two of its outputs, a LUT node reading the third --, two instances, on MK2 (n = 30) and on MK4-N2048 (n = 10,
two parties): every wire equal to the flat calls in a row and to the model composed from the CPU oracle's pieces, the same with one node per launch
and one node per multi-value slice, the plan's figures, and the dispatch of thfhe.circuits."""
import numpy as np
import pytest

import mk_lut_reference as R
import mk_mv_lut_reference as MV

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name,over", [("MK2", dict(n=30)), ("MK4-N2048", dict(n=10, parties=2))])
def test_mv_lut_and_gate_rows_equal_the_flat_calls_and_the_model(O, name, over):
    import thfhe
    from thfhe import circuits as CIR
    p = O.make_params(name, **over)
    s = O.SIGMAS[name]
    K = O.MKKeys(p, 61, s["bk"], s["ks"])
    orc = O.MKOracle(p, K.bk, K.ksk)
    ck = thfhe.MKCloudKey(thfhe.make_params(**p.as_dict()), K.bk, K.ksk, device=0)
    try:
        rng = np.random.default_rng(5)
        Q, q, taps = 2, 3, 4
        x = np.stack([R.encrypt_words(K, rng.integers(-2**31, 2**31, 2), s["lwe"], 40 + i) for i in range(Q)])   # [instance][wire][words]
        tv0 = rng.integers(-2**63, 2**63, p.N, dtype=np.int64)
        fac = rng.integers(-2**31, 2**31, (q, taps)).astype(np.int32)
        tv = rng.integers(-2**63, 2**63, p.N, dtype=np.int64)
        out_bias, weights, bias = int(rng.integers(-2**63, 2**63, dtype=np.int64)), (3, -2), 12345

        cir = CIR.Circuit()
        a, b = cir.inputs(2)
        m = cir.mv(cir.mv_base(tv0), fac, [a, b], weights=weights, bias=bias, out_bias=out_bias)
        g = cir.gate(thfhe.NAND, m[0], m[1])
        l = cir.lut(cir.table(tv), [m[2]])[0]
        assert (m, g, l) == ([2, 3, 4], 5, 6)

        # the flat calls in a row ...
        f_mv = ck.mv_lut_bootstrap(fac, x[:, 0], x[:, 1], tv0=tv0, weights=weights, bias=bias, out_bias=out_bias)
        f_nand = ck.gates(thfhe.NAND, f_mv[:, 0], f_mv[:, 1])
        f_lut = ck.lut_bootstrap(tv, f_mv[:, 2])[:, 0]
        flat = np.concatenate([x, f_mv, f_nand[:, None], f_lut[:, None]], axis=1)
        # ... and the model
        for i in range(Q):
            r_mv = MV.mv_lut(orc, [x[i, 0], x[i, 1]], weights, bias, tv0, fac, out_bias)
            assert np.array_equal(flat[i, 2:5], r_mv), (name, i)
            assert np.array_equal(flat[i, 5], orc.gates(O.NAND, r_mv[0:1], r_mv[1:2])[0]), (name, i)
            assert np.array_equal(flat[i, 6], R.lut_bootstrap(orc, [r_mv[2]], (1,), 0, tv, 1)[0]), (name, i)

        st = {}
        wires = CIR.evaluate_batch(ck, cir, x, stats=st)
        assert np.array_equal(wires, flat), name
        # MV level, then the gate and the LUT: three launch groups, one rotation per node and instance
        assert (st["levels"], st["launches"], st["rotations"], st["widest_level"], st["instances"]) == (2, 3, 3 * Q, Q, Q)
        assert np.array_equal(CIR.evaluate(ck, cir, x[1]), flat[1])
        sel = CIR.evaluate_batch(ck, cir, x, out_wires=[6, 3])
        assert np.array_equal(sel, flat[:, [6, 3]])
        try:   # one node per launch, one node per multi-value slice
            ck.set_dag_slice(1)
            ck.set_mv_slice(q)
            assert np.array_equal(CIR.evaluate_batch(ck, cir, x), flat), name
            ck.set_dag_slice(8192)
            assert np.array_equal(CIR.evaluate_batch(ck, cir, x), flat), name
        finally:
            ck.set_dag_slice(8192)
            ck.set_mv_slice(4096)
        # the raw entry without LUT families, and the opcode refused by the entries that have no multi-value generation
        mvs, bases, words = cir.mv_families()
        rows = cir.nodes()[:4]
        out, st2 = ck.dag_run_mv_batch(x, rows, mvs=mvs, mv_tv0=bases, mv_factors=words, mv_out_bias=[out_bias])
        assert np.array_equal(out, flat[:, 2:6]) and st2["launches"] == 2
        with pytest.raises(thfhe.ThfheError):
            ck.dag_run_lut_batch(x, cir.nodes(), cir.specs, np.stack(cir.tables))
        with pytest.raises(thfhe.ThfheError):
            ck.dag_run_batch(x, rows[:, :4])
        assert np.array_equal(ck.gates(thfhe.NAND, f_mv[:, 0], f_mv[:, 1]), f_nand)   # the context stays usable
    finally:
        ck.close()
