"""CPU yardstick of the gate-DAG executor with multi-value nodes (thfhe_dag_run_mv_batch) -- TEST INFRASTRUCTURE ONLY, single
key: dag_tree_reference's walk over a circuit's rows with MV nodes through mv_lut_reference.mv_lut and TREE_MV nodes through
tree_mvk_reference.tree_mvk; every other row as there."""
import numpy as np

import dag_tree_reference as DT
import mv_lut_reference as MV
import tree_mvk_reference as TK

MV_OP, TREE_MV_OP = 19, 20


def evaluate(orc, cir, input_records, pk=None, t=None, basebit=None):
    """int32[n_wires][words] of one instance: the rows in order, runs of rows without multi-value nodes through dag_tree_reference.evaluate."""
    n_in = cir.n_inputs
    words = np.asarray(input_records).shape[-1]
    vals = np.zeros((cir.n_wires(), words), np.int32)
    vals[:n_in] = np.asarray(input_records, np.int32).reshape(n_in, words)
    one = type(cir)()
    for g, (op, a, b, c) in enumerate(cir.gates):
        o = n_in + g
        if op == DT.LUT_OUT:
            continue
        if op in (MV_OP, TREE_MV_OP):
            mi, ti = cir.mv_rows[g]
            lo, hi, p, q, k, base, tabs = cir.mv_specs[mi]
            ops = (a, b, c)
            lo_recs = [vals[x] for x in ops[:lo[0]]]
            if op == MV_OP:
                vals[o:o + q] = MV.mv_lut(orc, lo_recs, lo[1][:lo[0]], lo[2], cir.mv_bases[base], tabs[ti][0])
            else:
                vals[o:o + k] = TK.tree_mvk(orc, pk, t, basebit, lo_recs, lo[1][:lo[0]], lo[2], [vals[x] for x in ops[lo[0]:lo[0] + hi[0]]],
                                            hi[1][:hi[0]], hi[2], cir.mv_bases[base], tabs[ti])[0]
            continue
        # any other row: a one-row circuit over the wires computed so far
        one.__dict__.update(cir.__dict__)
        one.n_inputs, one.gates = o, [(op, a, b, c)]
        one.lut_rows = {0: cir.lut_rows[g]} if g in cir.lut_rows else {}
        one.ext_rows = {0: cir.ext_rows[g]} if g in cir.ext_rows else {}
        theta = cir.specs[(cir.lut_rows.get(g) or cir.ext_rows.get(g))[0]][3] if op in (DT.LUT, DT.LUT_ENC) else 1
        one.gates += [(DT.LUT_OUT, o, -1, -1)] * (theta - 1)
        vals[o:o + theta] = DT.evaluate(orc, one, vals[:o], pk, t, basebit)[o:o + theta]
    return vals
