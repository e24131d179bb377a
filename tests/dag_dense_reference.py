"""CPU yardstick of the gate-DAG executor with DENSE nodes (thfhe_dag_run_dense_batch / thfhe_mk_dag_run_dense_batch) -- TEST
INFRASTRUCTURE ONLY: a circuit's rows in order for ONE instance, wire by wire.  A DENSE node is linear_reference.linear on the records of its
operand wires, then lut_reference / mk_lut_reference .lut_bootstrap (weight 1, bias 0, key switch) of every sum on its output's table; gates go
through the oracle, LUT nodes through the same composed PBS reference, NOT / COPY on the host.  No library call."""
import numpy as np

import linear_reference as LR
import lut_reference
import mk_lut_reference
import oracle_lib as O

LUT, LUT_OUT, DENSE = 14, 15, 25


def dense_node(orc, ref, cir, g, vals, pmap=map):
    """the M theta records of the DENSE node at gate index g, int32[M theta][words]"""
    W, bias, tids, theta = cir.dense_specs[cir.dense_rows[g][0]]
    off = cir.gates[g][1]
    x = vals[cir.dense_wires[off:off + W.shape[1]]][None]
    tv = [np.asarray(t) for t in cir.tables]
    out = LR.fused(ref.lut_bootstrap, orc, W, x, bias, tv, theta, tids, True, pmap)
    return out.reshape(W.shape[0] * theta, -1)


def evaluate(orc, cir, input_records, multi_key=False, pmap=map):
    """int32[n_wires][words] of one instance.  multi_key: the 3-gen oracle and Torus64 tables.  Circuits of gates, LUT and DENSE rows."""
    ref = mk_lut_reference if multi_key else lut_reference
    n_in = cir.n_inputs
    words = np.asarray(input_records).shape[-1]
    vals = np.zeros((cir.n_wires(), words), np.int32)
    vals[:n_in] = np.asarray(input_records, np.int32).reshape(n_in, words)
    for g, (op, a, b, c) in enumerate(cir.gates):
        o = n_in + g
        if op == LUT_OUT:
            continue   # written by its head
        if op == DENSE:
            r = dense_node(orc, ref, cir, g, vals, pmap)
            vals[o:o + r.shape[0]] = r
        elif op == LUT:
            si, ti = cir.lut_rows[g]
            nin, w, bias, theta = cir.specs[si]
            recs = [vals[x] for x in (a, b, c)[:nin]]
            vals[o:o + theta] = ref.lut_bootstrap(orc, recs, w[:nin], bias, np.asarray(cir.tables[ti]), theta)
        elif op == O.NOT:
            vals[o] = (0 - vals[a].astype(np.int64)).astype(np.int32)
        elif op == O.COPY:
            vals[o] = vals[a]
        else:
            vals[o] = orc.gates(op, vals[a][None], vals[b][None], vals[c][None] if op in (O.MUX, O.AND3) else None)[0]
    return vals
