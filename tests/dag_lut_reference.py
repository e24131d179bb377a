"""CPU yardstick of the gate-DAG executor with LUT nodes (thfhe_dag_run_lut_batch / thfhe_mk_dag_run_lut_batch) -- TEST
INFRASTRUCTURE ONLY: a circuit's rows in order, gates through the oracle (Oracle / MKOracle .gates), LUT nodes through the composed PBS
reference (lut_reference / mk_lut_reference), NOT / COPY on the host."""
import numpy as np

import lut_reference
import mk_lut_reference
import oracle_lib as O

LUT, LUT_OUT = 14, 15


def evaluate(orc, cir, input_records, multi_key=False, only=None):
    """int32[n_wires][words] of one instance.  multi_key: the 3-gen oracle and Torus64 tables.  only: the gate indices to compute (with
    every row they read); None = all."""
    ref = mk_lut_reference if multi_key else lut_reference
    n_in = cir.n_inputs
    words = np.asarray(input_records).shape[-1]
    vals = np.zeros((cir.n_wires(), words), np.int32)
    vals[:n_in] = np.asarray(input_records, np.int32).reshape(n_in, words)
    need = None
    if only is not None:
        need, todo = set(), list(only)
        while todo:
            g = todo.pop()
            if g in need:
                continue
            need.add(g)
            op, a, b, c = cir.gates[g]
            if op == LUT_OUT:
                todo.append(a - n_in)
                continue
            todo += [w - n_in for w in (a, b, c) if w >= n_in]
    for g, (op, a, b, c) in enumerate(cir.gates):
        if need is not None and g not in need:
            continue
        o = n_in + g
        if op == LUT_OUT:
            continue   # written by its head
        if op == LUT:
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
