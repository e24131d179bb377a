"""CPU yardstick of the gate-DAG executor with encrypted-table, select and tree nodes (thfhe_dag_run_tree_batch) -- TEST
INFRASTRUCTURE ONLY, single key: a circuit's rows in order, gates through the oracle, LUT nodes through lut_reference, LUT_ENC nodes through
tree_lut_reference.lut_enc, SELECT nodes through its pack_boxes + lut_enc, TREE nodes through its tree; NOT / COPY on the host."""
import numpy as np

import lut_reference as R
import oracle_lib as O
import tree_lut_reference as TR

LUT, LUT_OUT, LUT_ENC, SELECT, TREE = 14, 15, 16, 17, 18


def reads(cir, g):
    """The wires row g reads: its operands, a LUT_OUT row's head, a SELECT's candidates."""
    op, a, b, c = cir.gates[g]
    if op == LUT_OUT:
        return [a]
    r = [w for w in (a, b, c) if w >= 0]
    if op == SELECT:
        ti, first = cir.ext_rows[g]
        r += list(range(first, first + cir.tree_specs[ti][2]))
    return r


def evaluate(orc, cir, input_records, pk=None, t=None, basebit=None, only=None):
    """int32[n_wires][words] of one instance.  pk, t, basebit: the packing key (SELECT / TREE nodes).  only: the gate indices to compute (with
    every row they read); None = all."""
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
            todo += [w - n_in for w in reads(cir, g) if w >= n_in]
    for g, (op, a, b, c) in enumerate(cir.gates):
        if (need is not None and g not in need) or op == LUT_OUT:
            continue
        o = n_in + g
        if op in (LUT, LUT_ENC):
            si, ti = cir.lut_rows[g] if op == LUT else cir.ext_rows[g]
            nin, w, bias, theta = cir.specs[si]
            recs = [vals[x] for x in (a, b, c)[:nin]]
            if op == LUT:
                vals[o:o + theta] = R.lut_bootstrap(orc, recs, w[:nin], bias, np.asarray(cir.tables[ti]), theta)
            else:
                vals[o:o + theta] = TR.lut_enc(orc, recs, w[:nin], bias, cir.enc_tables[ti][0], cir.enc_tables[ti][1], theta)
        elif op == SELECT:
            ti, first = cir.ext_rows[g]
            _, hi, p = cir.tree_specs[ti]
            ta, tb = TR.pack_boxes(vals[first:first + p], pk, t, basebit, p)
            vals[o] = TR.lut_enc(orc, [vals[x] for x in (a, b, c)[:hi[0]]], hi[1][:hi[0]], hi[2], ta[0], tb[0], 1)[0]
        elif op == TREE:
            ti, row0 = cir.ext_rows[g]
            lo, hi, p = cir.tree_specs[ti]
            ops = (a, b, c)
            rows = np.stack(cir.tv1[row0:row0 + p // lo[3]])
            vals[o] = TR.tree(orc, pk, t, basebit, [vals[x] for x in ops[:lo[0]]], lo[1][:lo[0]], lo[2], lo[3],
                              [vals[x] for x in ops[lo[0]:lo[0] + hi[0]]], hi[1][:hi[0]], hi[2], rows, p)[0]
        elif op == O.NOT:
            vals[o] = (0 - vals[a].astype(np.int64)).astype(np.int32)
        elif op == O.COPY:
            vals[o] = vals[a]
        else:
            vals[o] = orc.gates(op, vals[a][None], vals[b][None], vals[c][None] if op in (O.MUX, O.AND3) else None)[0]
    return vals
