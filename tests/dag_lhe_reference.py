"""CPU yardstick of the gate-DAG executor with leveled nodes (thfhe_dag_run_lhe_batch) -- TEST INFRASTRUCTURE ONLY, single key.  It adds
no arithmetic of its own: a circuit's rows in order, LHE_LOOKUP nodes through lhe_reference.lookup, LHE_GATHER nodes through the box packing of
tree_lut_reference (as dag_tree_reference packs a SELECT's candidates) and lhe_reference.lookup on the packed samples, LHE_WFA nodes through
wfa_reference.wfa, every other row through dag_mv_reference / dag_tree_reference (the oracle's gates, the LUT models)."""
import numpy as np

import lhe_reference as LR
import oracle_lib as O
import tree_lut_reference as TR
import wfa_reference as WR

LUT_OUT, LHE_LOOKUP, LHE_GATHER, LHE_WFA = 15, 21, 22, 23


def reads(cir, g):
    """The wires row g reads: its operands, a LUT_OUT row's head, a GATHER's candidates."""
    op, a, b, c = cir.gates[g]
    if op == LUT_OUT:
        return [a]
    r = [w for w in (a, b, c) if w >= 0]
    if op == LHE_GATHER:
        lk, first = cir.lhe_rows[g]
        r += list(range(first, first + (1 << (cir.lhe_specs[lk][1] + cir.lhe_specs[lk][2]))))
    return r


def leveled(orc, cir, g, vals, Cs, pk=None, t=None, basebit=None):
    """The records int32[outputs][words] of the leveled row g on one instance: Cs = its TGSW samples, a list over the sets of int32[d][2l][2][N]."""
    op = cir.gates[g][0]
    x, y = cir.lhe_rows[g]
    fam = cir.lhe_families()
    if op == LHE_WFA:
        trans, step_bit, start, theta, set0, n_sets = cir.wfa_specs[x]
        n = trans.shape[1]
        r = WR.wfa(orc, Cs[set0:set0 + n_sets], trans, step_bit, None if fam["fin_a"] is None else fam["fin_a"][y:y + n], fam["fin_b"][y:y + n], theta, start)
        return r.reshape(-1, r.shape[-1])
    set_id, d_tree, d_rot, theta = cir.lhe_specs[x]
    if op == LHE_GATHER:
        tab_a, tab_b = TR.pack_boxes(vals[y:y + (1 << (d_tree + d_rot))], pk, t, basebit, 1 << d_rot)
    else:
        tab_b = fam["tab_b"][y:y + (1 << d_tree)]
        tab_a = None if fam["tab_a"] is None else fam["tab_a"][y:y + (1 << d_tree)]
    return LR.lookup(orc, Cs[set_id], tab_a, tab_b, d_tree, d_rot, theta)


def evaluate(orc, cir, input_records, Cs, pk=None, t=None, basebit=None, only=None):
    """int32[n_wires][words] of one instance.  Cs: the instance's TGSW samples per set; pk, t, basebit: the packing key (GATHER nodes).  only: the
    gate indices to compute (with every row they read); None = all.  Circuits here hold gates, NOT / COPY and leveled nodes (plus LUT nodes through
    dag_tree_reference when the circuit has them)."""
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
        if op in (LHE_LOOKUP, LHE_GATHER, LHE_WFA):
            r = leveled(orc, cir, g, vals, Cs, pk, t, basebit)
            vals[o:o + r.shape[0]] = r
        elif op == 14:   # a LUT node: the model of dag_tree_reference
            import lut_reference as R
            si, ti = cir.lut_rows[g]
            nin, w, bias, theta = cir.specs[si]
            vals[o:o + theta] = R.lut_bootstrap(orc, [vals[x] for x in (a, b, c)[:nin]], w[:nin], bias, np.asarray(cir.tables[ti]), theta)
        elif op == O.NOT:
            vals[o] = (0 - vals[a].astype(np.int64)).astype(np.int32)
        elif op == O.COPY:
            vals[o] = vals[a]
        else:
            vals[o] = orc.gates(op, vals[a][None], vals[b][None], vals[c][None] if op in (O.MUX, O.AND3) else None)[0]
    return vals
