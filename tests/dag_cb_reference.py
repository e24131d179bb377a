"""CPU yardstick of the gate-DAG executor with circuit-bootstrap nodes (thfhe_dag_run_cb_batch) -- TEST INFRASTRUCTURE ONLY, single
key.  It adds no arithmetic of its own: a circuit level by level, a CB node's TGSW rows through cb_reference.circuit_bootstrap (per level) or
cb_one_reference.circuit_bootstrap_one (one rotation) on the model's OWN wires, a leveled row through dag_lhe_reference.leveled on the client's
samples or on those rows, every other row as dag_lhe_reference.evaluate does it (the oracle's gates)."""
import numpy as np

import cb_one_reference as C1
import cb_reference as CB
import dag_lhe_reference as DL
import oracle_lib as O

CB_OP, LUT_OUT = 24, 15


class Sets:
    """what dag_lhe_reference.leveled indexes by a circuit's set ids: the client's samples below CB_SET_BASE, the computed rows from it on"""
    def __init__(self, client, computed, base):
        self.client, self.computed, self.base = list(client), computed, base

    def one(self, s):
        return self.computed[s - self.base] if s >= self.base else self.client[s]

    def __getitem__(self, key):
        if isinstance(key, slice):
            return [self.one(s) for s in range(key.start, key.stop)]
        return self.one(key)


def cb_rows(S, recs, t, basebit, one_rotation):
    """int32[d][2l][2][N]: the TGSW rows of the d gate records `recs` under the keys S (cb_cases.Keys)"""
    l, Bgbit = S.tp.l, S.tp.Bgbit
    fn = C1.circuit_bootstrap_one if one_rotation else CB.circuit_bootstrap
    return fn(S.orc2, S.pks, np.ascontiguousarray(recs), l, Bgbit, t, basebit)


def evaluate(S, cir, input_records, Cs, t, basebit, one_rotation=False, pk=None, only=None):
    """(int32[n_wires][words], {computed set: its rows int32[d][2l][2][N]}) of one instance.  S: cb_cases.Keys (orc, orc2, pks; tp, p); Cs: the
    instance's CLIENT TGSW samples per set; t, basebit: the private key's; pk: the packing key (GATHER nodes).  only: the gate indices to compute
    (with every row they read, a computed set's CB row and its operands included); None = all."""
    from thfhe.circuits import CB_SET_BASE
    n_in = cir.n_inputs
    words = np.asarray(input_records).shape[-1]
    vals = np.zeros((cir.n_wires(), words), np.int32)
    vals[:n_in] = np.asarray(input_records, np.int32).reshape(n_in, words)
    cb_gate = {c: g for g, (c, _) in cir.cb_rows.items()}

    def reads(g):
        op = cir.gates[g][0]
        if op == CB_OP:
            return list(cir.cb_specs[cir.cb_rows[g][0]])
        r = DL.reads(cir, g)
        if op in (DL.LHE_LOOKUP, DL.LHE_GATHER):
            ids = [cir.lhe_specs[cir.lhe_rows[g][0]][0]]
        elif op == DL.LHE_WFA:
            spec = cir.wfa_specs[cir.lhe_rows[g][0]]
            ids = range(spec[4], spec[4] + spec[5])
        else:
            ids = []
        return r + [n_in + cb_gate[s - CB_SET_BASE] for s in ids if s >= CB_SET_BASE]

    need = None
    if only is not None:
        need, todo = set(), list(only)
        while todo:
            g = todo.pop()
            if g not in need:
                need.add(g)
                todo += [w - n_in for w in reads(g) if w >= n_in]
    computed = {}
    sets = Sets(Cs, computed, CB_SET_BASE)
    for level in cir.levels():
        for g in level:
            op, a, b, c = cir.gates[g]
            if (need is not None and g not in need) or op == LUT_OUT:
                continue
            o = n_in + g
            if op == CB_OP:
                wires = cir.cb_specs[cir.cb_rows[g][0]]
                computed[cir.cb_rows[g][0]] = cb_rows(S, vals[wires], t, basebit, one_rotation).reshape(len(wires), 2 * S.tp.l, 2, -1)
                vals[o] = vals[wires[0]]
            elif op in (DL.LHE_LOOKUP, DL.LHE_GATHER, DL.LHE_WFA):
                r = DL.leveled(S.orc, cir, g, vals, sets, pk, S.p.ks_t, S.p.ks_basebit)
                vals[o:o + r.shape[0]] = r
            elif op == O.NOT:
                vals[o] = (0 - vals[a].astype(np.int64)).astype(np.int32)
            elif op == O.COPY:
                vals[o] = vals[a]
            else:
                vals[o] = S.orc.gates(op, vals[a][None], vals[b][None], vals[c][None] if op in (O.MUX, O.AND3) else None)[0]
    return vals, computed
