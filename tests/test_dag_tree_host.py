"""Encrypted-table, select and tree nodes in the gate-DAG executor, host side (no GPU): Circuit.lut_enc / select / tree wire
numbering, deduplication and the six-column rows; levels() / census() of a mixed circuit; every host check of thfhe_dag_run_tree_batch, which
runs before either context is looked at; plans of node lists without the new opcodes; and the CPU yardstick (tests/dag_tree_reference.py)
decrypting a mixed circuit on reduced keys to simulate's values."""
import ctypes as C

import numpy as np
import pytest

import dag_tree_reference as DT
import lut_reference as R

I32, I64 = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
N = 1024
NAND, AND, MUX, NOT, AND3, LUT, LUT_OUT, LUT_ENC, SELECT, TREE = 0, 2, 10, 11, 13, 14, 15, 16, 17, 18


def test_opcodes_and_exports():
    import thfhe
    assert (thfhe.LUT_ENC, thfhe.SELECT, thfhe.TREE) == (16, 17, 18)
    assert "thfhe_dag_run_tree_batch" in thfhe.SIGNATURES and hasattr(thfhe.lib(), "thfhe_dag_run_tree_batch")
    assert C.sizeof(thfhe.TreeSpec) == 2 * C.sizeof(thfhe.LutSpec) + 4


def test_new_node_rows_wires_and_dedup():
    import thfhe
    from thfhe import circuits as Cc, lut
    c = Cc.Circuit()
    x = c.inputs(4)                                            # wires 0 .. 3
    rng = np.random.default_rng(1)
    ea, eb = rng.integers(-2**31, 2**31, (2, N)).astype(np.int32)
    e0 = c.enc_table(ea, eb)
    assert c.enc_table(ea.copy(), eb.copy()) == e0 and c.enc_table(eb, ea) == 1 and len(c.enc_tables) == 2
    rows2 = lut.tree_test_vectors(lambda h, l: (h + l) % 4, 4, 4, 4, theta=2)      # R = 2
    rows4 = lut.tree_test_vectors(lambda h, l: (h * l) % 4, 4, 4, 4, theta=1)      # R = 4
    r2, r4 = c.tree_rows(rows2), c.tree_rows(rows4)
    assert (r2, r4) == (0, 2) and c.tree_rows(rows2.copy()) == 0 and len(c.tv1) == 6
    o1 = c.lut_enc(e0, [x[0], x[1]], weights=(1, 2), theta=4)                     # wires 4 .. 7
    t1 = c.tree(r2, [x[0]], [x[1], x[2]], 4, hi_weights=(1, 2), theta1=2)         # 8
    s1 = c.select([x[3]], o1[0], 4)                                                # 9
    t2 = c.tree(r4, [x[2]], [x[3]], 4)                                             # 10
    t3 = c.tree(r2, [x[1]], [x[2], x[0]], 4, hi_weights=(1, 2), theta1=2)         # 11: t1's tree spec, deduplicated
    s2 = c.select([x[0], x[1]], 0, 8, weights=(1, 4), bias=7)                      # 12
    o2 = c.lut_enc(1, [s2], bias=-3)                                               # 13
    assert o1 == [4, 5, 6, 7] and (t1, s1, t2, t3, s2) == (8, 9, 10, 11, 12) and o2 == [13]
    assert c.specs == [(2, (1, 2, 0), 0, 4), (1, (1, 0, 0), -3, 1)]
    one = lambda th: (1, (1, 0, 0), 0, th)
    assert c.tree_specs == [(one(2), (2, (1, 2, 0), 0, 1), 4), (None, one(1), 4), (one(1), one(1), 4), (None, (2, (1, 4, 0), 7, 1), 8)]
    nodes = c.nodes()
    assert nodes.dtype == np.int32 and nodes.shape == (10, 6)
    assert nodes.tolist() == [
        [LUT_ENC, 0, 1, -1, 0, e0]] + [[LUT_OUT, 4, -1, -1, -1, -1]] * 3 + [
        [TREE, 0, 1, 2, 0, r2], [SELECT, 3, -1, -1, 1, 4], [TREE, 2, 3, -1, 2, r4], [TREE, 1, 2, 0, 0, r2],
        [SELECT, 0, 1, -1, 3, 0], [LUT_ENC, 12, -1, -1, 1, 1]]
    assert c.has_tree_nodes() and not c.has_luts() and c.tables == [] and c.lut_rows == {}
    for bad in (lambda: c.lut_enc(5, [x[0]]), lambda: c.lut_enc(e0, [x[0]], theta=3), lambda: c.lut_enc(e0, [x[0], x[1]]),
                lambda: c.tree(r2, [x[0], x[1]], [x[2], x[3]], 4), lambda: c.tree(r4, [x[0]], [x[1]], 8), lambda: c.tree(r2, [x[0]], [x[1]], 4, theta1=3),
                lambda: c.tree(r2, [], [x[1]], 4), lambda: c.select([x[0]], 12, 4), lambda: c.select([x[0]], 0, 6), lambda: c.select([], 0, 4),
                lambda: c.tree_rows(np.zeros(N, np.int32))):
        with pytest.raises(ValueError):
            bad()
    assert len(c.gates) == 10


def test_levels_and_census_of_a_mixed_circuit():
    import thfhe
    from thfhe import circuits as Cc, lut
    c = Cc.Circuit()
    a, b, d = c.inputs(3)
    tab = c.table(Cc.adder_table())
    rows = c.tree_rows(lut.tree_test_vectors(lambda h, l: (h + l) % 8, 8, 8, 8, theta=2))   # R = 4
    et = c.enc_table(np.zeros(N, np.int32), lut.test_vector(lut.int_outputs(lambda m: m, 4), 4))
    g = c.gate(thfhe.AND, a, b)                                  # level 1
    s, cy = c.lut(tab, [a, b], weights=(1, 1), theta=2)          # level 1
    t = c.tree(rows, [a], [b], 8, theta1=2)                      # level 1
    e = c.lut_enc(et, [d], theta=2)                              # level 1 (two wires)
    n = c.gate(thfhe.NOT, g)                                     # free
    sel = c.select([d], s, 2)                                    # level 2: candidates s, cy
    sel2 = c.select([a], e[0], 2)                                # level 2
    t2 = c.tree(rows, [sel], [t], 8, theta1=2)                   # level 3
    gi = lambda w: w - c.n_inputs
    assert c.levels() == [[gi(g), gi(s), gi(cy), gi(t), gi(e[0]), gi(e[1])], [gi(n)], [gi(sel), gi(sel2)], [gi(t2)]]
    assert c.census() == dict(gates=10, bootstrapped=7, mux=0, rotations=7 + 4 + 4, depth=3, luts=1, luts_enc=1, selects=2, trees=2)
    # a SELECT sits above its candidates even when its index operand is an input
    c2 = Cc.Circuit()
    a, b = c2.inputs(2)
    g1 = c2.gate(thfhe.AND, a, b)
    g2 = c2.gate(thfhe.AND, g1, b)
    sel = c2.select([a], g1, 2)
    assert c2.levels() == [[0], [1], [2]]


def test_circuits_without_new_nodes_are_unchanged():
    # values written down from the code before the new rows existed
    import thfhe
    from thfhe import circuits as Cc
    c = Cc.Circuit()
    a, b = c.inputs(2), c.inputs(2)
    s, cy = Cc.lut_ripple_add(c, a, b)
    g = c.gate(thfhe.NOT, Cc.to_gate_bit(c, cy))
    assert not c.has_tree_nodes() and c.enc_tables == [] and c.tree_specs == [] and c.tv1 == [] and c.ext_rows == {}
    assert c.specs == [(2, (1, 1, 0), 0, 2), (3, (1, 1, 1), 0, 2), (1, (1, 0, 0), 0, 1)] and len(c.tables) == 2
    assert c.lut_rows == {0: (0, 0), 2: (1, 0), 4: (2, 1)}
    assert c.levels() == [[0, 1], [2, 3], [4], [5]]
    assert c.census() == dict(gates=6, bootstrapped=3, mux=0, rotations=3, depth=3, luts=3)
    assert c.nodes().tolist() == [[LUT, 0, 2, -1, 0, 0], [LUT_OUT, 4, -1, -1, -1, -1], [LUT, 1, 3, 5, 1, 0], [LUT_OUT, 6, -1, -1, -1, -1],
                                  [LUT, 7, -1, -1, 2, 1], [NOT, 8, -1, -1, -1, -1]]
    # the new entry plans such a node list as the old one does: {levels, launches, rotations, widest level}
    st = np.full(4, -1, np.int64)
    rc, msg = _call(thfhe.lib(), c.nodes(), n_inputs=4, specs=c.specs, n_luts=2, stats=st)
    assert rc == -1 and "null ctx" in msg and st.tolist() == [3, 3, 3, 1]
    # gate-only circuit, boolean simulate as before
    c = Cc.Circuit()
    a, b, cin = c.inputs(2), c.inputs(2), c.inputs(1)[0]
    sm, carry = Cc.full_adder(c, a, b, cin)
    c.gate(thfhe.MUX, sm[0], sm[1], carry[0])
    v = Cc.simulate(c, [1, 0, 1, 1, 1])
    assert v.dtype == bool and v.astype(int).tolist() == [1, 0, 1, 1, 1, 1, 0, 0, 1, 1, 0, 1, 1, 0, 0]
    st = np.full(4, -1, np.int64)
    nodes = np.concatenate([np.array(c.gates, np.int32), np.full((len(c.gates), 2), -1, np.int32)], axis=1)
    rc, msg = _call(thfhe.lib(), nodes, n_inputs=5, specs=[], n_luts=0, stats=st)
    assert rc == -1 and "null ctx" in msg and st.tolist() == [5, 5, 11, 4]


SPECS = [(1, (1, 0, 0), 0, 1), (2, (1, 1, 0), 0, 2), (3, (1, 1, 1), 0, 4)]
ONE, TWO = (1, (1, 0, 0), 0, 1), (2, (1, 1, 0), 0, 1)
TREES = [(ONE, ONE, 4), ((1, (1, 0, 0), 0, 2), TWO, 4), (TWO, TWO, 8)]   # trees[2]: four operands


def _call(L, nodes, n_inputs=4, specs=SPECS, n_specs=None, tv=True, n_luts=2, enc=(True, True), n_enc=2, trees=TREES, n_trees=None, tv1=True, n_rows=6,
          out_wires=None, stats=None, entry="thfhe_dag_run_tree_batch"):
    import thfhe
    sp = (thfhe.LutSpec * max(len(specs), 1))(*[thfhe._lut_spec(s) for s in specs])
    tr = (thfhe.TreeSpec * max(len(trees), 1))(*[thfhe.TreeSpec(thfhe._lut_spec(lo), thfhe._lut_spec(hi), p) for lo, hi, p in trees])
    nodes = np.ascontiguousarray(nodes, np.int32).reshape(-1, 6)
    x = np.zeros((1, n_inputs, 631), np.int32)
    out = np.zeros((1, max(nodes.shape[0], 1), 631), np.int32)
    tab = np.zeros((8, N), np.int32)
    ptab = tab.ctypes.data_as(I32)
    sel = None if out_wires is None else np.ascontiguousarray(out_wires, np.int32)
    common = (1, None if sel is None else sel.ctypes.data_as(I32), 0 if sel is None else len(sel), out.ctypes.data_as(I32),
              None if stats is None else stats.ctypes.data_as(I64))
    head = (x.ctypes.data_as(I32), n_inputs, nodes.ctypes.data_as(I32), nodes.shape[0])
    if entry == "thfhe_dag_run_tree_batch":
        rc = L.thfhe_dag_run_tree_batch(None, None, *head, sp if specs else None, len(specs) if n_specs is None else n_specs, ptab if tv and n_luts else None, n_luts,
                                        ptab if enc[0] else None, ptab if enc[1] else None, n_enc, tr if trees else None, len(trees) if n_trees is None else n_trees,
                                        ptab if tv1 else None, n_rows, *common)
    elif entry == "thfhe_dag_run_lut_batch":
        rc = L.thfhe_dag_run_lut_batch(None, *head, sp, len(specs), ptab, n_luts, *common)
    elif entry == "thfhe_mk_dag_run_lut_batch":
        rc = L.thfhe_mk_dag_run_lut_batch(None, *head, sp, len(specs), np.zeros((2, N), np.int64).ctypes.data_as(I64), n_luts, *common)
    else:
        raise ValueError(entry)
    return rc, L.thfhe_last_error().decode()


OK_ROWS = [[LUT, 0, 1, -1, 1, 0], [LUT_OUT, 4, -1, -1, -1, -1], [NAND, 4, 5, -1, -1, -1],
           [LUT_ENC, 0, 1, 2, 2, 1], [LUT_OUT, 7, -1, -1, -1, -1], [LUT_OUT, 7, -1, -1, -1, -1], [LUT_OUT, 7, -1, -1, -1, -1],
           [SELECT, 3, -1, -1, 0, 7], [TREE, 0, 1, 2, 1, 4], [TREE, 11, 12, -1, 0, 2], [NOT, 13, -1, -1, -1, -1]]


def test_tree_dag_rejections_without_a_device():
    import thfhe
    L = thfhe.lib()

    def bad(rule, nodes, **kw):
        rc, msg = _call(L, nodes, **kw)
        assert rc == -1 and rule in msg, (rule, msg)

    # the plan of the valid list gets as far as the missing contexts, with its figures: 3 levels; launches = gates 1 + LUT 1 + LUT_ENC 1 + SELECT 1 +
    # two TREE groups x 2; rotations = 1 + 1 + 1 + 1 + (2 + 1) + (4 + 1); widest level 1
    st = np.zeros(4, np.int64)
    rc, msg = _call(L, OK_ROWS, stats=st)
    assert rc == -1 and "null ctx" in msg and st.tolist() == [3, 8, 12, 1]
    # ---- what dag_lut_plan checks
    bad("null", OK_ROWS, n_luts=2, tv=False)
    bad("null", OK_ROWS, specs=[], n_specs=1)
    bad("n_specs", OK_ROWS, n_specs=1025)
    bad("n_luts", OK_ROWS, n_luts=1025)
    bad("n_luts", OK_ROWS, n_luts=-1)
    bad("n_inputs", OK_ROWS, specs=[(1, (1, 0, 0), 0, 1), (4, (1, 1, 0), 0, 2)])
    bad("theta", OK_ROWS, specs=[(1, (1, 0, 0), 0, 3)])
    bad("output wire", OK_ROWS, out_wires=[0, 15])
    bad("spec index", [[LUT, 0, -1, -1, 3, 0]])
    bad("spec index", [[LUT_ENC, 0, -1, -1, 3, 0]])
    bad("table index", [[LUT, 0, -1, -1, 0, 2]])
    bad("operands do not match", [[LUT_ENC, 0, 1, -1, 0, 0]])
    bad("missing LUT_OUT", [[LUT_ENC, 0, 1, -1, 1, 0]])
    bad("missing LUT_OUT", [[LUT_ENC, 0, 1, -1, 1, 0], [SELECT, 0, -1, -1, 0, 0]])
    bad("without a LUT node", [[LUT_ENC, 0, -1, -1, 0, 0], [LUT_OUT, 4, -1, -1, -1, -1]])
    bad("wrong head", [[LUT_ENC, 0, 1, -1, 1, 0], [LUT_OUT, 3, -1, -1, -1, -1]])
    bad("spec and lut must be -1", [[NAND, 0, 1, -1, 0, -1]])
    bad("topological", [[TREE, 0, 4, -1, 0, 0]])
    bad("topological", [[SELECT, 5, -1, -1, 0, 0]])
    bad("opcode", [[19, 0, 1, -1, -1, -1]])
    bad("opcode", [[AND3, 0, 1, 2, -1, -1]])
    # ---- indices out of range
    bad("etab out of range", [[LUT_ENC, 0, -1, -1, 0, 2]])
    bad("etab out of range", [[LUT_ENC, 0, -1, -1, 0, -1]])
    bad("tree index out of range", [[SELECT, 0, -1, -1, 3, 0]])
    bad("tree index out of range", [[TREE, 0, 1, -1, -1, 0]])
    bad("row0 + R out of range", [[TREE, 0, 1, -1, 0, 3]])          # R = 4 rows from 3 of 6
    bad("row0 + R out of range", [[TREE, 0, 1, 2, 1, 5]])           # R = 2
    bad("row0 + R out of range", [[TREE, 0, 1, -1, 0, -1]])
    # ---- n_enc with a LUT_ENC row present
    bad("n_enc", [[LUT_ENC, 0, -1, -1, 0, 0]], enc=(False, False), n_enc=0)
    bad("n_enc", OK_ROWS, n_enc=(1 << 18) + 1)
    bad("n_enc", OK_ROWS, n_enc=-1)
    # ---- tree specs thfhe_tree_lut_bootstrap would refuse
    bad("spec_hi theta", OK_ROWS, trees=[(ONE, (1, (1, 0, 0), 0, 2), 4)])
    for p in (0, 1, 3, 6, 1024):
        bad("p_hi", OK_ROWS, trees=[(ONE, ONE, p)])
    bad("n_inputs", OK_ROWS, trees=[(ONE, (0, (1, 0, 0), 0, 1), 4)])
    bad("n_inputs", [[TREE, 0, 1, -1, 0, 0]], trees=[((4, (1, 0, 0), 0, 1), ONE, 4)])
    bad("theta", [[TREE, 0, 1, -1, 0, 0]], trees=[((1, (1, 0, 0), 0, 3), ONE, 4)])
    bad("divide", [[TREE, 0, 1, -1, 0, 0]], trees=[((1, (1, 0, 0), 0, 4), ONE, 2)])
    rc, msg = _call(L, [[SELECT, 0, -1, -1, 0, 1]], trees=[((9, (1, 0, 0), 0, 3), ONE, 2)])   # a SELECT ignores `lo`
    assert rc == -1 and "null ctx" in msg
    bad("n_trees", OK_ROWS, n_trees=1025)
    bad("n_tv1_rows", OK_ROWS, n_rows=(1 << 18) + 1)
    # ---- operand counts
    bad("operands exceed three", [[TREE, 0, 1, 2, 2, 0]])
    bad("operands do not match", [[TREE, 0, 1, -1, 1, 0]])          # trees[1]: 1 + 2 operands
    bad("operands do not match", [[TREE, 0, 1, 2, 0, 0]])           # trees[0]: 1 + 1
    bad("operands do not match", [[SELECT, 0, 1, -1, 0, 0]])        # hi names one
    bad("operands do not match", [[SELECT, 0, -1, -1, 1, 0]])       # hi names two
    # ---- SELECT candidates
    bad("candidate is not an earlier wire", [[SELECT, 0, -1, -1, 0, 1]])           # 1 .. 4: wire 4 is the node itself
    bad("candidate is not an earlier wire", [[SELECT, 0, -1, -1, 0, -1]])
    bad("candidate is not an earlier wire", [[NAND, 0, 1, -1, -1, -1], [SELECT, 0, -1, -1, 0, 2], [NAND, 0, 1, -1, -1, -1]])
    # ---- a table family that is NULL while a row refers to it
    bad("null table family", [[LUT, 0, -1, -1, 0, 0]], specs=[], n_luts=0)
    bad("null table family", [[LUT, 0, -1, -1, 0, 0]], n_luts=0)
    bad("null table family", [[LUT_ENC, 0, -1, -1, 0, 0]], specs=[])
    bad("null table family", [[LUT_ENC, 0, -1, -1, 0, 0]], enc=(False, False), n_enc=0)
    bad("null table family", [[SELECT, 0, -1, -1, 0, 0]], trees=[])
    bad("null table family", [[TREE, 0, 1, -1, 0, 0]], tv1=False, n_rows=0)
    bad("null", OK_ROWS, enc=(True, False))
    bad("null", OK_ROWS, tv1=False)
    # every family absent is a valid call for a gate-only list
    rc, msg = _call(L, [[NAND, 0, 1, -1, -1, -1]], specs=[], n_luts=0, enc=(False, False), n_enc=0, trees=[], tv1=False, n_rows=0)
    assert rc == -1 and "null ctx" in msg


@pytest.mark.parametrize("entry", ["thfhe_dag_run_lut_batch", "thfhe_mk_dag_run_lut_batch"])   # the gate-only entries want a context first: tests/test_gpu_dag_tree.py
@pytest.mark.parametrize("row", [[LUT_ENC, 0, -1, -1, 0, 0], [SELECT, 0, -1, -1, 0, 1], [TREE, 0, 1, -1, 0, 0]])
def test_old_entries_refuse_the_new_opcodes(entry, row):
    import thfhe
    rc, msg = _call(thfhe.lib(), [[NAND, 0, 1, -1, -1, -1], row], entry=entry)
    assert rc == -1 and "opcode" in msg, msg


def _mixed(K, rng, sigma_bk=2.0**-25):
    """gate -> LUT -> TREE -> SELECT over a many-LUT node's outputs -> LUT_ENC, at p = 4.  Returns (circuit, named wires)."""
    import thfhe
    from thfhe import circuits as Cc, lut
    c = Cc.Circuit()
    g0, g1, d, e, idx = c.inputs(5)
    g = c.gate(thfhe.AND, g0, g1)
    bit = Cc.from_gate_bit(c, g)                                                   # 0 / 1 at p = 4
    rows = c.tree_rows(lut.tree_test_vectors(lambda h, l: (2 * h + l + 1) % 4, 4, 4, 4, theta=2))
    t = c.tree(rows, [d], [e], 4, theta1=2)
    many = c.table(lut.test_vector([lut.int_outputs(lambda m, j=j: (m + 2 * j) % 3, 4) for j in range(4)], 4, theta=4))
    m = c.lut(many, [t], theta=4)                                                  # four outputs in 0 .. 2
    sel = c.select([idx], m[0], 4)
    tv = lut.test_vector(lut.int_outputs(lambda v: (3 * v + 1) % 4, 4), 4)
    ta, tb = lut.encrypt_table(K.rlwe_key[0], tv, sigma_bk, rng)
    out = c.lut_enc(c.enc_table(ta, tb, plain=tv), [sel, bit], weights=(1, 1))[0]   # sel + bit <= 3
    return c, dict(g=g, bit=bit, t=t, m=m, sel=sel, out=out)


def test_simulate_on_digits():
    from thfhe import circuits as Cc, lut

    class NoKey:
        rlwe_key = [np.zeros(N, np.int32)]
    c, w = _mixed(NoKey, np.random.default_rng(0), 0.0)
    for bits, d, e, idx in (((1, 1), 3, 2, 1), ((0, 1), 0, 0, 3), ((1, 0), 2, 3, 0), ((1, 1), 1, 1, 2)):
        x = np.concatenate([[lut.MU8 if b else -lut.MU8 for b in bits], lut.encode([d, e, idx], 4)])
        v = Cc.simulate(c, x)
        assert v.dtype == np.int32 and v.shape == (c.n_wires(),)
        bit = bits[0] & bits[1]
        t = (2 * e + d + 1) % 4
        m = [(t + 2 * j) % 3 for j in range(4)]
        assert (v[w["g"]] > 0) == bool(bit)
        assert lut.decode(v[[w["bit"], w["t"], w["sel"], w["out"]] + w["m"]], 4).tolist() == [bit, t, m[idx], (3 * (m[idx] + bit) + 1) % 4] + m
    # tree_mul_digits: all 64 products
    c = Cc.Circuit()
    a, b = c.inputs(2)
    lo, hi = Cc.tree_mul_digits(c, a, b)
    assert c.census() == dict(gates=2, bootstrapped=2, mux=0, rotations=10, depth=1, luts_enc=0, selects=0, trees=2)
    assert len(c.tv1) == 8 and len(c.tree_specs) == 1
    for A in range(8):
        for B in range(8):
            v = lut.decode(Cc.simulate(c, lut.encode([A, B], 8)), 8)
            assert (v[lo], v[hi]) == ((A * B) % 8, (A * B) // 8)


def test_cpu_model_decrypts_a_mixed_circuit_to_simulate(O, sk_small):
    # reduced keys (n = 16, SK-128's ring, gadget and key-switch shape).  Run alone first on these seeds: the model decrypts every case
    from thfhe import circuits as Cc, keygen, lut
    p, K, orc = sk_small
    sigma = 2.0**-15
    pk = keygen.gen_pack_key(np.random.default_rng(21), K.lwe_key, K.rlwe_key[0], p.ks_t, p.ks_basebit, 2.0**-25)
    c, w = _mixed(K, np.random.default_rng(8))
    cases = [((1, 1), 3, 2, 1), ((0, 1), 0, 0, 3), ((1, 0), 2, 3, 0), ((1, 1), 1, 1, 2)]
    for k, (bits, d, e, idx) in enumerate(cases):
        x = np.concatenate([K.encrypt_bits(list(bits), sigma, 50 + k), R.encrypt_words(K, lut.encode([d, e, idx], 4), sigma, 60 + k)])
        v = DT.evaluate(orc, c, x, pk, p.ks_t, p.ks_basebit)
        want = Cc.simulate(c, np.concatenate([[lut.MU8 if b else -lut.MU8 for b in bits], lut.encode([d, e, idx], 4)]))
        ints = [w["bit"], w["t"], w["sel"], w["out"]] + w["m"]
        assert np.array_equal(lut.decode(K.phases(v[ints]), 4), lut.decode(want[ints], 4)), (k, lut.decode(K.phases(v[ints]), 4))
        assert K.decrypt_bits(v[[w["g"]]])[0] == (want[w["g"]] > 0)
    # `only`: the SELECT alone pulls in its candidates, their head's operands and the index, and nothing else
    v1 = DT.evaluate(orc, c, x, pk, p.ks_t, p.ks_basebit, only=[w["sel"] - c.n_inputs])
    assert np.array_equal(v1[w["sel"]], v[w["sel"]]) and not v1[w["out"]].any() and not v1[w["bit"]].any()
