"""Dense-layer nodes in the gate-DAG executor, host side (no GPU): the opcode, the exported entries and the struct layouts;
every host check of thfhe_dag_run_dense_batch and thfhe_mk_dag_run_dense_batch, made with NULL contexts, which proves it runs before a context is
looked at; with dense = NULL the answers of the entries below them; every other six-column entry refusing the opcode; the planner through stats (the
DENSE rows of a level that share an entry are one group, M rotations per node); Circuit.dense_layer / dense rows, pools, de-duplication, levels()
and census(); simulate against dense_plain; dense_network and dense_argmax against their plain twins."""
import ctypes as C
import re

import numpy as np
import pytest

import test_dag_cb_host as CBH

I32, I64 = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
N = 1024
NAND, XOR, NOT, LUT, LUT_OUT, DENSE = 0, 3, 11, 14, 15, 25
# (M, K, theta, w_off, bias_off, lut_off): a 2 x 3 layer with bias and per-output tables, a 1 x 2 layer of theta = 2 without either
LAYERS = [(2, 3, 1, 0, 6, 8), (1, 2, 2, 10, -1, -1)]
WORDS = [1, -2, 3, 4, 5, -6] + [7, 8] + [1, 0] + [9, -9]
POOL = [2, 0, 1, 3, 3, 4, 8, 5]     # descending, a repeat, a node's output next to an input
ENTRIES = ["thfhe_dag_run_dense_batch", "thfhe_mk_dag_run_dense_batch"]

G = lambda op, a, b: [op, a, b, -1, -1, -1]
D = lambda off, layer: [DENSE, off, -1, -1, layer, -1]
OUT = lambda head: [LUT_OUT, head, -1, -1, -1, -1]
GOOD = [D(0, 0), OUT(8),      # 8, 9    level 1, layer 0
        D(3, 0), OUT(10),     # 10, 11  level 1, layer 0: the same entry at another wire_off
        D(6, 1), OUT(12),     # 12, 13  level 2, layer 1 (theta = 2): pool wires 8 and 5
        G(NAND, 9, 13)]       # 14      level 3


def _call(L, nodes, entry=ENTRIES[0], n_inputs=8, layers=LAYERS, n_layers=None, words=WORDS, n_words=None, pool=POOL, n_pool=None, n_luts=2, dense=True,
          stats=None):
    """the entry with NULL contexts: every answer comes from the host checks"""
    import thfhe
    ls = (thfhe.DagDenseSpec * max(len(layers), 1))(*[thfhe.DagDenseSpec(*l) for l in layers])
    w, pl = np.array(words, np.int32), np.array(pool, np.int32)
    fam = thfhe.DagDenseFamilies(ls if layers else None, len(layers) if n_layers is None else n_layers, w.ctypes.data_as(I32) if len(w) else None,
                                 len(w) if n_words is None else n_words, pl.ctypes.data_as(I32) if len(pl) else None, len(pl) if n_pool is None else n_pool)
    sp = (thfhe.LutSpec * 1)(thfhe._lut_spec((1, (1, 0, 0), 0, 1)))
    nodes = np.ascontiguousarray(nodes, np.int32).reshape(-1, 6)
    x = np.zeros((1, n_inputs, 17), np.int32)
    out = np.zeros((1, max(nodes.shape[0], 1), 17), np.int32)
    head = (x.ctypes.data_as(I32), n_inputs, nodes.ctypes.data_as(I32), nodes.shape[0])
    tail = (C.byref(fam) if dense else None, 1, None, 0, out.ctypes.data_as(I32), None if stats is None else stats.ctypes.data_as(I64))
    mk = entry.startswith("thfhe_mk_")
    t = np.zeros((2, N), np.int64 if mk else np.int32)
    pt = t.ctypes.data_as(I64 if mk else I32) if n_luts else None
    fams = (sp, 1, pt, n_luts, None, None, 0, None, 0, None, 0, None, 0, None, 0, None, 0)
    if entry == "thfhe_dag_run_dense_batch":
        rc = L.thfhe_dag_run_dense_batch(None, None, None, *head, *fams, None, None, *tail)
    elif entry == "thfhe_mk_dag_run_dense_batch":
        rc = L.thfhe_mk_dag_run_dense_batch(None, *head, *fams, None, *tail)
    elif entry == "thfhe_mk_dag_run_tree_batch":
        rc = L.thfhe_mk_dag_run_tree_batch(None, *head, *fams, None, *tail[1:])
    elif entry == "thfhe_mk_dag_run_mv_batch":
        rc = L.thfhe_mk_dag_run_mv_batch(None, *head, sp, 1, pt, n_luts, None, 0, None, 0, None, 0, None, *tail[1:])
    else:
        raise ValueError(entry)
    return rc, L.thfhe_last_error().decode()


def test_opcode_exports_and_struct_layout():
    import thfhe
    assert thfhe.DENSE == 25
    for name in ENTRIES:
        assert name in thfhe.SIGNATURES and hasattr(thfhe.lib(), name)
    sig = thfhe.SIGNATURES
    assert len(sig["thfhe_dag_run_dense_batch"][1]) == len(sig["thfhe_dag_run_cb_batch"][1]) + 1
    assert len(sig["thfhe_mk_dag_run_dense_batch"][1]) == len(sig["thfhe_mk_dag_run_tree_batch"][1]) + 1
    # the family pointer sits right before `instances`, after every argument of the entry below
    assert sig["thfhe_dag_run_dense_batch"][1][:-6] == sig["thfhe_dag_run_cb_batch"][1][:-5]
    assert sig["thfhe_mk_dag_run_dense_batch"][1][:-6] == sig["thfhe_mk_dag_run_tree_batch"][1][:-5]
    assert C.sizeof(thfhe.DagDenseSpec) == 24 and C.sizeof(thfhe.DagDenseFamilies) == 48
    assert "thfhe_dag_last_stage_ms" in thfhe.SIGNATURES and thfhe.lib().thfhe_dag_last_stage_ms(None, None) == -1
    src = open(CBH.ROOT + "/include/thfhe_hip.h").read()
    assert "THFHE_DENSE = 25" in src and "thfhe_dag_dense_spec" in src and "int32_t M, K;" in src


@pytest.mark.parametrize("entry", ENTRIES)
def test_a_good_plan_passes_the_host_checks_and_stops_at_the_context(entry):
    import thfhe
    st = np.full(5, -7, np.int64)
    rc, msg = _call(thfhe.lib(), GOOD, entry=entry, stats=st)
    assert rc == -1 and "null ctx" in msg, msg
    # 3 levels; launch groups: the two layer-0 nodes of level 1 as ONE group, the layer-1 node, the NAND; rotations 2 x 2 + 1 + 1; widest group 2 nodes
    assert st[:4].tolist() == [3, 3, 6, 2]


@pytest.mark.parametrize("entry", ENTRIES)
def test_two_nodes_of_one_entry_are_one_group_and_another_entry_is_another(entry):
    import thfhe
    st = np.zeros(5, np.int64)
    # all three on level 1: layer 0 twice (one group), layer 1 once -> 2 groups, M1 2 + M2 = 5 rotations; the NOT of a LUT_OUT wire rides on the level
    nodes = [D(0, 0), OUT(8), D(3, 0), OUT(10), D(6, 1), OUT(12), G(NOT, 11, -1)]
    rc, msg = _call(thfhe.lib(), nodes, entry=entry, pool=[2, 0, 1, 3, 3, 4, 7, 5], stats=st)
    assert rc == -1 and "null ctx" in msg, msg
    assert st[:4].tolist() == [1, 2, 5, 2]


def test_a_circuit_without_dense_nodes_plans_as_before():
    import thfhe
    L = thfhe.lib()
    nodes = [G(XOR, 0, 1), [LUT, 8, -1, -1, 0, 1], G(NAND, 8, 9)]
    a, b = np.zeros(5, np.int64), np.zeros(5, np.int64)
    ra = _call(L, nodes, stats=a)
    rb = CBH._call(L, nodes, stats=b, cb=False, lhe=False)
    assert ra == rb and ra[0] == -1 and "null ctx" in ra[1]
    assert a.tolist() == b.tolist() and a[:4].tolist() == [3, 3, 3, 1]
    a[:], b[:] = 0, 0
    ra = _call(L, nodes, entry="thfhe_mk_dag_run_dense_batch", stats=a)
    rb = _call(L, nodes, entry="thfhe_mk_dag_run_tree_batch", stats=b)
    assert ra == rb and a.tolist() == b.tolist() and a[:4].tolist() == [3, 3, 3, 1]


def _words(at, v):
    w = list(WORDS)
    w[at] = v
    return w


def _pool(at, v):
    q = list(POOL)
    q[at] = v
    return q


def _layer(i, field, v):
    ls = [list(l) for l in LAYERS]
    ls[i][field] = v
    return [tuple(l) for l in ls]


BAD = [
    ("a count but no pointer", GOOD, dict(layers=[], n_layers=2)),
    ("a count but no pointer", GOOD, dict(words=[], n_words=12)),
    ("a count but no pointer", GOOD, dict(pool=[], n_pool=8)),
    ("n_layers must be", GOOD, dict(n_layers=0)),
    ("n_layers must be", GOOD, dict(n_layers=1025)),
    ("n_layers must be", GOOD, dict(layers=[], n_layers=0)),
    ("n_words must be", GOOD, dict(n_words=0)),
    ("n_words must be", GOOD, dict(n_words=(1 << 28) + 1)),
    ("n_words must be", GOOD, dict(words=[], n_words=0)),
    ("M and K must be", GOOD, dict(layers=_layer(0, 0, 0))),
    ("M and K must be", GOOD, dict(layers=_layer(0, 0, 65537))),
    ("M and K must be", GOOD, dict(layers=_layer(1, 1, 0))),
    ("M and K must be", GOOD, dict(layers=_layer(1, 1, 65537))),
    ("theta must be 1, 2 or 4", GOOD, dict(layers=_layer(0, 2, 3))),
    ("theta must be 1, 2 or 4", GOOD, dict(layers=_layer(1, 2, 0))),
    ("w_off \\+ M K runs past", GOOD, dict(layers=_layer(0, 3, 7))),
    ("w_off \\+ M K runs past", GOOD, dict(layers=_layer(1, 3, 11))),
    ("w_off \\+ M K runs past", GOOD, dict(layers=_layer(0, 3, -1))),
    ("w_off \\+ M K runs past", GOOD, dict(n_words=11)),
    ("bias_off \\+ M runs past", GOOD, dict(layers=_layer(0, 4, 11))),
    ("bias_off \\+ M runs past", GOOD, dict(layers=_layer(0, 4, -2))),
    ("lut_off \\+ M runs past", GOOD, dict(layers=_layer(0, 5, 11))),
    ("lut_off \\+ M runs past", GOOD, dict(layers=_layer(1, 5, 12))),
    ("lut_off entry is out of range", GOOD, dict(words=_words(8, 2))),
    ("lut_off entry is out of range", GOOD, dict(words=_words(9, -1))),
    ("lut_off entry is out of range", GOOD, dict(n_luts=1)),
    ("layer out of range", [D(0, 2), OUT(8)], {}),
    ("layer out of range", [D(0, -1), OUT(8)], {}),
    ("wire_off \\+ K runs past the wire pool", [D(6, 0), OUT(8)], {}),
    ("wire_off \\+ K runs past the wire pool", [D(-1, 0), OUT(8)], {}),
    ("wire_off \\+ K runs past the wire pool", GOOD, dict(n_pool=7)),
    ("pool wire is not an earlier wire", GOOD, dict(pool=_pool(0, 8))),              # the row's own wire
    ("pool wire is not an earlier wire", GOOD, dict(pool=_pool(4, -1))),
    ("pool wire is not an earlier wire", GOOD, dict(pool=_pool(6, 12))),             # the third node reading itself
    ("pool wire is not an earlier wire", [D(6, 1), OUT(8), D(0, 0), OUT(10)], {}),   # pool wire 8 is the row itself
    ("operand fields 2, 3 and field 5", [[DENSE, 0, 1, -1, 0, -1], OUT(8)], {}),
    ("operand fields 2, 3 and field 5", [[DENSE, 0, -1, 2, 0, -1], OUT(8)], {}),
    ("operand fields 2, 3 and field 5", [[DENSE, 0, -1, -1, 0, 0], OUT(8)], {}),
    ("missing LUT_OUT row", [D(0, 0)], {}),
    ("missing LUT_OUT row", [D(0, 0), G(NAND, 0, 1)], {}),
    ("missing LUT_OUT row", [D(6, 1)], dict(pool=_pool(6, 7))),
    ("LUT_OUT row without", [D(0, 0), OUT(8), OUT(8)], {}),
    ("names the wrong head", [D(0, 0), OUT(9)], {}),
    ("names the wrong head", [D(0, 0), OUT(8), D(3, 0), OUT(8)], {}),
    ("no tables given", GOOD, dict(n_luts=0)),
    ("not defined for this engine", GOOD, dict(dense=False)),                        # without the family the call is the entry below
    ("not an earlier wire", [G(NAND, 0, 9)], {}),                                    # ... and the earlier checks stay
]


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("case", range(len(BAD)))
def test_refusals_before_any_context_is_looked_at(case, entry):
    import thfhe
    what, nodes, kw = BAD[case]
    rc, msg = _call(thfhe.lib(), nodes, entry=entry, **kw)
    assert rc == -1 and re.search(what, msg), (what, msg)
    assert "null ctx" not in msg


@pytest.mark.parametrize("entry", ["thfhe_dag_run_cb_batch", "thfhe_dag_run_lhe_batch", "thfhe_dag_run_mv_batch", "thfhe_dag_run_tree_batch",
                                   "thfhe_dag_run_lut_batch", "thfhe_mk_dag_run_lut_batch", "thfhe_mk_dag_run_mv_batch", "thfhe_mk_dag_run_tree_batch"])
def test_every_other_entry_rejects_the_opcode(entry):
    import thfhe
    call = _call if entry in ("thfhe_mk_dag_run_mv_batch", "thfhe_mk_dag_run_tree_batch") else CBH._call
    rc, msg = call(thfhe.lib(), [D(0, 0), OUT(8)], entry=entry)
    assert rc == -1 and "not defined for this engine" in msg, msg


def _network():
    """inputs -> two windows of one 2 x 3 layer and a 1 x 2 layer on another entry, all on level 1 -> a NOT of a LUT_OUT wire"""
    from thfhe import circuits as CI
    from thfhe import lut
    cir = CI.Circuit()
    x = cir.inputs(6)
    t0 = cir.table(lut.test_vector(lut.int_outputs(lambda s: (s + 1) % 8, 8), 8))
    t1 = cir.table(lut.test_vector(lut.int_outputs(lambda s: (3 * s) % 8, 8), 8))
    W = [[1, 1, 0], [0, 1, 2]]
    bias = CI.dense_bias(W, 8, m_max=1)
    la = cir.dense_layer(W, bias, [t1, t0])
    lb = cir.dense_layer([[1, 1]], None, None, theta=2)
    a = cir.dense(la, [x[2], x[1], x[0]])
    b = cir.dense(la, [x[3], x[3], x[4]])
    c = cir.dense(lb, [x[5], x[0]])
    return cir, x, (t0, t1), (W, bias), (la, lb), (a, b, c)


def test_circuit_rows_pools_and_deduplication():
    from thfhe import circuits as CI
    cir, x, (t0, t1), (W, bias), (la, lb), (a, b, c) = _network()
    assert cir.dense_layer(W, bias, [t1, t0]) == la and cir.dense_layer(W, bias, [t0, t1]) != la       # equal layers share one id
    assert len(cir.dense_specs) == 3 and cir.has_dense_nodes()
    assert a == [[6], [7]] and b == [[8], [9]] and c == [[10, 11]]
    rows = cir.nodes()
    assert rows[0].tolist() == [DENSE, 0, -1, -1, la, -1] and rows[1].tolist() == [LUT_OUT, 6, -1, -1, -1, -1]
    assert rows[2].tolist() == [DENSE, 3, -1, -1, la, -1] and rows[4].tolist() == [DENSE, 6, -1, -1, lb, -1] and rows[5].tolist() == [LUT_OUT, 10, -1, -1, -1, -1]
    fam = cir.dense_families()
    assert fam["dense_wires"].tolist() == [x[2], x[1], x[0], x[3], x[3], x[4], x[5], x[0]]
    assert fam["dense_layers"][:2] == [(2, 3, 1, 0, 6, 8), (1, 2, 2, 10, -1, -1)]
    assert fam["dense_words"][:12].tolist() == [1, 1, 0, 0, 1, 2] + list(bias) + [t1, t0] + [1, 1]
    with pytest.raises(ValueError):
        cir.dense(la, [x[0], x[1]])                      # K = 3
    with pytest.raises(ValueError):
        cir.dense(lb, [x[0], cir.n_wires()])             # not defined above the node
    with pytest.raises(ValueError):
        cir.dense_layer(W, bias, [t0, 7])                # unknown table
    with pytest.raises(ValueError):
        cir.dense_layer(W, bias[:1])


def test_levels_and_census_of_two_nodes_on_one_entry_and_one_on_another():
    import thfhe
    cir, x, _, _, _, (a, b, c) = _network()
    n = cir.gate(NOT, b[1][0])
    g = cir.gate(NAND, a[0][0], c[0][1])
    lv = cir.levels()
    depth = {gi + 6: d for d, level in enumerate(lv) for gi in level}
    assert [depth[w] for w in (a[0][0], a[1][0], b[0][0], c[0][0], c[0][1], n, g)] == [0, 0, 0, 0, 0, 1, 2]
    cen = cir.census()
    assert cen["denses"] == 3 and cen["rotations"] == 2 * 2 + 1 + 1 and cen["depth"] == 2 and cen["bootstrapped"] == 4
    # the native planner agrees: 2 groups on the DENSE level (+ the NAND's), M1 2 + M2 rotations (+ the NAND's)
    fam = cir.dense_families()
    st = np.zeros(5, np.int64)
    rc, msg = _call(thfhe.lib(), cir.nodes(), n_inputs=6, layers=fam["dense_layers"][:2], words=fam["dense_words"].tolist(), pool=fam["dense_wires"].tolist(), stats=st)
    assert rc == -1 and "null ctx" in msg, msg
    assert st[:4].tolist() == [2, 3, 6, 2]


def test_simulate_agrees_with_dense_plain():
    from thfhe import circuits as CI
    from thfhe import lut
    cir, x, (t0, t1), (W, bias), _, (a, b, c) = _network()
    off = CI.dense_bias_messages(W, 8, m_max=1)
    rng = np.random.default_rng(0xDE25)
    for _ in range(16):
        bits = rng.integers(0, 2, 6)
        v = CI.simulate(cir, lut.encode(bits, 8))
        for outs, ins in ((a, [2, 1, 0]), (b, [3, 3, 4])):
            s = CI.dense_plain(W, off, bits[ins], 8)
            assert s.max() < 8
            want = [(3 * int(s[0])) % 8, (int(s[1]) + 1) % 8]
            assert lut.decode(v[[outs[0][0], outs[1][0]]], 8).tolist() == want
        s = int(CI.dense_plain([[1, 1]], None, bits[[5, 0]], 8)[0])
        assert lut.decode(v[c[0][0]], 8) == (s + 1) % 8          # theta = 2 on table 0: output 0 is the table's value
        assert np.array_equal(CI.simulate_mk(cir, lut.encode(bits, 8)), v)


def test_dense_network_and_argmax_against_their_plain_twins():
    from thfhe import circuits as CI
    from thfhe import lut
    p = 8
    cir = CI.Circuit()
    x = cir.inputs(5)
    relu = cir.table(lut.test_vector(lut.int_outputs(lambda s: min(s, 3), p), p))
    W1 = np.array([[1, 1, 0, 0, 0], [0, 1, 1, 1, 0], [1, 0, 1, 0, 1], [0, 0, 0, 1, 1]])
    W2 = np.array([[1, 0, 1, 0], [0, 1, 0, 1], [1, 1, 0, 0]])
    layers = CI.dense_network(cir, x, [(W1, None, [relu] * 4), (W2, None, [relu] * 3)])
    assert [len(l) for l in layers] == [4, 3] and len(cir.dense_specs) == 2
    win = CI.dense_argmax(cir, layers[-1], p)
    assert cir.census()["denses"] == 2 and cir.census()["luts"] == 3
    seen = set()
    for m in range(32):
        bits = np.array([(m >> i) & 1 for i in range(5)])
        h = np.minimum(CI.dense_plain(W1, None, bits, p), 3)
        s = np.minimum(CI.dense_plain(W2, None, h, p), 3)
        v = CI.simulate(cir, lut.encode(bits, p))
        assert lut.decode(v[layers[-1]], p).tolist() == s.tolist()
        got = (v[win] > 0).astype(np.int64)
        assert got.tolist() == CI.dense_argmax_plain(s).tolist() and got.sum() == 1
        seen.add(int(got.argmax()))
    assert seen == {0, 1, 2}
