"""Circuit-bootstrap nodes in the gate-DAG executor, host side (no GPU): the opcode, the exported entries and the struct
layouts; every host check of thfhe_dag_run_cb_batch, made with NULL contexts and NULL sets, which proves it runs before either is looked at; with
cb = NULL the answers of thfhe_dag_run_lhe_batch; every other six-column entry refusing the opcode; the planner through stats (a leveled row inherits
its depth from its set, the CB nodes of a level are one group, stats[4] in both modes, a circuit without CB nodes plans as before); Circuit.cb_set rows,
levels(), census() and the families; simulate against the plain twins of cb_lookup_dag, cb_array_read and cb_mux_max; the model decoding every case
of tests/dag_cb_cases.py; and the boundary lines of tests/cb_cases.py still in the sources."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import cb_cases as CC
import dag_cb_cases as DC

I32, I64 = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
N = 1024
NAND, XOR, MUX, NOT, LUT_OUT, LOOKUP, GATHER, WFA, CB = 0, 3, 10, 11, 15, 21, 22, 23, 24
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# one client set (index 0) and two computed sets (indices 1, 2): d = 3 on pool wires 0, 2, 8 (8 is a gate wire) and d = 2 on pool wires 1, 3
CBS = [(3, 0), (2, 3)]
POOL = [0, 2, 8, 1, 3]
# (set, d_tree, d_rot, theta): on the client set, on computed set 0 (d = 3), on computed set 1 (d = 2), a gather on computed set 1
LKS = [(0, 1, 2, 1), (1, 1, 2, 1), (2, 0, 2, 1), (2, 1, 1, 1)]
# (n_steps, n_states, theta, n_out, set0, n_sets, trans_off, step_off, start_off): 2 steps over the client set and computed set 0 (a mixed spec)
WFAS = [(2, 2, 1, 1, 0, 2, 0, 8, 10)]
WORDS = [0, 1, 1, 0, 1, 1, 0, 0] + [16 * 0 + 1, 16 * 1 + 2] + [0]


def _call(L, nodes, n_inputs=8, cbs=CBS, n_cbs=None, pool=POOL, n_pool=None, mode=0, lks=LKS, wfas=WFAS, sets=1, cb=True, lhe=True, stats=None,
          entry="thfhe_dag_run_cb_batch"):
    """the entry with NULL contexts and NULL sets: every answer comes from the host checks"""
    import thfhe
    lk = (thfhe.DagLheSpec * max(len(lks), 1))(*[thfhe.DagLheSpec(*k) for k in lks])
    wf = (thfhe.DagWfaSpec * max(len(wfas), 1))(*[thfhe.DagWfaSpec(*a) for a in wfas])
    hs = (C.c_void_p * max(sets, 1))()
    words = np.array(WORDS, np.int32)
    t = np.zeros((8, N), np.int32)
    pt = t.ctypes.data_as(I32)
    fam = thfhe.DagLheFamilies(hs if sets else None, sets, lk if lks else None, len(lks), None, pt, 6, wf if wfas else None, len(wfas), words.ctypes.data_as(I32),
                               len(words), None, pt, 4)
    cs = (thfhe.DagCbSpec * max(len(cbs), 1))(*[thfhe.DagCbSpec(*s) for s in cbs])
    pl = np.array(pool, np.int32)
    cbf = thfhe.DagCbFamilies(cs if cbs else None, len(cbs) if n_cbs is None else n_cbs, pl.ctypes.data_as(I32) if len(pl) else None,
                              len(pl) if n_pool is None else n_pool, mode, None)
    sp = (thfhe.LutSpec * 1)(thfhe._lut_spec((1, (1, 0, 0), 0, 1)))
    nodes = np.ascontiguousarray(nodes, np.int32).reshape(-1, 6)
    x = np.zeros((1, n_inputs, 17), np.int32)
    out = np.zeros((1, max(nodes.shape[0], 1), 17), np.int32)
    common = (1, None, 0, out.ctypes.data_as(I32), None if stats is None else stats.ctypes.data_as(I64))
    head = (x.ctypes.data_as(I32), n_inputs, nodes.ctypes.data_as(I32), nodes.shape[0])
    mid = (sp, 1, pt, 2, None, None, 0, None, 0, None, 0, None, 0, None, 0, None, 0)
    pf = C.byref(fam) if lhe else None
    if entry == "thfhe_dag_run_cb_batch":
        rc = L.thfhe_dag_run_cb_batch(None, None, None, *head, *mid, pf, C.byref(cbf) if cb else None, *common)
    elif entry == "thfhe_dag_run_lhe_batch":
        rc = L.thfhe_dag_run_lhe_batch(None, None, *head, *mid, pf, *common)
    elif entry == "thfhe_dag_run_mv_batch":
        rc = L.thfhe_dag_run_mv_batch(None, None, *head, *mid, *common)
    elif entry == "thfhe_dag_run_tree_batch":
        rc = L.thfhe_dag_run_tree_batch(None, None, *head, *mid[:11], *common)
    elif entry == "thfhe_dag_run_lut_batch":
        rc = L.thfhe_dag_run_lut_batch(None, *head, sp, 1, pt, 2, *common)
    elif entry == "thfhe_mk_dag_run_lut_batch":
        rc = L.thfhe_mk_dag_run_lut_batch(None, *head, sp, 1, np.zeros((2, N), np.int64).ctypes.data_as(I64), 2, *common)
    else:
        raise ValueError(entry)
    return rc, L.thfhe_last_error().decode()


G = lambda op, a, b: [op, a, b, -1, -1, -1]
CBR = lambda s: [CB, -1, -1, -1, s, -1]
LK = lambda lk, row0: [LOOKUP, -1, -1, -1, lk, row0]
GA = lambda lk, first: [GATHER, -1, -1, -1, lk, first]
WF = lambda wfa, fin0: [WFA, -1, -1, -1, wfa, fin0]
GOOD = [G(XOR, 0, 1),      # 8   level 1
        CBR(0),            # 9   level 2: its pool holds wire 8
        CBR(1),            # 10  level 1: inputs only
        LK(0, 0),          # 11  level 1: the client's set
        LK(1, 0),          # 12  level 3: computed set 0
        LK(2, 0),          # 13  level 2: computed set 1
        G(NAND, 12, 13),   # 14  level 4
        WF(0, 0)]          # 15  level 3: the client's set and computed set 0


def test_opcode_exports_and_struct_layout():
    import thfhe
    assert thfhe.CB == 24
    for name in ("thfhe_dag_run_cb_batch", "thfhe_dag_cb_release"):
        assert name in thfhe.SIGNATURES and hasattr(thfhe.lib(), name)
    assert len(thfhe.SIGNATURES["thfhe_dag_run_cb_batch"][1]) == len(thfhe.SIGNATURES["thfhe_dag_run_lhe_batch"][1]) + 2
    assert C.sizeof(thfhe.DagCbSpec) == 8 and C.sizeof(thfhe.DagCbFamilies) == 48
    assert thfhe.lib().thfhe_dag_cb_release(None) == -1


def test_a_good_plan_passes_the_host_checks_and_stops_at_the_contexts():
    import thfhe
    L = thfhe.lib()
    st = np.full(5, -7, np.int64)
    rc, msg = _call(L, GOOD, stats=st, mode=1)
    assert rc == -1 and "null tgsw set" in msg, msg          # the plan is accepted: the first thing missing is the client's set
    # 4 levels.  Launch groups: level 1: the XOR, CB(set 1), lookup lk 0 | level 2: CB(set 0), lookup lk 2 | level 3: lookup lk 1, the automaton |
    # level 4: the NAND.  One level-1 rotation per gate; the widest group is one node.  5 level-2 rotations per instance in one-rotation mode.
    assert st.tolist() == [4, 8, 2, 1, 5]
    st[:] = -7
    rc, msg = _call(L, GOOD, stats=st, mode=0)
    assert rc == -1 and st.tolist() == [4, 8, 2, 1, 0]       # per level: sum d x l, written once the context is known


def test_two_cb_nodes_of_one_level_are_one_group_and_a_leveled_row_sits_above_its_set():
    import thfhe
    L = thfhe.lib()
    st = np.zeros(5, np.int64)
    # both CB nodes on inputs: ONE group on level 1; both lookups on level 2 although they have no wire operands
    rc, msg = _call(L, [CBR(0), CBR(1), LK(0, 0), LK(1, 0)], pool=[0, 2, 4, 1, 3], sets=0, lks=[(0, 1, 2, 1), (1, 0, 2, 1)], wfas=[], stats=st, mode=1)
    assert rc == -1 and "null ctx" in msg, msg               # no client set: the first thing missing is the context
    assert st.tolist() == [2, 3, 0, 2, 5]
    # a GATHER on computed set 1 whose candidates are inputs: its depth is its set's, not its candidates'
    rc, msg = _call(L, [G(XOR, 0, 1), G(XOR, 8, 2), CBR(0), CBR(1), GA(0, 0)], pool=[0, 2, 9, 1, 3], sets=0, lks=[(1, 1, 1, 1)], wfas=[], stats=st, mode=1)
    assert rc == -1 and "null ctx" in msg, msg
    assert st.tolist() == [3, 5, 2, 1, 5]                    # XOR, CB(set 1) | XOR, the GATHER on set 1 | CB(set 0)


def test_a_circuit_without_cb_nodes_plans_as_before():
    import thfhe
    L = thfhe.lib()
    nodes = [G(XOR, 0, 1), LK(0, 0), GA(0, 2), G(NAND, 9, 10)]
    a, b = np.zeros(5, np.int64), np.zeros(5, np.int64)
    ra = _call(L, nodes, stats=a, cb=False, wfas=[])
    rb = _call(L, nodes, stats=b, entry="thfhe_dag_run_lhe_batch", wfas=[])
    assert ra == rb and ra[0] == -1 and "null tgsw set" in ra[1]
    assert a.tolist() == b.tolist() and a[4] == 0 and a[0] == 3


BAD = [
    ("mode must be", GOOD, dict(mode=2)),
    ("mode must be", GOOD, dict(mode=-1)),
    ("cb: n_sets must be", GOOD, dict(n_cbs=0)),
    ("cb: n_sets must be", GOOD, dict(n_cbs=65)),
    ("cb: n_sets must be", GOOD, dict(cbs=[], n_cbs=2)),
    ("client sets \\+ computed sets", GOOD, dict(sets=63)),
    ("cb: d must be", GOOD, dict(cbs=[(0, 0), (2, 3)])),
    ("cb: d must be", GOOD, dict(cbs=[(17, 0), (2, 3)])),
    ("past the wire pool", GOOD, dict(cbs=[(3, 0), (2, 4)])),
    ("past the wire pool", GOOD, dict(cbs=[(3, -1), (2, 3)])),
    ("past the wire pool", GOOD, dict(n_pool=4)),
    ("a count but no pointer", GOOD, dict(pool=[], n_pool=5)),
    ("pool wire is not an earlier wire", GOOD, dict(pool=[0, 2, 9, 1, 3])),        # the CB row's own wire
    ("pool wire is not an earlier wire", GOOD, dict(pool=[0, 2, 8, 1, -1])),
    ("pool wire is not an earlier wire", [CBR(0), G(XOR, 0, 1), CBR(1)], {}),      # wire 8 is the CB row itself, the gate comes later
    ("cbset out of range", [G(XOR, 0, 1), CBR(2), CBR(1)], {}),
    ("cbset out of range", [G(XOR, 0, 1), CBR(-1), CBR(1)], {}),
    ("no CB row", [G(XOR, 0, 1), CBR(0)], {}),
    ("has a CB row already", [G(XOR, 0, 1), CBR(0), CBR(0), CBR(1)], {}),
    ("before the set's CB row", [G(XOR, 0, 1), LK(1, 0), CBR(0), CBR(1)], {}),
    ("before the set's CB row", [G(XOR, 0, 1), CBR(1), WF(0, 0), CBR(0)], {}),     # a mixed automaton: its computed set comes later
    ("operand fields and field 5", [G(XOR, 0, 1), [CB, 0, -1, -1, 0, -1], CBR(1)], {}),
    ("operand fields and field 5", [G(XOR, 0, 1), [CB, -1, -1, 2, 0, -1], CBR(1)], {}),
    ("operand fields and field 5", [G(XOR, 0, 1), [CB, -1, -1, -1, 0, 0], CBR(1)], {}),
    ("d_tree \\+ d_rot must equal the set's d", [G(XOR, 0, 1), CBR(0), CBR(1), LK(1, 0)], dict(lks=[(0, 1, 2, 1), (1, 1, 1, 1)])),
    ("d_tree \\+ d_rot must equal the set's d", [G(XOR, 0, 1), CBR(0), CBR(1), GA(1, 0)], dict(lks=[(0, 1, 2, 1), (2, 1, 2, 1)])),
    ("set is out of range", [G(XOR, 0, 1), CBR(0), CBR(1), LK(1, 0)], dict(lks=[(0, 1, 2, 1), (3, 1, 2, 1)])),
    ("set0 \\+ n_sets out of range", [G(XOR, 0, 1), CBR(0), CBR(1), WF(0, 0)], dict(wfas=[(2, 2, 1, 1, 2, 2, 0, 8, 10)])),
    ("step_bit must name", [G(XOR, 0, 1), CBR(0), CBR(1), WF(0, 0)], dict(sets=0, wfas=[(2, 2, 1, 1, 0, 2, 0, 8, 10)])),   # bit 2 of computed set 1 (d = 2)
    ("not defined for this engine", GOOD, dict(cb=False)),                       # without the family the call is thfhe_dag_run_lhe_batch
    ("not an earlier wire", [G(NAND, 0, 9)], {}),                                  # ... and the earlier checks stay
    ("null family", [LK(0, 0)], dict(lks=[], cbs=CBS)),
]


@pytest.mark.parametrize("case", range(len(BAD)))
def test_refusals_before_any_context_or_set_is_looked_at(case):
    import thfhe
    what, nodes, kw = BAD[case]
    rc, msg = _call(thfhe.lib(), nodes, **kw)
    assert rc == -1 and re.search(what, msg), (what, msg)
    assert "null ctx" not in msg and "null tgsw set" not in msg


def test_without_the_family_the_call_is_the_leveled_entry():
    import thfhe
    import test_dag_lhe_host as LH
    L = thfhe.lib()
    for nodes, kw in [([LK(0, 0)], {}), ([LK(0, 7)], {}), ([GA(0, 1)], {}), ([LK(0, 0)], dict(lks=[(0, 7, 0, 1)])), ([WF(0, 0)], dict(wfas=[(2, 65, 1, 1, 0, 1, 0, 8, 10)])),
                      ([LK(0, 0)], dict(sets=65)), ([LK(0, 0)], dict(lhe=False)), ([CBR(0)], {}), ([G(NAND, 0, 9)], {}), ([LK(0, 0), [LUT_OUT, 8, -1, -1, -1, -1]], {})]:
        a, b = np.zeros(5, np.int64), np.zeros(5, np.int64)
        ra = _call(L, nodes, cb=False, stats=a, **kw)
        rb = _call(L, nodes, entry="thfhe_dag_run_lhe_batch", stats=b, **kw)
        assert ra == rb and ra[0] == -1, (nodes, kw, ra, rb)
        assert a.tolist() == b.tolist()
    assert len(LH.BAD) > 40                  # the leveled entry's own refusals are tests/test_dag_lhe_host.py's, unchanged


@pytest.mark.parametrize("entry", ["thfhe_dag_run_lhe_batch", "thfhe_dag_run_mv_batch", "thfhe_dag_run_tree_batch", "thfhe_dag_run_lut_batch",
                                   "thfhe_mk_dag_run_lut_batch"])
def test_every_other_entry_rejects_the_opcode(entry):
    import thfhe
    rc, msg = _call(thfhe.lib(), [CBR(0)], entry=entry)
    assert rc == -1 and "not defined for this engine" in msg, msg


def test_circuit_rows_levels_and_families():
    from thfhe import circuits as CI
    cir = CI.Circuit()
    x = cir.inputs(4)
    g = cir.gate(XOR, x[0], x[1])
    s0 = cir.cb_set([x[2], g])
    own = cir.n_wires() - 1
    s1 = cir.cb_set([x[3]])
    tab = cir.lhe_table(np.zeros((2, N), np.int32))
    a = cir.lhe_lookup(s0, tab, 1, 1)[0]
    b = cir.lhe_lookup(0, tab, 0, 1)[0]          # a client set beside them
    c = cir.lhe_lookup(s1, tab, 0, 1)[0]
    assert (s0, s1) == (CI.CB_SET_BASE, CI.CB_SET_BASE + 1) and cir.has_cb_nodes() and cir.n_lhe_sets() == 1
    assert cir.nodes()[own - 4].tolist() == [CB, -1, -1, -1, 0, -1]
    fam = cir.cb_families()
    assert fam["cb_sets"] == [(2, 0), (1, 2)] and fam["cb_wires"].tolist() == [x[2], g, x[3]]
    assert [k[0] for k in cir.lhe_families()["lks"]] == [1, 0, 2]          # the client's sets first, then the computed ones
    lv = cir.levels()
    depth = {gi + 4: d for d, level in enumerate(lv) for gi in level}
    assert [depth[w] for w in (g, own, own + 1, a, b, c)] == [0, 1, 0, 2, 0, 1]
    assert cir.census()["cbs"] == 2 and cir.census()["cb_bits"] == 3 and cir.census()["bootstrapped"] == 1
    with pytest.raises(ValueError):
        cir.lhe_lookup(s0, tab, 0, 1)            # d_tree + d_rot != 2
    with pytest.raises(ValueError):
        cir.cb_set([cir.n_wires()])
    with pytest.raises(ValueError):
        cir.lhe_wfa(CI.wfa_equal(1), [0, s0], cir.lhe_finals(np.zeros((4, N), np.int32)))


def test_simulate_agrees_with_the_plain_twins():
    from thfhe import circuits as CI
    rng = np.random.default_rng(0xDCB0)
    table = rng.integers(0, 8, 8)
    cir = CI.Circuit()
    a, b = cir.inputs(3), cir.inputs(3)
    out = CI.cb_lookup_dag(cir, a, b, table, d_tree=1)
    from thfhe import lut
    for va in range(8):
        for vb in range(8):
            bits = [(va >> i) & 1 for i in range(3)] + [(vb >> i) & 1 for i in range(3)]
            assert lut.decode(CI.simulate(cir, DC.GATE(bits))[out], 8) == CI.cb_lookup_plain(va, vb, table)
    cir = CI.Circuit()
    x = cir.inputs(11)
    out = CI.cb_array_read(cir, x[:8], [x[10], x[8], x[9]], 1, 2)         # not consecutive, not in order
    for addr in range(8):
        bits = rng.integers(0, 2, 11)
        bits[[10, 8, 9]] = [(addr >> i) & 1 for i in range(3)]
        assert (CI.simulate(cir, DC.GATE(bits))[out] > 0) == bool(bits[addr])
    cir = CI.Circuit()
    a, b = cir.inputs(3), cir.inputs(3)
    out = CI.cb_mux_max(cir, a, b, 3)
    for va in range(8):
        for vb in range(8):
            bits = [(va >> (2 - i)) & 1 for i in range(3)] + [(vb >> (2 - i)) & 1 for i in range(3)]
            got = CI.simulate(cir, DC.GATE(bits))[out] > 0
            assert int((got << np.arange(2, -1, -1)).sum()) == max(va, vb)


@pytest.mark.parametrize("case", range(len(DC.ALL)))
def test_the_model_decodes_every_case(O, case):
    name, make = DC.ALL[case]
    c = make(O)                                  # the builders assert the decode
    assert c["ref"].size and c["rows"] is not None, name


def test_the_slice_boundaries_are_still_in_the_sources():
    for name, (value, fname, pattern) in CC.BOUNDARIES.items():
        m = re.search(pattern, open(os.path.join(ROOT, "torus-fhe_amd", "csrc", fname)).read())
        assert m and int(m.group(1)) == value, name
    src = open(os.path.join(ROOT, "torus-fhe_amd", "csrc", "thfhe_dag_cb.h")).read()
    assert "kCbSliceBits / bits" in src          # the group's slice rule is sized by the same constant
    assert DC.SLICE_INSTANCES * 3 == CC.SLICE_BITS + 1
