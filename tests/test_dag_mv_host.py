"""Multi-value nodes in the gate-DAG executor, host side (no GPU): Circuit.mv / tree_mv rows, wire numbering and
deduplication; levels() / census(); every host check of thfhe_dag_run_mv_batch, which runs before either context is looked at; the earlier
six-column entries refusing the two opcodes (the four-column ones: tests/test_gpu_dag_mv.py, they need a live context); the plan's figures; simulate of sbox_digits on all 64 inputs; and the CPU yardstick
(tests/dag_mv_reference.py) on reduced keys."""
import ctypes as C

import numpy as np
import pytest

import dag_mv_reference as DM
import lut_reference as R

I32, I64 = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
N = 1024
NAND, NOT, LUT, LUT_OUT, SELECT, TREE, MV, TREE_MV = 0, 11, 14, 15, 17, 18, 19, 20
ONE = (1, (1, 0, 0), 0, 1)
TWO = (2, (1, 2, 0), 0, 1)
# (lo, hi, p, q, k, base, factors_off, n_tables): an MV spec with q = 3 outputs and two tables, a TREE_MV spec with k = 2 outputs of p_hi = 4, an
# MV spec at q = 1
MVS = [(TWO, ONE, 8, 3, 1, 0, 0, 2), (ONE, TWO, 4, 4, 2, 1, 48, 1), (ONE, ONE, 2, 1, 1, 1, 80, 1)]
N_WORDS = 48 + 32 + 2
TREES = [(ONE, ONE, 4)]


def test_opcodes_exports_and_struct_layout():
    import thfhe
    assert (thfhe.MV, thfhe.TREE_MV) == (19, 20)
    assert "thfhe_dag_run_mv_batch" in thfhe.SIGNATURES and hasattr(thfhe.lib(), "thfhe_dag_run_mv_batch")
    assert len(thfhe.SIGNATURES["thfhe_dag_run_mv_batch"][1]) == len(thfhe.SIGNATURES["thfhe_dag_run_tree_batch"][1]) + 6
    assert C.sizeof(thfhe.MvSpec) == 2 * C.sizeof(thfhe.LutSpec) + 24


def _call(L, nodes, n_inputs=4, mvs=MVS, n_mvs=None, tv0=True, n_bases=2, fac=True, n_words=N_WORDS, trees=TREES, stats=None, entry="thfhe_dag_run_mv_batch"):
    import thfhe
    mk = lambda m: thfhe.MvSpec(thfhe._lut_spec(m[0]), thfhe._lut_spec(m[1]), *m[2:])
    mv = (thfhe.MvSpec * max(len(mvs), 1))(*[mk(m) for m in mvs])
    tr = (thfhe.TreeSpec * max(len(trees), 1))(*[thfhe.TreeSpec(thfhe._lut_spec(lo), thfhe._lut_spec(hi), p) for lo, hi, p in trees])
    sp = (thfhe.LutSpec * 1)(thfhe._lut_spec(ONE))
    nodes = np.ascontiguousarray(nodes, np.int32)
    x = np.zeros((1, n_inputs, 631), np.int32)
    out = np.zeros((1, max(nodes.shape[0], 1), 631), np.int32)
    tab = np.zeros((8, N), np.int32)
    ptab = tab.ctypes.data_as(I32)
    common = (1, None, 0, out.ctypes.data_as(I32), None if stats is None else stats.ctypes.data_as(I64))
    head = (x.ctypes.data_as(I32), n_inputs, nodes.ctypes.data_as(I32), nodes.shape[0])
    if entry == "thfhe_dag_run_mv_batch":
        rc = L.thfhe_dag_run_mv_batch(None, None, *head, sp, 1, ptab, 2, None, None, 0, tr if trees else None, len(trees), ptab, 4, mv if mvs else None,
                                      len(mvs) if n_mvs is None else n_mvs, ptab if tv0 else None, n_bases, ptab if fac else None, n_words, *common)
    elif entry == "thfhe_dag_run_tree_batch":
        rc = L.thfhe_dag_run_tree_batch(None, None, *head, sp, 1, ptab, 2, None, None, 0, tr, len(trees), ptab, 4, *common)
    elif entry == "thfhe_dag_run_lut_batch":
        rc = L.thfhe_dag_run_lut_batch(None, *head, sp, 1, ptab, 2, *common)
    elif entry == "thfhe_mk_dag_run_lut_batch":
        rc = L.thfhe_mk_dag_run_lut_batch(None, *head, sp, 1, np.zeros((2, N), np.int64).ctypes.data_as(I64), 2, *common)
    else:
        raise ValueError(entry)
    return rc, L.thfhe_last_error().decode()


OUT = lambda h: [LUT_OUT, h, -1, -1, -1, -1]
# wires: 4..6 MV (spec 0, table 1), 7 NAND, 8..9 TREE_MV (spec 1), 10 MV (spec 2), 11 LUT on an MV wire, 12 SELECT over the wires 4..7, 13..14 TREE_MV, 15 NOT
OK_ROWS = [[MV, 0, 1, -1, 0, 1], OUT(4), OUT(4), [NAND, 0, 1, -1, -1, -1], [TREE_MV, 2, 0, 1, 1, 0], OUT(8), [MV, 3, -1, -1, 2, 0],
           [LUT, 4, -1, -1, 0, 1], [SELECT, 10, -1, -1, 0, 4], [TREE_MV, 8, 9, 12, 1, 0], OUT(13), [NOT, 13, -1, -1, -1, -1]]


def test_a_valid_plan_reaches_the_contexts_and_counts():
    import thfhe
    L = thfhe.lib()
    st = np.full(4, -1, np.int64)
    rc, msg = _call(L, OK_ROWS, stats=st)
    assert rc == -1 and "null ctx" in msg, msg
    # level 1 = gate, MV spec 0, MV spec 2, TREE_MV (2 launches); level 2 = LUT (it reads an MV wire), SELECT; level 3 = TREE_MV (2).  Rotations 1 + 1 + 1 + 3, 1 + 1, 3.  The widest group holds one node.
    assert st.tolist() == [3, 9, 11, 1]
    # without TREE_MV / SELECT nodes the packing context is not asked for: only the gate context is missing
    rc, msg = _call(L, OK_ROWS[:4], stats=st)
    assert rc == -1 and "null ctx" in msg and st.tolist() == [1, 2, 2, 1]
    # the three families absent: the call is thfhe_dag_run_tree_batch
    rows = [[NAND, 0, 1, -1, -1, -1], [TREE, 0, 1, -1, 0, 0]]
    for entry in ("thfhe_dag_run_mv_batch", "thfhe_dag_run_tree_batch"):
        st[:] = -1
        rc, msg = _call(L, rows, mvs=[], tv0=False, n_bases=0, fac=False, n_words=0, stats=st, entry=entry)
        assert rc == -1 and "null ctx" in msg and st.tolist() == [1, 3, 6, 1], (entry, msg)


BAD_PLANS = [
    ("mv index", [[MV, 0, 1, -1, 3, 0], OUT(4), OUT(4)], {}, "mv index out of range"),
    ("mv index", [[MV, 0, 1, -1, -1, 0], OUT(4), OUT(4)], {}, "mv index out of range"),
    ("t", [[MV, 0, 1, -1, 0, 2], OUT(4), OUT(4)], {}, "table index out of range"),
    ("t", [[TREE_MV, 0, 1, 2, 1, -1], OUT(4)], {}, "table index out of range"),
    ("base", [[MV, 0, -1, -1, 2, 0]], dict(n_bases=1), "base out of range"),
    ("base", [[MV, 0, -1, -1, 2, 0]], dict(mvs=MVS[:2] + [(ONE, ONE, 2, 1, 1, -1, 80, 1)]), "base out of range"),
    ("factors", [[MV, 0, -1, -1, 2, 0]], dict(n_words=81), "factors_off"),
    ("factors", [[MV, 0, 1, -1, 0, 0], OUT(4), OUT(4)], dict(mvs=[(TWO, ONE, 8, 3, 1, 0, 35, 2)] + MVS[1:]), "factors_off"),
    ("factors", [[MV, 0, -1, -1, 2, 0]], dict(mvs=MVS[:2] + [(ONE, ONE, 2, 1, 1, 1, -2, 1)]), "factors_off"),
    ("spec theta", [[MV, 0, -1, -1, 2, 0]], dict(mvs=MVS[:2] + [((1, (1, 0, 0), 0, 2), ONE, 2, 1, 1, 1, 80, 1)]), "theta must be 1"),
    ("spec p", [[MV, 0, -1, -1, 2, 0]], dict(mvs=MVS[:2] + [(ONE, ONE, 3, 1, 1, 1, 80, 1)]), "p must be"),
    ("spec q", [[MV, 0, -1, -1, 2, 0]], dict(mvs=MVS[:2] + [(ONE, ONE, 2, 65, 1, 1, 0, 1)], n_words=4096), "q must be"),
    ("spec q", [[MV, 0, -1, -1, 2, 0]], dict(mvs=MVS[:2] + [(ONE, ONE, 2, 0, 1, 1, 80, 1)]), "q must be"),
    ("spec n_tables", [[MV, 0, -1, -1, 2, 0]], dict(mvs=MVS[:2] + [(ONE, ONE, 2, 1, 1, 1, 80, 0)]), "n_tables"),
    ("MV on k = 2", [[MV, 0, -1, -1, 1, 0], OUT(4), OUT(4), OUT(4)], {}, "k must be 1"),
    ("tree p_hi", [[TREE_MV, 0, 1, 2, 0, 0]], {}, "p_hi must be"),                                        # spec 0 has q = 3
    ("tree k", [[TREE_MV, 0, 1, 2, 1, 0]], dict(mvs=[MVS[0], (ONE, TWO, 4, 4, 0, 1, 48, 1), MVS[2]]), "k must be"),
    ("tree k q", [[TREE_MV, 0, 1, 2, 1, 0]] + [OUT(4)] * 16, dict(mvs=[MVS[0], (ONE, TWO, 4, 4, 17, 1, 0, 1), MVS[2]], n_words=1 << 20), "k p_hi must be at most 64"),
    ("tree hi theta", [[TREE_MV, 0, 1, 2, 1, 0], OUT(4)], dict(mvs=[MVS[0], (ONE, (2, (1, 2, 0), 0, 2), 4, 4, 2, 1, 48, 1), MVS[2]]), "spec_hi theta"),
    ("tree hi spec", [[TREE_MV, 0, 1, 2, 1, 0], OUT(4)], dict(mvs=[MVS[0], (ONE, (4, (1, 2, 0), 0, 1), 4, 4, 2, 1, 48, 1), MVS[2]]), "n_inputs"),
    ("LUT_OUT missing", [[MV, 0, 1, -1, 0, 0], OUT(4), [NAND, 0, 1, -1, -1, -1]], {}, "missing LUT_OUT"),
    ("LUT_OUT missing at the end", [[TREE_MV, 0, 1, 2, 1, 0]], {}, "missing LUT_OUT"),
    ("LUT_OUT extra", [[MV, 0, 1, -1, 0, 0], OUT(4), OUT(4), OUT(4)], {}, "LUT_OUT row without"),
    ("LUT_OUT extra after q = 1", [[MV, 0, -1, -1, 2, 0], OUT(4)], {}, "LUT_OUT row without"),
    ("LUT_OUT wrong head", [[TREE_MV, 0, 1, 2, 1, 0], OUT(3)], {}, "wrong head"),
    ("operands", [[MV, 0, -1, -1, 0, 0], OUT(4), OUT(4)], {}, "operands do not match"),
    ("operands", [[MV, 0, 1, 2, 0, 0], OUT(4), OUT(4)], {}, "operands do not match"),
    ("operands", [[TREE_MV, 0, 1, -1, 1, 0], OUT(4)], {}, "operands do not match"),
    ("operands exceed three", [[TREE_MV, 0, 1, 2, 1, 0], OUT(4)], dict(mvs=[MVS[0], (TWO, TWO, 4, 4, 2, 1, 48, 1), MVS[2]]), "exceed three"),
    ("operand order", [[MV, 0, 4, -1, 0, 0], OUT(4), OUT(4)], {}, "not an earlier wire"),
    ("null mvs", [[MV, 0, 1, -1, 0, 0], OUT(4), OUT(4)], dict(mvs=[]), "null table family"),
    ("null bases", [[MV, 0, 1, -1, 0, 0], OUT(4), OUT(4)], dict(tv0=False, n_bases=0), "null table family"),
    ("null factors", [[MV, 0, 1, -1, 0, 0], OUT(4), OUT(4)], dict(fac=False, n_words=0), "null table family"),
    ("count without pointer", [[NAND, 0, 1, -1, -1, -1]], dict(tv0=False), "count but no pointer"),
    ("count without pointer", [[NAND, 0, 1, -1, -1, -1]], dict(fac=False), "count but no pointer"),
    ("n_mvs", [[NAND, 0, 1, -1, -1, -1]], dict(n_mvs=1025), "n_mvs"),
    ("n_mvs", [[NAND, 0, 1, -1, -1, -1]], dict(n_mvs=0), "n_mvs"),
    ("n_bases", [[NAND, 0, 1, -1, -1, -1]], dict(n_bases=1025), "n_bases"),
    ("n_factor_words", [[NAND, 0, 1, -1, -1, -1]], dict(n_words=(1 << 28) + 1), "n_factor_words"),
    ("earlier checks stay", [[TREE, 0, 1, -1, 1, 0]], {}, "tree index out of range"),
    ("earlier checks stay", [[21, 0, 1, -1, -1, -1]], {}, "opcode not defined"),
]


@pytest.mark.parametrize("what, rows, kw, needle", BAD_PLANS, ids=[f"{i}-{b[0]}" for i, b in enumerate(BAD_PLANS)])
def test_every_plan_error_comes_before_the_contexts(what, rows, kw, needle):
    import thfhe
    rc, msg = _call(thfhe.lib(), rows, **kw)
    assert rc == -1 and needle in msg and "null ctx" not in msg, msg


@pytest.mark.parametrize("op", [MV, TREE_MV])
def test_the_earlier_node_list_entries_refuse_the_two_opcodes(op):
    import thfhe
    L = thfhe.lib()
    row6 = [[op, 0, 1, 2 if op == TREE_MV else -1, 0 if op == MV else 1, 0]] + [OUT(4)] * (2 if op == MV else 1)
    for entry in ("thfhe_dag_run_tree_batch", "thfhe_dag_run_lut_batch", "thfhe_mk_dag_run_lut_batch"):
        rc, msg = _call(L, row6, entry=entry)
        assert rc == -1 and "opcode not defined" in msg, (entry, msg)
    # thfhe_dag_run(_batch) and thfhe_mk_dag_run(_batch) look at their context before they plan, so a NULL-context call cannot show their refusal:
    # tests/test_gpu_dag_mv.py shows it with live contexts


def test_circuit_rows_wires_dedup_levels_and_census():
    import thfhe
    from thfhe import circuits as Cc, lut
    c = Cc.Circuit()
    x = c.inputs(3)                                                      # wires 0 .. 2
    rng = np.random.default_rng(2)
    tv0 = lut.mv_base(1 << 30)
    b0 = c.mv_base(tv0)
    assert c.mv_base(tv0.copy()) == b0 and c.mv_base(lut.mv_base(1 << 29)) == 1 and len(c.mv_bases) == 2
    wa, wb = rng.integers(-9, 9, (2, 3, 8)).astype(np.int32)
    wt = rng.integers(-9, 9, (2, 4, 4)).astype(np.int32)
    m1 = c.mv(b0, wa, [x[0], x[1]], weights=(1, 2))                      # 3, 4, 5
    g = c.gate(thfhe.NAND, x[0], x[1])                                   # 6
    m2 = c.mv(b0, wb, [x[1], x[2]], weights=(1, 2))                      # 7, 8, 9: m1's spec, its second table
    t1 = c.tree_mv(1, wt, [x[2]], [x[0], x[1]], hi_weights=(1, 2))       # 10, 11
    m3 = c.mv(b0, wa.copy(), [g, m2[2]], weights=(1, 2))                 # 12, 13, 14: table 0 again, level 2
    s = c.select([t1[1]], m3[0], 2)                                      # 15: level 3, candidates 12, 13
    t2 = c.tree_mv(1, wt, [s], [m1[0], x[1]], hi_weights=(1, 2))         # 16, 17: level 4
    n = c.gate(thfhe.NOT, t2[1])                                         # 18
    assert (m1, g, m2, t1, m3, s, t2, n) == ([3, 4, 5], 6, [7, 8, 9], [10, 11], [12, 13, 14], 15, [16, 17], 18)
    two, one = (2, (1, 2, 0), 0, 1), (1, (1, 0, 0), 0, 1)
    assert [sp[:6] for sp in c.mv_specs] == [[two, None, 8, 3, 1, 0], [one, two, 4, 4, 2, 1]]
    assert [len(sp[6]) for sp in c.mv_specs] == [2, 1]
    assert c.mv_rows == {0: (0, 0), 4: (0, 1), 7: (1, 0), 9: (0, 0), 13: (1, 0)}
    assert c.has_mv_nodes() and c.has_tree_nodes() and not c.has_luts()
    out = lambda h: [LUT_OUT, h, -1, -1, -1, -1]
    assert c.nodes().tolist() == [[MV, 0, 1, -1, 0, 0], out(3), out(3), [NAND, 0, 1, -1, -1, -1], [MV, 1, 2, -1, 0, 1], out(7), out(7),
                                  [TREE_MV, 2, 0, 1, 1, 0], out(10), [MV, 6, 9, -1, 0, 0], out(12), out(12), [SELECT, 11, -1, -1, 0, 12],
                                  [TREE_MV, 15, 3, 1, 1, 0], out(16), [NOT, 17, -1, -1, -1, -1]]
    mvs, bases, fac = c.mv_families()
    assert mvs == [(two, None, 8, 3, 1, 0, 0, 2), (one, two, 4, 4, 2, 1, 48, 1)] and bases.shape == (2, N)
    assert fac.dtype == np.int32 and np.array_equal(fac, np.concatenate([wa.ravel(), wb.ravel(), wt.ravel()]))
    assert c.levels() == [[0, 1, 2, 3, 4, 5, 6, 7, 8], [9, 10, 11], [12], [13, 14], [15]]
    assert c.census() == dict(gates=16, bootstrapped=7, mux=0, rotations=7 + 2 + 2, depth=4, luts_enc=0, selects=1, trees=0, mvs=3, tree_mvs=2)
    # the library plans these rows to the same figures: levels, launches (level 1: gate, MV, TREE_MV x 2; MV; SELECT; TREE_MV x 2), rotations
    st = np.full(4, -1, np.int64)
    rc, msg = _call(thfhe.lib(), c.nodes(), n_inputs=3, mvs=[(m[0], m[1] or ONE) + m[2:] for m in mvs], n_words=len(fac), trees=[(ONE, ONE, 2)], stats=st)
    assert rc == -1 and "null ctx" in msg and st.tolist() == [4, 8, 11, 2], (msg, st)
    for bad in (lambda: c.mv(5, wa, [x[0]]), lambda: c.mv(b0, wa[0], [x[0]]), lambda: c.mv(b0, wa, [x[0], x[1]]), lambda: c.mv(b0, np.zeros((3, 6), np.int32), [x[0]]),
                lambda: c.mv(b0, np.zeros((65, 2), np.int32), [x[0]]), lambda: c.tree_mv(b0, wt, [x[0], x[1]], [x[2], x[0]]),
                lambda: c.tree_mv(b0, wt, [], [x[0]]), lambda: c.tree_mv(b0, wt[0], [x[0]], [x[1]]), lambda: c.tree_mv(b0, np.zeros((17, 4, 4), np.int32), [x[0]], [x[1]]),
                lambda: c.tree_mv(b0, np.zeros((2, 3, 4), np.int32), [x[0]], [x[1]])):
        with pytest.raises(ValueError):
            bad()
    assert len(c.gates) == 16


def test_sbox_digits_simulates_on_all_64_inputs():
    from thfhe import circuits as Cc, lut
    table = np.random.default_rng(9).integers(0, 16, 64)
    c = Cc.Circuit()
    hi, lo = c.inputs(2)
    bits = Cc.sbox_digits(c, hi, lo, table)
    assert bits == [2, 3, 4, 5] and c.nodes().tolist() == [[TREE_MV, 1, 0, -1, 0, 0]] + [[LUT_OUT, 2, -1, -1, -1, -1]] * 3
    assert c.mv_specs[0][2:5] == [8, 8, 4] and c.census()["rotations"] == 5 and c.levels() == [[0, 1, 2, 3]]
    for h in range(8):
        for l in range(8):
            v = Cc.simulate(c, lut.encode(np.array([h, l]), 8))
            assert v.dtype == np.int32
            d = lut.decode(v[bits], 2)
            assert int((d << np.arange(4)).sum()) == table[8 * h + l], (h, l)
    with pytest.raises(ValueError):
        Cc.sbox_digits(c, hi, lo, list(range(63)))


def test_simulate_of_mv_and_select():
    # an MV node's q = 4 wires as a SELECT's candidates: f_j(m) for j = the selecting digit
    from thfhe import circuits as Cc, lut
    F = np.array([[0, 1, 1, 0], [1, 1, 0, 0], [0, 0, 0, 1], [1, 0, 1, 1]])
    c = Cc.Circuit()
    m, j = c.inputs(2)
    outs = c.mv(c.mv_base(lut.mv_base(1 << 30)), lut.mv_factors(F, 4), [m])
    s = c.select([j], outs[0], 4)
    for mm in range(4):
        for jj in range(4):
            v = Cc.simulate(c, lut.encode(np.array([mm, jj]), 4))
            assert lut.decode(v[outs], 2).tolist() == F[:, mm].tolist() and lut.decode(v[s:s + 1], 2)[0] == F[jj, mm]


def test_cpu_yardstick_decrypts_a_mixed_circuit_on_reduced_keys(sk_small):
    # the model of the executor (dag_mv_reference) on n = 16 keys: an MV node, a SELECT over its wires and a TREE_MV node decrypt to simulate's digits
    from thfhe import circuits as Cc, keygen, lut
    p, K, orc = sk_small
    pk = keygen.gen_pack_key(np.random.default_rng(12), K.lwe_key, K.rlwe_key[0], p.ks_t, p.ks_basebit, 2.0**-25)
    F = np.array([[0, 1, 1, 0], [1, 1, 0, 0], [0, 0, 0, 1], [1, 0, 1, 1]])
    c = Cc.Circuit()
    m, j = c.inputs(2)
    b0 = c.mv_base(lut.mv_base(1 << 30))
    outs = c.mv(b0, lut.mv_factors(F, 4), [m])
    s = c.select([j], outs[0], 4)
    tv0, w = lut.tree_mvk_factors([lambda h, l: (h ^ l) & 1, lambda h, l: int(h >= l)], 4, 4)
    t = c.tree_mv(c.mv_base(tv0), w, [m], [j])
    for mm, jj in ((0, 0), (1, 3), (2, 1), (3, 2)):
        x = R.encrypt_words(K, lut.encode(np.array([mm, jj]), 4), 2.0**-15, 60 + mm)
        vals = DM.evaluate(orc, c, x, pk, p.ks_t, p.ks_basebit)
        sim = Cc.simulate(c, lut.encode(np.array([mm, jj]), 4))
        got = lut.decode(K.phases(vals[2:]), 2)
        assert got.tolist() == lut.decode(sim[2:], 2).tolist() == F[:, mm].tolist() + [F[jj, mm], (jj ^ mm) & 1, int(jj >= mm)], (mm, jj)
