"""Encrypted-table, tree and multi-value tree nodes in the 3-gen gate-DAG executor, host side (no GPU): the plan's figures
for circuits mixing gate, LUT, MV, LUT_ENC, TREE and TREE_MV rows, every host check of thfhe_mk_dag_run_tree_batch (they run before the context is
looked at), SELECT's refusal with its own message, the older entries still refusing the opcodes, and the Circuit helpers on Torus64 tables.  The
golden plans of tests/test_dag_plan.py belong to the other entries and are not touched."""
import ctypes as C

import numpy as np
import pytest

I32, I64 = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
N = 1024
NAND, MUX, NOT, LUT, LUT_OUT, LUT_ENC, SELECT, TREE, MV, TREE_MV = 0, 9, 11, 14, 15, 16, 17, 18, 19, 20
ONE = (1, (1, 0, 0), 0, 1)
ONE2 = (1, (1, 0, 0), 0, 2)          # theta = 2
TWO = (2, (1, 2, 0), 0, 1)
SPECS = [ONE, ONE2]
TREES = [(ONE2, ONE, 4), (ONE, TWO, 2)]          # (lo, hi, p_hi): R = 2 rows; R = 2 rows with a two-operand selection
# (lo, hi, p, q, k, base, factors_off, n_tables): an MV spec of q = 3; a TREE_MV spec of k = 2 tables of p_hi = q = 4 candidates of p_lo = 4 taps
MVS = [(ONE, ONE, 4, 3, 1, 0, 0, 2), (ONE, ONE, 4, 4, 2, 1, 24, 1)]
N_WORDS = 24 + 32
OUT = lambda h: [LUT_OUT, h, -1, -1, -1, -1]


def _call(L, nodes, n_inputs=2, specs=SPECS, tv=True, n_luts=2, enc=(True, True), n_enc=2, trees=TREES, n_trees=None, tv1=True, n_rows=4, mvs=MVS, n_mvs=None,
          tv0=True, n_bases=2, fac=True, n_words=N_WORDS, bias=True, stats=None, entry="thfhe_mk_dag_run_tree_batch"):
    import thfhe
    spec = lambda s: thfhe._lut_spec(s)
    mv = (thfhe.MvSpec * max(len(mvs), 1))(*[thfhe.MvSpec(spec(m[0]), spec(m[1]), *m[2:]) for m in mvs])
    tr = (thfhe.TreeSpec * max(len(trees), 1))(*[thfhe.TreeSpec(spec(t[0]), spec(t[1]), t[2]) for t in trees])
    sp = (thfhe.LutSpec * max(len(specs), 1))(*[spec(s) for s in specs])
    nodes = np.ascontiguousarray(nodes, np.int32)
    x = np.zeros((1, n_inputs, 1041), np.int32)
    out = np.zeros((1, max(nodes.shape[0], 1), 1041), np.int32)
    tab = np.zeros((4, N), np.int64)
    words = np.zeros(4096, np.int32)
    ob = np.zeros(max(len(mvs), 1), np.int64)
    ptab = tab.ctypes.data_as(I64)
    common = (1, None, 0, out.ctypes.data_as(I32), None if stats is None else stats.ctypes.data_as(I64))
    head = (x.ctypes.data_as(I32), n_inputs, nodes.ctypes.data_as(I32), nodes.shape[0])
    luts = (sp if specs else None, len(specs), ptab if tv else None, n_luts)
    mvf = (mv if mvs else None, len(mvs) if n_mvs is None else n_mvs, ptab if tv0 else None, n_bases, words.ctypes.data_as(I32) if fac else None, n_words,
           ob.ctypes.data_as(I64) if bias else None)
    if entry == "thfhe_mk_dag_run_tree_batch":
        rc = L.thfhe_mk_dag_run_tree_batch(None, *head, *luts, ptab if enc[0] else None, ptab if enc[1] else None, n_enc, tr if trees else None,
                                           len(trees) if n_trees is None else n_trees, ptab if tv1 else None, n_rows, *mvf, *common)
    elif entry == "thfhe_mk_dag_run_mv_batch":
        rc = L.thfhe_mk_dag_run_mv_batch(None, *head, *luts, *mvf, *common)
    elif entry == "thfhe_mk_dag_run_lut_batch":
        rc = L.thfhe_mk_dag_run_lut_batch(None, *head, *luts, *common)
    else:
        raise ValueError(entry)
    return rc, L.thfhe_last_error().decode()


# wires: 2 NAND; 3 LUT on it; 4 TREE (tree 0, rows 0 .. 1) lo = 3, hi = 0; 5, 6 TREE_MV (mv 1) lo = 4, hi = 1; 7 LUT_ENC on 5 (table 1); 8 NAND(7, 6)
CHAIN = [[NAND, 0, 1, -1, -1, -1], [LUT, 2, -1, -1, 0, 1], [TREE, 3, 0, -1, 0, 0], [TREE_MV, 4, 1, -1, 1, 0], OUT(5), [LUT_ENC, 5, -1, -1, 0, 1],
         [NAND, 7, 6, -1, -1, -1]]


def test_symbol_and_signature():
    import thfhe
    assert "thfhe_mk_dag_run_tree_batch" in thfhe.SIGNATURES and hasattr(thfhe.lib(), "thfhe_mk_dag_run_tree_batch")
    # enc_a, enc_b, n_enc, trees, n_trees, tv1, n_tv1_rows after the LUT family
    assert len(thfhe.SIGNATURES["thfhe_mk_dag_run_tree_batch"][1]) == len(thfhe.SIGNATURES["thfhe_mk_dag_run_mv_batch"][1]) + 7


def test_valid_plans_reach_the_context_and_count():
    import thfhe
    L = thfhe.lib()
    st = np.full(4, -1, np.int64)
    rc, msg = _call(L, CHAIN, stats=st)
    assert rc == -1 and "null ctx" in msg, msg
    # six levels; launches 1 + 1 + 2 (TREE) + 2 (TREE_MV) + 1 + 1; rotations 1 + 1 + (R + 1 = 3) + (1 + k = 3) + 1 + 1
    assert st.tolist() == [6, 8, 10, 1]
    # one level: two TREE nodes of one spec are one group, another spec another; two LUT_ENC nodes of one theta one group, theta = 2 another; an MV group
    rows = [[TREE, 0, 1, -1, 0, 0], [TREE, 1, 0, -1, 0, 2], [TREE, 0, 0, 1, 1, 1], [LUT_ENC, 0, -1, -1, 0, 0], [LUT_ENC, 1, -1, -1, 0, 1],
            [LUT_ENC, 1, -1, -1, 1, 0], OUT(7), [MV, 0, -1, -1, 0, 1], OUT(9), OUT(9), [TREE_MV, 0, 1, -1, 1, 0], OUT(12)]
    rc, msg = _call(L, rows, stats=st)
    assert rc == -1 and "null ctx" in msg, msg
    # launches: TREE 2 + 2, LUT_ENC 1 + 1, MV 1, TREE_MV 2; rotations: 3 x 3, 3, 1, 3; widest group 2
    assert st.tolist() == [1, 9, 16, 2]
    # a plan without tree rows needs none of the tree families; without MV rows none of the multi-value ones
    rc, msg = _call(L, [[NAND, 0, 1, -1, -1, -1], [LUT, 2, -1, -1, 0, 0]], enc=(False, False), n_enc=0, trees=[], tv1=False, n_rows=0, mvs=[], tv0=False,
                    n_bases=0, fac=False, n_words=0, bias=False, stats=st)
    assert rc == -1 and "null ctx" in msg and st.tolist() == [2, 2, 2, 1], msg
    rc, msg = _call(L, [[LUT_ENC, 0, -1, -1, 0, 0]], tv=False, n_luts=0, trees=[], tv1=False, n_rows=0, mvs=[], tv0=False, n_bases=0, fac=False, n_words=0, stats=st)
    assert rc == -1 and "null ctx" in msg and st.tolist() == [1, 1, 1, 1], msg


SELECT_MSG = "SELECT node: not run on the 3-gen engine"
BAD_PLANS = [
    ("SELECT", [[SELECT, 0, -1, -1, 0, 0]], {}, SELECT_MSG),
    ("SELECT after valid rows", CHAIN + [[SELECT, 8, -1, -1, 0, 2]], {}, SELECT_MSG),
    ("SELECT before a bad row", [[SELECT, 0, -1, -1, 0, 0], [TREE, 0, 1, -1, 9, 0]], {}, "D = P n packing key"),
    ("LUT_OUT missing after TREE_MV", [[TREE_MV, 0, 1, -1, 1, 0], [NAND, 0, 1, -1, -1, -1]], {}, "missing LUT_OUT"),
    ("LUT_OUT missing at the end", [[TREE_MV, 0, 1, -1, 1, 0]], {}, "missing LUT_OUT"),
    ("LUT_OUT extra after TREE_MV", [[TREE_MV, 0, 1, -1, 1, 0], OUT(2), OUT(2)], {}, "LUT_OUT row without"),
    ("LUT_OUT after TREE", [[TREE, 0, 1, -1, 0, 0], OUT(2)], {}, "LUT_OUT row without"),
    ("LUT_OUT missing after LUT_ENC theta 2", [[LUT_ENC, 0, -1, -1, 1, 0]], {}, "missing LUT_OUT"),
    ("LUT_OUT extra after LUT_ENC", [[LUT_ENC, 0, -1, -1, 0, 0], OUT(2)], {}, "LUT_OUT row without"),
    ("LUT_OUT wrong head", [[TREE_MV, 0, 1, -1, 1, 0], OUT(3)], {}, "wrong head"),
    ("etab", [[LUT_ENC, 0, -1, -1, 0, 2]], {}, "etab out of range"),
    ("etab", [[LUT_ENC, 0, -1, -1, 0, -1]], {}, "etab out of range"),
    ("LUT_ENC spec", [[LUT_ENC, 0, -1, -1, 2, 0]], {}, "spec index out of range"),
    ("LUT_ENC operands", [[LUT_ENC, 0, 1, -1, 0, 0]], {}, "operands do not match"),
    ("LUT_ENC without tables", [[LUT_ENC, 0, -1, -1, 0, 0]], dict(enc=(False, False), n_enc=0), "null table family"),
    ("LUT_ENC without specs", [[LUT_ENC, 0, -1, -1, 0, 0]], dict(specs=[], tv=False, n_luts=0), "null table family"),
    ("enc masks without bodies", [[NAND, 0, 1, -1, -1, -1]], dict(enc=(True, False)), "count but no pointer"),
    ("n_enc", [[NAND, 0, 1, -1, -1, -1]], dict(n_enc=(1 << 18) + 1), "n_enc"),
    ("tree index", [[TREE, 0, 1, -1, 2, 0]], {}, "tree index out of range"),
    ("tree index", [[TREE, 0, 1, -1, -1, 0]], {}, "tree index out of range"),
    ("row0", [[TREE, 0, 1, -1, 0, 3]], {}, "row0 + R out of range"),
    ("row0", [[TREE, 0, 1, -1, 0, -1]], {}, "row0 + R out of range"),
    ("TREE operands", [[TREE, 0, -1, -1, 0, 0]], {}, "operands do not match"),
    ("TREE operands", [[TREE, 0, 1, -1, 1, 0]], {}, "operands do not match"),
    ("TREE operand order", [[TREE, 0, 2, -1, 0, 0]], {}, "not an earlier wire"),
    ("TREE without specs", [[TREE, 0, 1, -1, 0, 0]], dict(trees=[]), "null table family"),
    ("TREE without rows", [[TREE, 0, 1, -1, 0, 0]], dict(tv1=False, n_rows=0), "null table family"),
    ("rows without pointer", [[NAND, 0, 1, -1, -1, -1]], dict(tv1=False), "count but no pointer"),
    ("n_trees", [[NAND, 0, 1, -1, -1, -1]], dict(n_trees=1025), "n_trees"),
    ("n_trees", [[NAND, 0, 1, -1, -1, -1]], dict(n_trees=0), "n_trees"),
    ("n_tv1_rows", [[NAND, 0, 1, -1, -1, -1]], dict(n_rows=(1 << 18) + 1), "n_tv1_rows"),
    ("tree p_hi", [[NAND, 0, 1, -1, -1, -1]], dict(trees=[(ONE, ONE, 3)]), "p_hi must be a power of two"),
    ("tree p_hi", [[NAND, 0, 1, -1, -1, -1]], dict(trees=[(ONE, ONE, 1)]), "p_hi must be a power of two"),
    ("tree p_hi past one packing", [[TREE, 0, 1, -1, 0, 0]], dict(trees=[(ONE, ONE, 128)], n_rows=128), "p_hi must be a power of two in 2 .. 64"),
    ("tree hi theta", [[NAND, 0, 1, -1, -1, -1]], dict(trees=[(ONE, ONE2, 4)]), "spec_hi theta must be 1"),
    ("tree hi n_inputs", [[NAND, 0, 1, -1, -1, -1]], dict(trees=[(ONE, (4, (1, 0, 0), 0, 1), 4)]), "n_inputs"),
    ("tree lo theta", [[TREE, 0, 1, -1, 0, 0]], dict(trees=[((1, (1, 0, 0), 0, 4), ONE, 2)]), "theta must divide p_hi"),
    ("tree lo theta", [[TREE, 0, 1, -1, 0, 0]], dict(trees=[((1, (1, 0, 0), 0, 3), ONE, 4)]), "theta"),
    ("tree lo + hi operands", [[TREE, 0, 1, 1, 0, 0]], dict(trees=[(TWO, TWO, 4)]), "exceed three"),
    ("mv index", [[TREE_MV, 0, 1, -1, 2, 0], OUT(2)], {}, "mv index out of range"),
    ("TREE_MV table", [[TREE_MV, 0, 1, -1, 1, 1], OUT(2)], {}, "table index out of range"),
    ("TREE_MV operands", [[TREE_MV, 0, -1, -1, 1, 0], OUT(2)], {}, "operands do not match"),
    ("TREE_MV k p_hi", [[TREE_MV, 0, 1, -1, 1, 0]], dict(mvs=[MVS[0], (ONE, ONE, 4, 16, 5, 1, 24, 1)], n_words=4096), "k p_hi must be at most 64"),
    ("TREE_MV k", [[TREE_MV, 0, 1, -1, 1, 0]], dict(mvs=[MVS[0], (ONE, ONE, 4, 4, 0, 1, 24, 1)]), "k must be at least 1"),
    ("TREE_MV p_hi", [[TREE_MV, 0, 1, -1, 1, 0]], dict(mvs=[MVS[0], (ONE, ONE, 4, 3, 1, 1, 24, 1)]), "p_hi must be a power of two"),
    ("TREE_MV p_lo", [[TREE_MV, 0, 1, -1, 1, 0]], dict(mvs=[MVS[0], (ONE, ONE, 6, 4, 2, 1, 24, 1)], n_words=4096), "p must be a power of two"),
    ("TREE_MV lo theta", [[TREE_MV, 0, 1, -1, 1, 0]], dict(mvs=[MVS[0], (ONE2, ONE, 4, 4, 2, 1, 24, 1)]), "theta must be 1"),
    ("TREE_MV hi theta", [[TREE_MV, 0, 1, -1, 1, 0]], dict(mvs=[MVS[0], (ONE, ONE2, 4, 4, 2, 1, 24, 1)]), "spec_hi theta must be 1"),
    ("TREE_MV factors", [[TREE_MV, 0, 1, -1, 1, 0], OUT(2)], dict(n_words=55), "factors_off"),
    ("TREE_MV base", [[TREE_MV, 0, 1, -1, 1, 0], OUT(2)], dict(n_bases=1), "base out of range"),
    ("TREE_MV n_tables", [[TREE_MV, 0, 1, -1, 1, 0]], dict(mvs=[MVS[0], (ONE, ONE, 4, 4, 2, 1, 24, 0)]), "n_tables"),
    ("an MV row on a k = 2 spec", [[MV, 0, -1, -1, 1, 0]], {}, "k must be 1"),
    ("null mvs", [[TREE_MV, 0, 1, -1, 1, 0], OUT(2)], dict(mvs=[]), "null table family"),
    ("earlier checks stay", [[LUT, 0, -1, -1, 2, 0]], {}, "spec index out of range"),
    ("earlier checks stay", [[NAND, 0, 1, -1, 0, -1]], {}, "spec and lut must be -1"),
    ("earlier checks stay", [[21, 0, 1, -1, -1, -1]], {}, "opcode not defined"),
    ("earlier checks stay", [[8, 0, 1, -1, -1, -1]], {}, "opcode not defined"),      # a single-key gate the 3-gen scheme has not
]


@pytest.mark.parametrize("what, rows, kw, needle", BAD_PLANS, ids=[f"{i}-{b[0]}" for i, b in enumerate(BAD_PLANS)])
def test_bad_plans_are_refused_before_the_context(what, rows, kw, needle):
    import thfhe
    st = np.full(4, -1, np.int64)
    rc, msg = _call(thfhe.lib(), rows, stats=st, **kw)
    assert rc == -1 and needle in msg and "null ctx" not in msg, (what, msg)
    assert st.tolist() == [-1] * 4          # no figures of a refused plan


def test_the_older_entries_still_refuse_the_opcodes():
    import thfhe
    L = thfhe.lib()
    for row in ([TREE_MV, 0, 1, -1, 1, 0], [TREE, 0, 1, -1, 0, 0], [LUT_ENC, 0, -1, -1, 0, 0], [SELECT, 0, -1, -1, 0, 0]):
        for entry in ("thfhe_mk_dag_run_mv_batch", "thfhe_mk_dag_run_lut_batch"):
            rc, msg = _call(L, [row], mvs=[MVS[0]], n_words=24, entry=entry)
            assert rc == -1 and "opcode not defined" in msg, (row, entry, msg)
    # ... and run what they ran
    rc, msg = _call(L, [[MV, 0, -1, -1, 0, 1], OUT(2), OUT(2)], mvs=[MVS[0]], n_words=24, entry="thfhe_mk_dag_run_mv_batch")
    assert rc == -1 and "null ctx" in msg


def test_circuit_helpers_keep_torus64_tables():
    from thfhe import circuits as CIR
    from thfhe import lut
    cir = CIR.Circuit()
    a, b = cir.inputs(2)
    rows = lut.tree_test_vectors(lambda h, l: (h + l) & 1, 4, 4, 2, theta=2, N=2048, torus_bits=64)
    r0 = cir.tree_rows(rows)
    assert r0 == 0 and cir.tree_rows(rows) == 0 and len(cir.tv1) == 2 and cir.tv1[0].dtype == np.int64 and cir.tv1[0].shape == (2048,)
    t = cir.tree(r0, [a], [b], 4, theta1=2)
    tv0, w, ob = lut.tree_mvk_bool_factors([lambda h, l: int(l > h), lambda h, l: (h ^ l) & 1], 4, 4, N=2048, torus_bits=64)
    base = cir.mv_base(tv0)
    outs = cir.tree_mv(base, w, [t], [a], out_bias=ob)
    assert outs == [3, 4] and cir.mv_out_bias == {0: ob} and cir.mv_bases[base].dtype == np.int64
    ea, eb = np.arange(2048, dtype=np.int64), np.arange(2048, dtype=np.int64) << 40
    e = cir.enc_table(ea, eb)
    assert cir.enc_tables[e][0].dtype == np.int64 and np.array_equal(cir.enc_tables[e][1], eb) and cir.enc_table(ea, eb) == e
    z = cir.lut_enc(e, [outs[0]])
    assert z == [5]
    n = cir.nodes()
    assert n[0].tolist() == [TREE, 0, 1, -1, 0, 0] and n[1].tolist() == [TREE_MV, 2, 0, -1, 0, 0] and n[3].tolist() == [LUT_ENC, 3, -1, -1, 0, 0]
    # int32 inputs stay int32 (the single-key engine)
    c32 = CIR.Circuit()
    c32.inputs(1)
    assert c32.tv1 == [] and c32.tree_rows(lut.tree_test_vectors(lambda h, l: h ^ l, 2, 2, 2)) == 0 and c32.tv1[0].dtype == np.int32
    assert c32.enc_tables == [] and c32.enc_table(np.zeros(1024, np.int32), np.ones(1024, np.int32)) == 0 and c32.enc_tables[0][1].dtype == np.int32
    # the digit circuits build on the 3-gen engine's ring and torus
    c64 = CIR.Circuit()
    x, y = c64.inputs(2)
    lo, hi = CIR.tree_mul_digits(c64, x, y, N=2048, torus_bits=64)
    bits = CIR.sbox_digits(c64, x, y, list(range(16)) * 4, N=2048, torus_bits=64)
    assert c64.tv1[0].dtype == np.int64 and c64.tv1[0].shape == (2048,) and c64.mv_bases[0].dtype == np.int64 and len(bits) == 4 and hi == lo + 1


def test_evaluate_refuses_select_and_leveled_rows_on_a_multi_key_context():
    import thfhe
    from thfhe import circuits as CIR
    ck = thfhe.MKCloudKey.__new__(thfhe.MKCloudKey)
    ck.params, ck.words, ck.h = thfhe.make_params("MK2"), 1041, None
    cir = CIR.Circuit()
    ins = cir.inputs(5)
    cir.select([ins[0]], 1, 4)
    with pytest.raises(ValueError, match="SELECT"):
        CIR.evaluate(ck, cir, np.zeros((5, 1041), np.int32))
    # a tree circuit goes to the new entry: without a context its host checks pass and the library answers
    cir = CIR.Circuit()
    a, b = cir.inputs(2)
    from thfhe import lut
    cir.tree(cir.tree_rows(lut.tree_test_vectors(lambda h, l: h ^ l, 2, 2, 2, N=1024, torus_bits=64)), [a], [b], 2)
    with pytest.raises(thfhe.ThfheError, match="null ctx"):
        CIR.evaluate(ck, cir, np.zeros((2, 1041), np.int32))
