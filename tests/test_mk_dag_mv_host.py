"""Multi-value nodes in the 3-gen gate-DAG executor, host side (no GPU): the plan's figures for circuits with MV, LUT and
gate rows, every host check of thfhe_mk_dag_run_mv_batch (they run before the context is looked at), the node kinds it refuses, the older entries
still refusing the opcode, and Circuit.mv on Torus64 base vectors."""
import ctypes as C

import numpy as np
import pytest

I32, I64 = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
N = 1024
NAND, MUX, NOT, LUT, LUT_OUT, LUT_ENC, SELECT, TREE, MV, TREE_MV = 0, 9, 11, 14, 15, 16, 17, 18, 19, 20
ONE = (1, (1, 0, 0), 0, 1)
TWO = (2, (1, 2, 0), 0, 1)
# (lo, hi, p, q, k, base, factors_off, n_tables): q = 3 outputs of p = 4 with two tables; q = 1 of p = 2 on the second base
MVS = [(ONE, ONE, 4, 3, 1, 0, 0, 2), (TWO, ONE, 2, 1, 1, 1, 24, 1)]
N_WORDS = 24 + 2
OUT = lambda h: [LUT_OUT, h, -1, -1, -1, -1]


def _call(L, nodes, n_inputs=2, mvs=MVS, n_mvs=None, tv0=True, n_bases=2, fac=True, n_words=N_WORDS, specs=True, bias=True, stats=None,
          entry="thfhe_mk_dag_run_mv_batch"):
    import thfhe
    mv = (thfhe.MvSpec * max(len(mvs), 1))(*[thfhe.MvSpec(thfhe._lut_spec(m[0]), thfhe._lut_spec(m[1]), *m[2:]) for m in mvs])
    sp = (thfhe.LutSpec * 1)(thfhe._lut_spec(ONE))
    nodes = np.ascontiguousarray(nodes, np.int32)
    x = np.zeros((1, n_inputs, 1041), np.int32)
    out = np.zeros((1, max(nodes.shape[0], 1), 1041), np.int32)
    tab = np.zeros((4, N), np.int64)
    words = np.zeros(4096, np.int32)
    ob = np.zeros(max(len(mvs), 1), np.int64)
    ptab = tab.ctypes.data_as(I64)
    common = (1, None, 0, out.ctypes.data_as(I32), None if stats is None else stats.ctypes.data_as(I64))
    head = (x.ctypes.data_as(I32), n_inputs, nodes.ctypes.data_as(I32), nodes.shape[0])
    luts = (sp, 1, ptab, 2) if specs else (None, 0, None, 0)
    if entry == "thfhe_mk_dag_run_mv_batch":
        rc = L.thfhe_mk_dag_run_mv_batch(None, *head, *luts, mv if mvs else None, len(mvs) if n_mvs is None else n_mvs, ptab if tv0 else None, n_bases,
                                         words.ctypes.data_as(I32) if fac else None, n_words, ob.ctypes.data_as(I64) if bias else None, *common)
    elif entry == "thfhe_mk_dag_run_lut_batch":
        rc = L.thfhe_mk_dag_run_lut_batch(None, *head, *luts, *common)
    else:
        raise ValueError(entry)
    return rc, L.thfhe_last_error().decode()


# wires: 2..4 MV (spec 0, table 1), 5 NAND of two of them, 6 LUT on the third, 7 MV (spec 1) on two inputs, 8 NOT, 9..11 MV (spec 0) on the LUT's wire
OK_ROWS = [[MV, 0, -1, -1, 0, 1], OUT(2), OUT(2), [NAND, 2, 3, -1, -1, -1], [LUT, 4, -1, -1, 0, 1], [MV, 0, 1, -1, 1, 0], [NOT, 5, -1, -1, -1, -1],
           [MV, 6, -1, -1, 0, 0], OUT(9), OUT(9)]


def test_symbols_and_signatures():
    import thfhe
    for name in ("thfhe_mk_mv_lut_bootstrap", "thfhe_mk_mv_lut_bootstrap_wo_keyswitch", "thfhe_mk_set_mv_slice", "thfhe_mk_dag_run_mv_batch"):
        assert name in thfhe.SIGNATURES and hasattr(thfhe.lib(), name), name
    assert len(thfhe.SIGNATURES["thfhe_mk_dag_run_mv_batch"][1]) == len(thfhe.SIGNATURES["thfhe_mk_dag_run_lut_batch"][1]) + 7
    assert len(thfhe.SIGNATURES["thfhe_mk_mv_lut_bootstrap"][1]) == len(thfhe.SIGNATURES["thfhe_mv_lut_bootstrap"][1]) + 1   # out_bias


def test_a_valid_plan_reaches_the_context_and_counts():
    import thfhe
    L = thfhe.lib()
    st = np.full(4, -1, np.int64)
    rc, msg = _call(L, OK_ROWS, stats=st)
    assert rc == -1 and "null ctx" in msg, msg
    # level 1: MV spec 0, MV spec 1 (one group per spec); level 2: the gate, the LUT; level 3: MV spec 0 again.  One rotation per MV node.
    assert st.tolist() == [3, 5, 5, 1]
    # two MV nodes of one spec on one level are one launch group of two, whatever their tables
    rows = [[MV, 0, -1, -1, 0, 0], OUT(2), OUT(2), [MV, 1, -1, -1, 0, 1], OUT(5), OUT(5)]
    rc, msg = _call(L, rows, stats=st)
    assert rc == -1 and "null ctx" in msg and st.tolist() == [1, 1, 2, 2]
    # no LUT row: specs and tv may be absent; no out_bias array: 0 for every spec
    rc, msg = _call(L, rows, specs=False, bias=False, stats=st)
    assert rc == -1 and "null ctx" in msg and st.tolist() == [1, 1, 2, 2]
    # the multi-value families absent: the call is thfhe_mk_dag_run_lut_batch, which gives its figures to a caller with a context only
    rows = [[NAND, 0, 1, -1, -1, -1], [LUT, 2, -1, -1, 0, 0]]
    for entry in ("thfhe_mk_dag_run_mv_batch", "thfhe_mk_dag_run_lut_batch"):
        st[:] = -1
        rc, msg = _call(L, rows, mvs=[], tv0=False, n_bases=0, fac=False, n_words=0, stats=st, entry=entry)
        assert rc == -1 and "null ctx" in msg and st.tolist() == [-1] * 4, (entry, msg)
    rc, msg = _call(L, rows, mvs=[], tv0=False, n_bases=0, fac=False, n_words=0, specs=False)
    assert rc == -1 and "null argument" in msg   # ... and requires specs and tv


BAD_PLANS = [
    ("mv index", [[MV, 0, -1, -1, 2, 0], OUT(2), OUT(2)], {}, "mv index out of range"),
    ("mv index", [[MV, 0, -1, -1, -1, 0], OUT(2), OUT(2)], {}, "mv index out of range"),
    ("t", [[MV, 0, -1, -1, 0, 2], OUT(2), OUT(2)], {}, "table index out of range"),
    ("t", [[MV, 0, 1, -1, 1, -1]], {}, "table index out of range"),
    ("base", [[MV, 0, 1, -1, 1, 0]], dict(n_bases=1), "base out of range"),
    ("factors", [[MV, 0, 1, -1, 1, 0]], dict(n_words=25), "factors_off"),
    ("factors", [[MV, 0, 1, -1, 1, 0]], dict(mvs=[MVS[0], (TWO, ONE, 2, 1, 1, 1, -2, 1)]), "factors_off"),
    ("spec theta", [[MV, 0, 1, -1, 1, 0]], dict(mvs=[MVS[0], ((2, (1, 2, 0), 0, 2), ONE, 2, 1, 1, 1, 24, 1)]), "theta must be 1"),
    ("spec p", [[MV, 0, 1, -1, 1, 0]], dict(mvs=[MVS[0], (TWO, ONE, 3, 1, 1, 1, 24, 1)]), "p must be"),
    ("spec p", [[MV, 0, 1, -1, 1, 0]], dict(mvs=[MVS[0], (TWO, ONE, 128, 1, 1, 1, 24, 1)], n_words=4096), "p must be"),
    ("spec q", [[MV, 0, 1, -1, 1, 0]], dict(mvs=[MVS[0], (TWO, ONE, 2, 65, 1, 1, 24, 1)], n_words=4096), "q must be"),
    ("spec q", [[MV, 0, 1, -1, 1, 0]], dict(mvs=[MVS[0], (TWO, ONE, 2, 0, 1, 1, 24, 1)]), "q must be"),
    ("spec n_tables", [[MV, 0, 1, -1, 1, 0]], dict(mvs=[MVS[0], (TWO, ONE, 2, 1, 1, 1, 24, 0)]), "n_tables"),
    ("spec k", [[MV, 0, 1, -1, 1, 0]], dict(mvs=[MVS[0], (TWO, ONE, 2, 1, 2, 1, 24, 1)]), "k must be 1"),
    ("spec n_inputs", [[MV, 0, 1, -1, 1, 0]], dict(mvs=[MVS[0], ((4, (1, 2, 0), 0, 1), ONE, 2, 1, 1, 1, 24, 1)]), "n_inputs"),
    ("LUT_OUT missing", [[MV, 0, -1, -1, 0, 0], OUT(2), [NAND, 0, 1, -1, -1, -1]], {}, "missing LUT_OUT"),
    ("LUT_OUT missing at the end", [[MV, 0, -1, -1, 0, 0], OUT(2)], {}, "missing LUT_OUT"),
    ("LUT_OUT extra", [[MV, 0, -1, -1, 0, 0], OUT(2), OUT(2), OUT(2)], {}, "LUT_OUT row without"),
    ("LUT_OUT extra after q = 1", [[MV, 0, 1, -1, 1, 0], OUT(2)], {}, "LUT_OUT row without"),
    ("LUT_OUT wrong head", [[MV, 0, -1, -1, 0, 0], OUT(2), OUT(3)], {}, "wrong head"),
    ("operands", [[MV, 0, 1, -1, 0, 0], OUT(2), OUT(2)], {}, "operands do not match"),
    ("operands", [[MV, 0, -1, -1, 1, 0]], {}, "operands do not match"),
    ("operand order", [[MV, 2, -1, -1, 0, 0], OUT(2), OUT(2)], {}, "not an earlier wire"),
    ("null mvs", [[MV, 0, -1, -1, 0, 0], OUT(2), OUT(2)], dict(mvs=[]), "null table family"),
    ("null bases", [[MV, 0, -1, -1, 0, 0], OUT(2), OUT(2)], dict(tv0=False, n_bases=0), "null table family"),
    ("null factors", [[MV, 0, -1, -1, 0, 0], OUT(2), OUT(2)], dict(fac=False, n_words=0), "null table family"),
    ("LUT without tables", [[LUT, 0, -1, -1, 0, 0]], dict(specs=False), "null table family"),
    ("count without pointer", [[NAND, 0, 1, -1, -1, -1]], dict(tv0=False), "count but no pointer"),
    ("count without pointer", [[NAND, 0, 1, -1, -1, -1]], dict(fac=False), "count but no pointer"),
    ("n_mvs", [[NAND, 0, 1, -1, -1, -1]], dict(n_mvs=1025), "n_mvs"),
    ("n_mvs", [[NAND, 0, 1, -1, -1, -1]], dict(n_mvs=0), "n_mvs"),
    ("n_bases", [[NAND, 0, 1, -1, -1, -1]], dict(n_bases=1025), "n_bases"),
    ("n_factor_words", [[NAND, 0, 1, -1, -1, -1]], dict(n_words=(1 << 28) + 1), "n_factor_words"),
    # no multi-key packing: the tree kinds and the encrypted tables are opcodes this engine does not define
    ("TREE_MV", [[TREE_MV, 0, 1, -1, 0, 0]], {}, "opcode not defined"),
    ("SELECT", [[SELECT, 0, -1, -1, 0, 0]], {}, "opcode not defined"),
    ("TREE", [[TREE, 0, 1, -1, 0, 0]], {}, "opcode not defined"),
    ("LUT_ENC", [[LUT_ENC, 0, -1, -1, 0, 0]], {}, "opcode not defined"),
    ("earlier checks stay", [[LUT, 0, -1, -1, 1, 0]], {}, "spec index out of range"),
    ("earlier checks stay", [[NAND, 0, 1, -1, 0, -1]], {}, "spec and lut must be -1"),
    ("earlier checks stay", [[21, 0, 1, -1, -1, -1]], {}, "opcode not defined"),
]


@pytest.mark.parametrize("what, rows, kw, needle", BAD_PLANS, ids=[f"{i}-{b[0]}" for i, b in enumerate(BAD_PLANS)])
def test_bad_plans_are_refused_before_the_context(what, rows, kw, needle):
    import thfhe
    rc, msg = _call(thfhe.lib(), rows, **kw)
    assert rc == -1 and needle in msg and "null ctx" not in msg, (what, msg)


def test_the_older_entries_still_refuse_the_opcode():
    import thfhe
    L = thfhe.lib()
    rc, msg = _call(L, [[MV, 0, -1, -1, 0, 0], OUT(2), OUT(2)], entry="thfhe_mk_dag_run_lut_batch")
    assert rc == -1 and "opcode not defined" in msg
    # the single-key multi-value entry keeps its own checks: a TREE_MV row is still a row of its, and refused for its spec, not its opcode
    import test_dag_mv_host as SK
    rc, msg = SK._call(L, [[TREE_MV, 0, 1, 2, 0, 0]])
    assert rc == -1 and "p_hi must be" in msg
    rc, msg = SK._call(L, [[MV, 0, 1, -1, 0, 1], SK.OUT(4), SK.OUT(4)])
    assert rc == -1 and "null ctx" in msg


def test_circuit_mv_keeps_torus64_bases_and_out_bias():
    from thfhe import circuits as CIR
    from thfhe import lut
    tabs = [[int(m >= t) for m in range(4)] for t in (1, 2, 3)]
    tv0, c, ob = lut.mv_bool_factors(tabs, 4, 64, 1024)
    cir = CIR.Circuit()
    a, b = cir.inputs(2)
    base = cir.mv_base(tv0)
    assert cir.mv_bases[base].dtype == np.int64 and np.all(cir.mv_bases[base] == 1 << 61)
    w = cir.mv(base, c, [a], out_bias=ob)
    w2 = cir.mv(base, c, [b], out_bias=ob)        # the same spec: one launch group
    w3 = cir.mv(base, c, [b])                     # another out_bias is another spec
    assert w == [2, 3, 4] and w2 == [5, 6, 7] and w3 == [8, 9, 10]
    assert cir.mv_out_bias == {0: ob} and len(cir.mv_specs) == 2
    mvs, bases, words = cir.mv_families()
    assert bases.dtype == np.int64 and bases.shape == (1, 1024) and [m[2:] for m in mvs] == [(4, 3, 1, 0, 0, 1), (4, 3, 1, 0, 12, 1)]
    assert cir.nodes()[0].tolist() == [MV, 0, -1, -1, 0, 0] and cir.nodes()[6].tolist() == [MV, 1, -1, -1, 1, 0]
    # an int32 base stays int32 (the single-key engine)
    assert CIR.Circuit().mv_bases == [] and cir.mv_base(lut.mv_base(1 << 30)) == 1 and cir.mv_bases[1].dtype == np.int32
