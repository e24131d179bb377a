"""Leveled nodes in the gate-DAG executor, host side (no GPU): the opcodes, the exported entry and the Julia binding's arity;
every host check of thfhe_dag_run_lhe_batch, made with NULL contexts and NULL sets, which proves it runs before either is looked at; the earlier
six-column entries refusing the three opcodes (the four-column ones need a live context: tests/test_gpu_dag_lhe_shapes.py); Circuit.lhe_lookup / lhe_gather / lhe_wfa rows, levels() and census(); simulate of lhe_array_read over all
16 addresses and of wfa_mux_max over all 256 pairs; the CPU yardstick (tests/dag_lhe_reference.py) against simulate on noiseless samples; and the
noise of a gathered wire on SK-128 in the model."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import dag_lhe_reference as DL
import lhe_reference as LR

I32, I64 = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
N = 1024
NAND, XOR, MUX, NOT, COPY, LUT_OUT, LOOKUP, GATHER, WFA = 0, 3, 10, 11, 12, 15, 21, 22, 23
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (set, d_tree, d_rot, theta): a lookup spec with theta = 2, a gather spec at d = 2 + 1, a lookup-only spec (d_rot = 0)
LKS = [(0, 1, 2, 2), (1, 1, 2, 1), (0, 2, 0, 1)]
# (n_steps, n_states, theta, n_out, set0, n_sets, trans_off, step_off, start_off): 2 steps, 3 states, theta 2, 2 outputs over both sets
WFAS = [(2, 3, 2, 2, 0, 2, 0, 12, 14)]
POOL = [1, 2, 2, 0, 0, 1, 0, 0, 2, 1, 1, 2] + [16 * 1 + 0, 16 * 0 + 1] + [2, 0]


def test_opcodes_exports_and_struct_layout():
    import thfhe
    assert (thfhe.LHE_LOOKUP, thfhe.LHE_GATHER, thfhe.LHE_WFA) == (21, 22, 23)
    assert "thfhe_dag_run_lhe_batch" in thfhe.SIGNATURES and hasattr(thfhe.lib(), "thfhe_dag_run_lhe_batch")
    assert len(thfhe.SIGNATURES["thfhe_dag_run_lhe_batch"][1]) == len(thfhe.SIGNATURES["thfhe_dag_run_mv_batch"][1]) + 1
    assert C.sizeof(thfhe.DagLheSpec) == 16 and C.sizeof(thfhe.DagWfaSpec) == 36
    src = open(os.path.join(ROOT, "torus-fhe_amd", "julia", "TFHE_HIP.jl")).read()
    m = re.search(r"ccall\(\(:thfhe_dag_run_lhe_batch, LIB\), *Cint, *\(([^()]*(?:\{[^()]*\}[^()]*)*)\)", src)
    assert m and len([a for a in m.group(1).split(",") if a.strip()]) == len(thfhe.SIGNATURES["thfhe_dag_run_lhe_batch"][1])


def _call(L, nodes, n_inputs=8, lks=LKS, n_lks=None, wfas=WFAS, n_wfas=None, pool=POOL, n_words=None, sets=2, tab=True, n_tab=6, fin=True, n_fin=4,
          lhe=True, stats=None, entry="thfhe_dag_run_lhe_batch"):
    """the entry with NULL contexts and NULL sets: every answer comes from the host checks"""
    import thfhe
    lk = (thfhe.DagLheSpec * max(len(lks), 1))(*[thfhe.DagLheSpec(*k) for k in lks])
    wf = (thfhe.DagWfaSpec * max(len(wfas), 1))(*[thfhe.DagWfaSpec(*a) for a in wfas])
    hs = (C.c_void_p * max(sets, 1))()
    pool = np.array(pool, np.int32)
    t = np.zeros((8, N), np.int32)
    pt = t.ctypes.data_as(I32)
    fam = thfhe.DagLheFamilies(hs if sets else None, sets, lk if lks else None, len(lks) if n_lks is None else n_lks, None, pt if tab else None, n_tab,
                               wf if wfas else None, len(wfas) if n_wfas is None else n_wfas, pool.ctypes.data_as(I32) if len(pool) else None,
                               len(pool) if n_words is None else n_words, None, pt if fin else None, n_fin)
    sp = (thfhe.LutSpec * 1)(thfhe._lut_spec((1, (1, 0, 0), 0, 1)))
    nodes = np.ascontiguousarray(nodes, np.int32).reshape(-1, 6)
    x = np.zeros((1, n_inputs, 631), np.int32)
    out = np.zeros((1, max(nodes.shape[0], 1), 631), np.int32)
    common = (1, None, 0, out.ctypes.data_as(I32), None if stats is None else stats.ctypes.data_as(I64))
    head = (x.ctypes.data_as(I32), n_inputs, nodes.ctypes.data_as(I32), nodes.shape[0])
    mid = (sp, 1, pt, 2, None, None, 0, None, 0, None, 0)
    if entry == "thfhe_dag_run_lhe_batch":
        rc = L.thfhe_dag_run_lhe_batch(None, None, *head, *mid, None, 0, None, 0, None, 0, C.byref(fam) if lhe else None, *common)
    elif entry == "thfhe_dag_run_mv_batch":
        rc = L.thfhe_dag_run_mv_batch(None, None, *head, *mid, None, 0, None, 0, None, 0, *common)
    elif entry == "thfhe_dag_run_tree_batch":
        rc = L.thfhe_dag_run_tree_batch(None, None, *head, *mid, *common)
    elif entry == "thfhe_dag_run_lut_batch":
        rc = L.thfhe_dag_run_lut_batch(None, *head, sp, 1, pt, 2, *common)
    elif entry == "thfhe_mk_dag_run_lut_batch":
        rc = L.thfhe_mk_dag_run_lut_batch(None, *head, sp, 1, np.zeros((2, N), np.int64).ctypes.data_as(I64), 2, *common)
    else:
        raise ValueError(entry)
    return rc, L.thfhe_last_error().decode()


OUT = lambda h: [LUT_OUT, h, -1, -1, -1, -1]
LK = lambda lk, row0: [LOOKUP, -1, -1, -1, lk, row0]
GA = lambda lk, first: [GATHER, -1, -1, -1, lk, first]
WF = lambda wfa, fin0: [WFA, -1, -1, -1, wfa, fin0]
GOOD = [LK(0, 4), OUT(8), GA(1, 0), WF(0, 1), OUT(11), OUT(11), OUT(11), LK(2, 2), GA(1, 3)]


def test_a_good_plan_passes_the_host_checks_and_stops_at_the_sets():
    import thfhe
    L = thfhe.lib()
    st = np.zeros(4, np.int64)
    rc, msg = _call(L, GOOD, stats=st)
    assert rc == -1 and "null tgsw set" in msg, msg          # the plan is accepted: the first thing missing is a set
    # LOOKUP and WFA nodes and the GATHER over inputs on level 1, the GATHER over wires 3 .. 10 above the first LOOKUP: 2 levels; no rotation;
    # one launch per (kind, spec) group of a level: lk 0, lk 2, gather lk 1, wfa 0 | gather lk 1
    assert st.tolist() == [2, 5, 0, 1]


BAD = [
    ("operand fields", [[LOOKUP, 0, -1, -1, 0, 0]], {}),
    ("operand fields", [[GATHER, -1, -1, 2, 1, 0]], {}),
    ("operand fields", [[WFA, -1, 1, -1, 0, 0], OUT(8), OUT(8), OUT(8)], {}),
    ("lk out of range", [LK(3, 0), OUT(8)], {}),
    ("lk out of range", [GA(-1, 0)], {}),
    ("wfa out of range", [WF(1, 0), OUT(8), OUT(8), OUT(8)], {}),
    ("row0 \\+ 2\\^d_tree out of range", [LK(0, 5), OUT(8)], {}),
    ("row0 \\+ 2\\^d_tree out of range", [LK(2, -1)], {}),
    ("fin_row0 \\+ n_states out of range", [WF(0, 2), OUT(8), OUT(8), OUT(8)], {}),
    ("missing LUT_OUT", [LK(0, 0), LK(2, 0)], {}),
    ("missing LUT_OUT", [WF(0, 0), OUT(8), OUT(8)], {}),
    ("LUT_OUT row without", [LK(2, 0), OUT(8)], {}),
    ("LUT_OUT row without", [GA(1, 0), OUT(8)], {}),
    ("candidate is not an earlier wire", [GA(1, 1)], {}),             # wires 1 .. 8: the node's own wire is the last
    ("candidate is not an earlier wire", [GA(1, -1)], {}),
    ("theta must be 1", [GA(0, 0)], {}),
    ("d_rot must be 1 .. 9", [GA(2, 0)], {}),
    ("d_rot must be 1 .. 9", [GA(0, 0)], dict(lks=[(0, 0, 10, 1)])),
    ("d_tree must be 0 .. 6", [LK(0, 0)], dict(lks=[(0, 7, 0, 1)])),
    ("d_rot must be 0 .. 10", [LK(0, 0)], dict(lks=[(0, 0, 11, 1)])),
    ("theta must be 1, 2 or 4", [LK(0, 0), OUT(8), OUT(8)], dict(lks=[(0, 0, 2, 3)])),
    ("must not exceed box", [LK(0, 0), OUT(8), OUT(8), OUT(8)], dict(lks=[(0, 0, 9, 4)])),
    ("set is out of range", [LK(0, 0)], dict(lks=[(2, 0, 1, 1)])),
    ("n_states must be", [WF(0, 0)], dict(wfas=[(2, 65, 1, 1, 0, 2, 0, 12, 14)])),
    ("n_steps must be", [WF(0, 0)], dict(wfas=[(0, 3, 1, 1, 0, 2, 0, 12, 14)])),
    ("n_out must be", [WF(0, 0)], dict(wfas=[(2, 3, 1, 0, 0, 2, 0, 12, 14)])),
    ("theta must be 1, 2 or 4", [WF(0, 0)], dict(wfas=[(2, 3, 3, 1, 0, 2, 0, 12, 14)])),
    ("set0 \\+ n_sets out of range", [WF(0, 0), OUT(8), OUT(8), OUT(8)], dict(wfas=[(2, 3, 2, 2, 1, 2, 0, 12, 14)])),
    ("pool offset", [WF(0, 0), OUT(8), OUT(8), OUT(8)], dict(wfas=[(2, 3, 2, 2, 0, 2, 5, 12, 14)])),
    ("pool offset", [WF(0, 0), OUT(8), OUT(8), OUT(8)], dict(wfas=[(2, 3, 2, 2, 0, 2, 0, 12, 15)])),
    ("pool offset", [WF(0, 0), OUT(8), OUT(8), OUT(8)], dict(n_words=15)),
    ("trans entry out of range", [WF(0, 0), OUT(8), OUT(8), OUT(8)], dict(pool=[3] + POOL[1:])),
    ("start entry out of range", [WF(0, 0), OUT(8), OUT(8), OUT(8)], dict(pool=POOL[:-1] + [3])),
    ("null family", [LK(0, 0), OUT(8)], dict(lks=[])),
    ("null family", [LK(0, 0), OUT(8)], dict(tab=False, n_tab=0)),
    ("null family", [LK(0, 0), OUT(8)], dict(sets=0)),
    ("null family", [WF(0, 0), OUT(8), OUT(8), OUT(8)], dict(wfas=[])),
    ("null family", [WF(0, 0), OUT(8), OUT(8), OUT(8)], dict(fin=False, n_fin=0)),
    ("null family", [WF(0, 0), OUT(8), OUT(8), OUT(8)], dict(pool=[], n_words=0)),
    ("with a count but no pointer", [LK(0, 0), OUT(8)], dict(tab=False)),
    ("with a count but no pointer", [LK(0, 0), OUT(8)], dict(lks=[], n_lks=2)),
    ("n_sets must be", [LK(0, 0), OUT(8)], dict(sets=65)),
    ("n_lks must be", [LK(0, 0), OUT(8)], dict(n_lks=1025)),
    ("not defined for this engine", [LK(0, 0), OUT(8)], dict(lhe=False)),                 # without the families the call is thfhe_dag_run_mv_batch
    ("not an earlier wire", [[NAND, 0, 9, -1, -1, -1]], {}),                              # ... and its own checks stay
]


@pytest.mark.parametrize("case", range(len(BAD)))
def test_every_host_check_runs_before_a_context_or_a_set_is_looked_at(case):
    import thfhe
    match, nodes, kw = BAD[case]
    rc, msg = _call(thfhe.lib(), nodes, **kw)
    assert rc == -1 and re.search(match, msg), (BAD[case], msg)


@pytest.mark.parametrize("entry", ["thfhe_dag_run_mv_batch", "thfhe_dag_run_tree_batch", "thfhe_dag_run_lut_batch", "thfhe_mk_dag_run_lut_batch"])
def test_the_earlier_entries_reject_the_three_opcodes(entry):
    import thfhe
    for nodes in ([LK(2, 0)], [GA(1, 0)], [WF(0, 0), OUT(8), OUT(8), OUT(8)]):
        rc, msg = _call(thfhe.lib(), nodes, entry=entry)
        assert rc == -1 and "not defined for this engine" in msg, (entry, nodes, msg)


def _gate_words(bits):
    return np.where(np.asarray(bits) > 0, 1 << 29, -(1 << 29)).astype(np.int32)


def test_circuit_rows_levels_and_census():
    from thfhe import circuits as CI
    cir = CI.Circuit()
    x = cir.inputs(8)
    g = [cir.gate(NAND, x[i], x[i + 1]) for i in range(4)]
    row0 = cir.lhe_table(np.zeros((4, N), np.int32))
    lk = cir.lhe_lookup(0, row0 + 2, 1, 2, theta=2)
    ga = cir.lhe_gather(1, g[0], 0, 2)
    aut = CI.wfa_less_than(2)
    w = cir.lhe_wfa(aut, [2, 3], cir.lhe_finals(np.zeros((4, N), np.int32)))
    top = cir.gate(MUX, w[0], ga, lk[1])
    assert cir.has_lhe_nodes() and not cir.has_luts() and cir.n_lhe_sets() == 4
    nodes = cir.nodes()
    assert nodes[4].tolist() == [LOOKUP, -1, -1, -1, 0, 2] and nodes[5].tolist() == [LUT_OUT, lk[0], -1, -1, -1, -1]
    assert nodes[6].tolist() == [GATHER, -1, -1, -1, 1, g[0]] and nodes[7].tolist() == [WFA, -1, -1, -1, 0, 0]
    assert cir.lhe_specs == [(0, 1, 2, 2), (1, 0, 2, 1)]
    assert cir.levels() == [[0, 1, 2, 3, 4, 5, 7], [6], [8]]        # LOOKUP and WFA on the first level, the GATHER above its candidates
    assert cir.census() == dict(gates=9, bootstrapped=5, mux=1, rotations=6, depth=3, lhe_lookups=1, lhe_gathers=1, lhe_wfas=1)
    fam = cir.lhe_families()
    assert fam["wfas"] == [(4, 4, 1, 1, 2, 2, 0, 32, 36)] and fam["wfa_words"].shape == (37,) and fam["tab_a"] is None
    with pytest.raises(ValueError):
        cir.lhe_gather(0, top, 0, 1)          # candidates past the last wire
    with pytest.raises(ValueError):
        cir.lhe_gather(0, 0, 1, 0)            # d_rot = 0
    with pytest.raises(ValueError):
        cir.lhe_wfa(aut, [0, 2], 0)           # sets that are not consecutive
    with pytest.raises(ValueError):
        cir.lhe_lookup(0, 3, 1, 0)            # row0 + 2 > 4
    plain = CI.Circuit()
    a = plain.inputs(2)
    plain.gate(NAND, a[0], a[1])
    assert not plain.has_lhe_nodes() and plain.census() == dict(gates=1, bootstrapped=1, mux=0, rotations=1, depth=1)


def test_simulate_array_read_at_every_address():
    from thfhe import circuits as CI
    cir = CI.Circuit()
    x = cir.inputs(20)
    scattered = [x[(7 * i) % 20] for i in range(16)]      # not consecutive: lhe_array_read copies them
    o = CI.lhe_array_read(cir, scattered, 0, 1, 3)
    o2 = CI.lhe_array_read(cir, x[2:18], 0, 3, 1)         # consecutive: no copies
    assert [g[0] for g in cir.gates].count(COPY) == 16
    rng = np.random.default_rng(5)
    w = _gate_words(rng.integers(0, 2, 20))
    for addr in range(16):
        v = CI.simulate(cir, w, [LR.address_bits([addr], 4)])
        assert v[o] == w[scattered[addr]] and v[o2] == w[x[2 + addr]], addr


def test_simulate_wfa_mux_max_on_every_pair():
    from thfhe import circuits as CI
    cir = CI.Circuit()
    a, b = cir.inputs(4), cir.inputs(4)
    m = CI.wfa_mux_max(cir, a, b, [0, 1], 4)
    assert cir.census()["bootstrapped"] == 4 and cir.census()["lhe_wfas"] == 1 and len(cir.levels()) == 2
    msb = lambda v: [(v >> (3 - i)) & 1 for i in range(4)]
    A, B = np.repeat(np.arange(16), 16), np.tile(np.arange(16), 16)
    bits = CI.wfa_pair_bits(A, B, 4)
    for q in range(256):
        v = CI.simulate(cir, _gate_words(msb(A[q]) + msb(B[q])), bits, instance=q)
        assert sum(int(v[m[i]] > 0) << (3 - i) for i in range(4)) == max(A[q], B[q]), (A[q], B[q])


def test_the_model_agrees_with_simulate_on_noiseless_samples(O, sk_small):
    # gates, a LOOKUP, GATHERs over gate outputs and a WFA feeding a MUX: every wire's decryption from the model equals simulate's word sign / digit
    from thfhe import circuits as CI, keygen
    import pack_reference as PR
    p, K, orc = sk_small
    rng = np.random.default_rng(77)
    pk = keygen.gen_pack_key(rng, K.lwe_key, K.rlwe_key[0], p.ks_t, p.ks_basebit, 0.0)
    cir = CI.Circuit()
    x = cir.inputs(8)
    g = [cir.gate(XOR if i & 1 else NAND, x[i], x[i + 1]) for i in range(4)]
    table = LR.table_polys(_gate_words(rng.integers(0, 2, (1, 8))), 1, 2)
    lk = cir.lhe_lookup(0, cir.lhe_table(table), 1, 2)
    ga = cir.lhe_gather(1, g[0], 0, 2)
    gb = cir.lhe_gather(0, x[0], 1, 2)
    m = CI.wfa_mux_max(cir, x[:2], x[2:4], [2, 3], 2)
    top = cir.gate(MUX, lk[0], ga, gb)
    for trial in range(3):
        bits_in = rng.integers(0, 2, 8)
        addr = [int(rng.integers(0, 8)), int(rng.integers(0, 4))]
        A, B = int(rng.integers(0, 4)), int(rng.integers(0, 4))
        plain = [LR.address_bits([addr[0]], 3), LR.address_bits([addr[1]], 2)] + CI.wfa_pair_bits([A], [B], 2)
        sim = CI.simulate(cir, _gate_words(bits_in), plain)
        recs = np.zeros((8, p.n + 1), np.int32)
        recs[:, -1] = _gate_words(bits_in)                 # trivial, noiseless
        Cs = [LR.trivial_tgsw(p, b[0]) for b in plain]
        vals = DL.evaluate(orc, cir, recs, Cs, pk, p.ks_t, p.ks_basebit)
        ph = PR.lwe_phase(vals, K.lwe_key)
        check = [w for w in range(cir.n_wires())]
        assert np.array_equal(np.asarray(ph)[check] > 0, sim[check] > 0), (trial, addr, A, B)
        assert np.abs(np.abs(np.asarray(ph, np.int64)[[ga, gb, lk[0]]]) - (1 << 29)).max() < 1 << 26


def test_gathered_wire_noise_in_the_model_on_sk128(O):
    # The model alone, on the seeds tests/test_gpu_dag_lhe.py uses: the gathered wires over gate outputs decrypt at +-1/8 and their noise is the
    # packing key switch's plus the final key switch's, sqrt(2) sigma_ks = 4.0e-3; the CMuxes and the packing add about 5e-4.  The
    # band [0.5, 1.5] x is the one DESIGN 4.10 and 4.11 use.  Measured on this model: 4.68e-3 at (1, 3), 3.85e-3 at (1, 2), 8 outputs each.
    import dag_lhe_cases as DC
    c = DC.array_read(O)
    S, ref, q = c["S"], c["ref"], np.arange(8)
    for name, wire, addr in (("(1, 3)", c["read16"], c["a16"]), ("(1, 2)", c["read8"], c["a8"])):
        want = c["want"][q, addr]
        assert np.array_equal(S.K.decrypt(ref[:, wire]), want), name
        std = DC.noise_std(S, ref[:, wire], want)
        print(f"\ngathered wires, SK-128 {name}: model std {std:.3e} over 8 outputs, sqrt(2) sigma_ks = {DC.SIGMA_GATHER:.1e}, ratio {std / DC.SIGMA_GATHER:.2f}")
        assert 0.5 * DC.SIGMA_GATHER <= std <= 1.5 * DC.SIGMA_GATHER, (name, std)
