"""Dense-layer nodes in the gate-DAG executor on the MI355X, single key (pytest -m gpu): thfhe_dag_run_dense_batch against
the level loop of flat calls (circuits.evaluate_levels, thfhe_linear_lut_bootstrap per node) and against the wire-by-wire model composed from the CPU
oracle's pieces (tests/dag_dense_reference.py), word for word.

  (1) tile edges: one DENSE node at every (M, K) around the kernel's output and reduction tiles on the 38-word record, with and without bias, theta
      1 / 2 / 4, with and without per-output tables, operand lists descending, with a repeat, and mixing inputs with a gate's output;
  (2) record widths: every shape of support.SHAPES at M = K = 17, and SK-128 (631 words: lanes past the record's end);
  (3) groups and slices: two rows of one entry and one of another on a level, a NOT of a LUT_OUT wire, gates and a LUT node between DENSE levels,
      the plan's figures, the same wires at every slice setting, out_wires, and a second run with a smaller layer on the same context;
  (4) with the other families: gate -> DENSE -> TREE and SELECT -> gate, and a DENSE output as an operand of a CB node whose set a LOOKUP reads;
  (5) the two-layer network of tests/test_gpu_linear.py with an argmax tail as ONE run on real SK-128 ciphertexts, decrypted exactly.

(1) - (4) run on random-word tables (and, but for the CB case, random records); the contract is word equality."""
import numpy as np
import pytest

import dag_dense_reference as DDR
from support import N, SHAPES, dec_int, differing, enc_int, pmap, shape_env, shape_id, sk128_cloud_key, words

pytestmark = pytest.mark.gpu
NAND, AND, NOT = 0, 2, 11
DAG_SLICE = 28672      # the single-key context's default (thfhe_set_dag_slice)


@pytest.fixture(scope="module")
def env(O):
    yield from shape_env(O)


@pytest.fixture(scope="module")
def env_pack(O):
    yield from shape_env(O, with_pack=True)


@pytest.fixture(scope="module")
def ck128(sk128):
    yield from sk128_cloud_key(sk128)


def same(got, ref, what):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.array_equal(got, ref), (what, differing(got, ref))


def one_node(rng, M, K, theta, bias, per_output, style, n_tables=3):
    """K + 1 inputs (at least 2), a NAND of the first two, and ONE DENSE node whose operand list follows `style`"""
    from thfhe import circuits as CI
    cir = CI.Circuit()
    x = cir.inputs(max(K + 1, 2))
    tids = [cir.table(words(rng, N)) for _ in range(n_tables)]
    g = cir.gate(NAND, x[0], x[1])
    ops = x[:K][::-1]                                   # descending
    if style == "repeat" and K > 1:
        ops[-1] = ops[0]
    if style == "mix":
        ops = x[:K]
        ops[K // 2] = g                                 # a gate's output among the inputs
    layer = cir.dense_layer(words(rng, M, K), words(rng, M) if bias else None, rng.integers(0, n_tables, M) if per_output else None, theta)
    outs = cir.dense(layer, ops)
    return cir, outs


def check(ck, orc, cir, x, what, model=True):
    """evaluate_batch = evaluate_levels (= the model) on every instance; returns the wires"""
    from thfhe import circuits as CI
    st = {}
    got = CI.evaluate_batch(ck, cir, x, stats=st)
    cen = cir.census()
    assert st["levels"] == cen["depth"] and st["rotations"] == cen["rotations"] * x.shape[0], (what, st, cen)
    for q in range(x.shape[0]):
        same(got[q], CI.evaluate_levels(ck, cir, x[q]), (what, "evaluate_levels", q))
        if model:
            same(got[q], DDR.evaluate(orc, cir, x[q], pmap=pmap), (what, "model", q))
    return got


# ---- (1) tile edges -------------------------------------------------------------------------------------------------------------------------------

EDGES = (1, 15, 16, 17, 33)
STYLES = ("desc", "repeat", "mix")


@pytest.mark.parametrize("M", EDGES)
def test_tile_edges(env, M):
    shape = SHAPES[2]
    assert shape[0] == 37
    p, K_, orc, ck = env(shape)
    assert ck.linear_tile() == (16, 16)
    rng = np.random.default_rng(2500 + M)
    seen = set()
    for ik, K in enumerate(EDGES):
        v = EDGES.index(M) * len(EDGES) + ik
        theta, bias, per_output, style = (1, 2, 4)[v % 3], v % 2 == 0, (v // 2) % 2 == 0, STYLES[(v // 3) % 3]
        seen.add((theta, bias, per_output, style))
        cir, outs = one_node(rng, M, K, theta, bias, per_output, style)
        assert len(outs) == M and all(len(o) == theta for o in outs)
        check(ck, orc, cir, words(rng, 1, cir.n_inputs, p.n + 1), (M, K, theta, bias, per_output, style))
    assert len(seen) == len(EDGES)


@pytest.mark.parametrize("M,K", [(17, 33), (33, 17)])
def test_tile_corners_with_every_variant_crossed(env, M, K):
    # the sweep above rotates the variants over the (M, K) pairs; here all 36 of them meet one pair on either side of both tiles
    p, K_, orc, ck = env(SHAPES[2])
    rng = np.random.default_rng(2560 + M)
    for theta in (1, 2, 4):
        for bias in (False, True):
            for per_output in (False, True):
                for style in STYLES:
                    cir, outs = one_node(rng, M, K, theta, bias, per_output, style)
                    check(ck, orc, cir, words(rng, 1, cir.n_inputs, p.n + 1), (M, K, theta, bias, per_output, style))


def test_every_variant_occurs_in_the_tile_edge_sweep():
    got = set()
    for v in range(len(EDGES) ** 2):
        got.add(((1, 2, 4)[v % 3], v % 2 == 0, (v // 2) % 2 == 0, STYLES[(v // 3) % 3]))
    assert {g[0] for g in got} == {1, 2, 4} and {g[3] for g in got} == set(STYLES)
    for theta in (1, 2, 4):
        assert {(g[1], g[2]) for g in got if g[0] == theta} == {(a, b) for a in (False, True) for b in (False, True)}


def test_the_bias_lands_on_the_body_word_only(env):
    # zero operand records: every sum is (0, ..., 0, bias[m]), so output m equals the flat LUT bootstrap of that record
    from thfhe import circuits as CI
    p, K_, orc, ck = env(SHAPES[2])
    rng = np.random.default_rng(2590)
    cir, outs = one_node(rng, 17, 17, 1, True, True, "desc")
    W, b, tids, theta = cir.dense_specs[0]
    x = np.zeros((1, cir.n_inputs, p.n + 1), np.int32)
    x[0, 17] = words(rng, p.n + 1)                       # the one input the node does not read
    got = CI.evaluate_batch(ck, cir, x, out_wires=[o[0] for o in outs])
    recs = np.zeros((17, p.n + 1), np.int32)
    recs[:, -1] = b
    ref = ck.lut_bootstrap(np.stack(cir.tables), recs, lut_index=tids)[:, 0]
    same(got[0], ref, "bias on the body word")


# ---- (2) record widths ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_record_widths(env, shape):
    p, K_, orc, ck = env(shape)
    rng = np.random.default_rng(2600 + shape[0])
    cir, outs = one_node(rng, 17, 17, 2, True, True, "mix")
    check(ck, orc, cir, words(rng, 1, cir.n_inputs, p.n + 1), shape)


def test_record_width_of_sk128(sk128, ck128):
    p, K_, orc = sk128
    assert ck128.words == 631
    rng = np.random.default_rng(2631)
    cir, outs = one_node(rng, 3, 5, 1, True, True, "mix")
    check(ck128, orc, cir, words(rng, 2, cir.n_inputs, 631), "sk128")


# ---- (3) groups and slices ------------------------------------------------------------------------------------------------------------------------

def grouped(rng):
    """level 1: layer A (M = 3, K = 2, per-output tables) at two wire_offs and layer B (M = 2, K = 3, theta = 2) once, a NOT of a LUT_OUT wire;
    level 2: a NAND of two DENSE outputs and a LUT node; level 3: layer A again on the LUT node's and the NOT's wires"""
    from thfhe import circuits as CI
    cir = CI.Circuit()
    x = cir.inputs(6)
    t = [cir.table(words(rng, N)) for _ in range(3)]
    A = cir.dense_layer(words(rng, 3, 2), words(rng, 3), [2, 0, 1])
    B = cir.dense_layer(words(rng, 2, 3), None, None, theta=2)
    a1 = cir.dense(A, [x[0], x[1]])
    a2 = cir.dense(A, [x[3], x[2]])
    b1 = cir.dense(B, [x[5], x[4], x[0]])
    n = cir.gate(NOT, a1[1][0])
    g = cir.gate(NAND, a1[0][0], b1[1][1])
    l = cir.lut(t[1], [a2[2][0]], weights=(3,), bias=12345)[0]
    a3 = cir.dense(A, [l, n])
    return cir, dict(a1=a1, a2=a2, b1=b1, n=n, g=g, l=l, a3=a3)


def test_groups_and_slices(env):
    import thfhe
    from thfhe import circuits as CI
    shape = SHAPES[3]
    p, K_, orc, ck = env(shape)
    rng = np.random.default_rng(2700)
    Q, M = 3, 3
    cir, w = grouped(rng)
    x = words(rng, Q, 6, p.n + 1)
    st = {}
    got = CI.evaluate_batch(ck, cir, x, stats=st)
    # three levels; launch groups: layer A, layer B | the NAND, the LUT node | layer A; rotations per instance 3 + 3 + 2 | 1 + 1 | 3
    assert (st["levels"], st["launches"], st["rotations"], st["widest_level"], st["instances"]) == (3, 5, 13 * Q, 2 * Q, Q)
    for q in range(Q):
        same(got[q], CI.evaluate_levels(ck, cir, x[q]), ("evaluate_levels", q))
        same(got[q], DDR.evaluate(orc, cir, x[q], pmap=pmap), ("model", q))
    try:
        # one node per slice | one sample per slice (M > 1) | two samples per slice of the cnt = 2 group | three: slices that begin and end inside an instance
        for name, dag, lin in (("dag_slice 1", 1, 4096), ("linear_slice 1", DAG_SLICE, 1), ("linear_slice 2M", DAG_SLICE, 2 * M), ("linear_slice 3M", DAG_SLICE, 3 * M),
                               ("linear_slice 2M - 1", DAG_SLICE, 2 * M - 1)):
            ck.set_dag_slice(dag)
            ck.set_linear_slice(lin)
            same(CI.evaluate_batch(ck, cir, x), got, name)
    finally:
        ck.set_dag_slice(DAG_SLICE)
        ck.set_linear_slice(4096)
    # the stage timer: refused without a profiled run, then three finite times whose levels hold the last group's
    with pytest.raises(thfhe.ThfheError, match="no profiled run"):
        ck.dag_last_stage_ms()
    ck.set_profiling(True)
    try:
        same(CI.evaluate_batch(ck, cir, x), got, "profiled")
        ms = ck.dag_last_stage_ms()
        assert all(np.isfinite(v) and v >= 0 for v in ms.values()) and ms["levels_ms"] >= ck.dag_last_group_ms() > 0, ms
        assert ck.linear_last_timings()["linear_ms"] > 0
    finally:
        ck.set_profiling(False)
    sel = [w["a3"][2][0], w["b1"][0][1], w["n"], w["a2"][1][0], 0]
    same(CI.evaluate_batch(ck, cir, x, out_wires=sel), got[:, sel], "out_wires")
    # a second run on the same context: a smaller layer without per-output tables -- no table index and no sum survives from the run before
    other = CI.Circuit()
    y = other.inputs(3)
    for tv in cir.tables:
        other.table(tv)
    C = other.dense_layer(words(rng, 2, 2), words(rng, 2))
    c1 = other.dense(C, [y[2], y[0]])
    other.dense(C, [c1[1][0], y[1]])
    x2 = words(rng, Q, 3, p.n + 1)
    got2 = CI.evaluate_batch(ck, other, x2)
    for q in range(Q):
        same(got2[q], CI.evaluate_levels(ck, other, x2[q]), ("second run, evaluate_levels", q))
        same(got2[q], DDR.evaluate(orc, other, x2[q], pmap=pmap), ("second run, model", q))
    same(CI.evaluate_batch(ck, cir, x), got, "the first circuit again")


# ---- (4) with the other families ------------------------------------------------------------------------------------------------------------------

def test_gate_dense_tree_select_gate(env_pack):
    from thfhe import circuits as CI
    shape = SHAPES[3]
    p, K_, orc, ck, pc, pk = env_pack(shape)
    rng = np.random.default_rng(2800)
    cir = CI.Circuit()
    x = cir.inputs(3)
    cir.table(words(rng, N))
    g = cir.gate(NAND, x[0], x[1])
    d = cir.dense(cir.dense_layer(words(rng, 4, 3), words(rng, 4)), [g, x[2], x[0]])
    t = cir.tree(cir.tree_rows(words(rng, 2, N)), [d[0][0]], [d[1][0]], 4, lo_weights=(3,), hi_weights=(-5,), lo_bias=1234567, hi_bias=-7654321, theta1=2)
    s = cir.select([x[1]], d[0][0], 4, weights=(7,), bias=99)         # picks among the node's four output wires
    f = cir.gate(NAND, t, s)
    Q = 2
    xs = words(rng, Q, 3, p.n + 1)
    st = {}
    got = CI.evaluate_batch(ck, cir, xs, stats=st, pack=pc)
    assert st["levels"] == 4 and st["rotations"] == Q * (1 + 4 + (2 + 1) + 1 + 1)
    for q in range(Q):
        same(got[q], CI.evaluate_levels(ck, cir, xs[q], pack=pc), ("evaluate_levels", q))
    assert f == cir.n_wires() - 1


def test_a_dense_output_feeds_a_cb_node_whose_set_a_lookup_reads(O):
    import dag_cb_cases as DC
    import thfhe
    from thfhe import circuits as CI
    from thfhe import lut
    import cb_cases as CC
    S = DC.keys(O, "SK-128", device=0)
    ck = thfhe.CloudKey(S.tp, S.K.bk, S.K.ksk, device=0)
    ck2 = thfhe.MKCloudKey(S.tp2, S.K2.bk, S.K2.ksk, device=0)
    try:
        ck.cb_key_set(ck2, S.pks, CC.T, CC.BASEBIT)
        rng = np.random.default_rng(2850)
        cir = CI.Circuit()
        x = cir.inputs(3)
        # a gate bit (+-1/8) at weight 1 with bias 1/8 is the p = 2 message 0 / 1; the outputs are gate bits again: the bit and its complement
        t_id = cir.table(lut.test_vector(lut.bool_outputs(lambda m: m == 1, 2), 2))
        t_not = cir.table(lut.test_vector(lut.bool_outputs(lambda m: m == 0, 2), 2))
        g = cir.gate(3, x[0], x[1])                                        # XOR
        d = cir.dense(cir.dense_layer([[1, 0], [0, 1]], [1 << 29, 1 << 29], [t_id, t_not]), [g, x[2]])
        s = cir.cb_set([d[0][0], d[1][0]])
        o = cir.lhe_lookup(s, cir.lhe_table(words(rng, 2, N)), 1, 1)[0]
        cir.gate(NAND, o, x[0])
        bits = np.array([[(q >> i) & 1 for i in range(3)] for q in (1, 5, 6)])      # both values of the XOR and of the third bit
        xs = DC.encrypt(S, bits, 0xDE25C)
        got = CI.evaluate_batch(ck, cir, xs)
        for q in range(len(bits)):
            same(got[q], CI.evaluate_levels(ck, cir, xs[q]), ("evaluate_levels", q))
        gb = bits[:, 0] ^ bits[:, 1]
        assert np.array_equal(S.K.decrypt(got[:, d[0][0]]), gb.astype(bool)) and np.array_equal(S.K.decrypt(got[:, d[1][0]]), ~bits[:, 2].astype(bool))
    finally:
        ck.close()
        ck2.close()


# ---- (5) a real network -----------------------------------------------------------------------------------------------------------------------------

def test_network_with_an_argmax_tail_as_one_run_on_sk128(sk128, ck128):
    """The network of tests/test_gpu_linear.py as one circuit: 7 fresh bits at p = 8 -> three threshold neurons at p = 4 -> majority, and a
    dense_argmax tail on the three neurons (LUT nodes on h_i - h_j + 2 at p = 4, NOTs and ANDs).  Margins: layer 1 reads fresh inputs
    (any row of W1 in {0, 1}^7: 12.9 sigma); layer 2 and the comparisons read bootstrapped wires, sum of W^2 = 3 and 2, inside the 7 that p = 4
    affords (9.5 sigma at 3)."""
    from thfhe import circuits as CI
    from thfhe import lut
    p, K, orc = sk128
    ck = ck128
    rng = np.random.default_rng(2900)
    Q = 8
    bits = rng.integers(0, 2, (Q, 7))
    bits[0], bits[1] = 0, 1
    W1 = np.array([[1, 1, 1, 1, 1, 1, 1], [1, 1, 1, 1, 0, 0, 0], [1, 0, 1, 0, 1, 0, 1]], np.int32)
    thr = [4, 2, 2]
    W2 = np.array([[1, 1, 1]], np.int32)
    cir = CI.Circuit()
    x = cir.inputs(7)
    t1 = [cir.table(lut.test_vector(lut.int_outputs(lambda s, t=t: int(s >= t), 4, 8), 8)) for t in thr]
    t2 = cir.table(lut.test_vector(lut.int_outputs(lambda s: int(s >= 2), 4, 4), 4))
    h, out = CI.dense_network(cir, x, [(W1, None, t1), (W2, None, [t2])])
    win = CI.dense_argmax(cir, h, 4)

    # the conditions, on the plaintext side: sum of W^2 on bootstrapped wires, and every reachable sum inside [0, p)
    assert (W2.astype(np.int64) ** 2).sum(axis=1).max() <= 7 and W1.max() <= 1 and W1.min() >= 0
    assert np.maximum(W1, 0).sum(axis=1).max() * 1 < 8 and np.maximum(W2, 0).sum(axis=1).max() * 1 < 4
    sums1 = CI.dense_plain(W1, None, bits, 8)
    want1 = (sums1 >= np.array(thr)).astype(np.int64)
    sums2 = CI.dense_plain(W2, None, want1, 4)
    want2 = (sums2 >= 2).astype(np.int64)
    wantw = CI.dense_argmax_plain(want1)
    assert sums1.max() < 8 and sums2.max() < 4 and len(set(want2.reshape(-1).tolist())) == 2 and len({tuple(r) for r in wantw.tolist()}) >= 2
    xs = enc_int(K, bits.reshape(-1), 8, 2901).reshape(Q, 7, p.n + 1)

    # the CPU reference alone decrypts every instance to the plaintext network's answers
    ref = np.stack(pmap(lambda q: DDR.evaluate(orc, cir, xs[q]), range(Q)))
    assert np.array_equal(dec_int(K, ref[:, h].reshape(-1, p.n + 1), 4).reshape(Q, 3), want1)
    assert np.array_equal(dec_int(K, ref[:, out].reshape(-1, p.n + 1), 4).reshape(Q, 1), want2)
    assert np.array_equal(K.phases(ref[:, win].reshape(-1, p.n + 1)).reshape(Q, 3) > 0, wantw.astype(bool))

    st = {}
    got = CI.evaluate_batch(ck, cir, xs, stats=st)
    same(got, ref, "every wire of every instance equals the model")
    assert st["levels"] == cir.census()["depth"] and st["rotations"] == Q * (3 + 1 + 3 + 3)
    assert np.array_equal(dec_int(K, got[:, out].reshape(-1, p.n + 1), 4).reshape(Q, 1), want2)
    assert np.array_equal(K.phases(got[:, win].reshape(-1, p.n + 1)).reshape(Q, 3) > 0, wantw.astype(bool))
    same(CI.evaluate_levels(ck, cir, xs[3]), got[3], "evaluate_levels")
