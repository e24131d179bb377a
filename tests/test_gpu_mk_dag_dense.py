"""Dense-layer nodes in the 3-gen gate-DAG executor on the MI355X (pytest -m gpu): thfhe_mk_dag_run_dense_batch on MK2
(n = 30) and MK4-N2048 (n = 10, two parties), Torus64 tables and records of P n + 1 words, against the level loop of flat calls
(circuits.evaluate_levels, thfhe_mk_linear_lut_bootstrap per node) and the wire-by-wire model composed from the CPU oracle's pieces
(tests/dag_dense_reference.py), word for word: one DENSE node at every (M, K) in {1, 16, 17}^2 with the variants of the single-key sweep; two rows of
one entry and one of another on a level with gates and a LUT node between DENSE levels, the plan's figures and every slice setting; and a DENSE ->
TREE_MV chain on the D = N packing key.  Tables, records and the packing key are random words: only word equality is asserted."""
import numpy as np
import pytest

import dag_dense_reference as DDR
from support import differing, pmap, words

pytestmark = pytest.mark.gpu
NAND, NOT = 0, 11
T_PK, BASEBIT = 2, 1      # the D = N packing key's digits
SETS = [("MK2", dict(n=30)), ("MK4-N2048", dict(n=10, parties=2))]
EDGES = (1, 16, 17)
STYLES = ("desc", "repeat", "mix")


def words64(rng, *shape):
    return rng.integers(-2**63, 2**63, size=shape, dtype=np.int64)


@pytest.fixture(scope="module")
def keys(O):
    """name -> (params, oracle, MKCloudKey), built once per set, every context closed at the end"""
    import thfhe
    made = {}

    def get(name):
        if name not in made:
            p = O.make_params(name, **dict(SETS)[name])
            s = O.SIGMAS[name]
            K = O.MKKeys(p, 71, s["bk"], s["ks"])
            made[name] = (p, O.MKOracle(p, K.bk, K.ksk), thfhe.MKCloudKey(thfhe.make_params(**p.as_dict()), K.bk, K.ksk, device=0))
        return made[name]
    yield get
    for v in made.values():
        v[2].close()


def same(got, ref, what):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.array_equal(got, ref), (what, differing(got, ref))


def one_node(rng, N, M, K, theta, bias, per_output, style, n_tables=3):
    from thfhe import circuits as CI
    cir = CI.Circuit()
    x = cir.inputs(max(K + 1, 2))
    tids = [cir.table(words64(rng, N)) for _ in range(n_tables)]
    g = cir.gate(NAND, x[0], x[1])
    ops = x[:K][::-1]
    if style == "repeat" and K > 1:
        ops[-1] = ops[0]
    if style == "mix":
        ops = x[:K]
        ops[K // 2] = g
    layer = cir.dense_layer(words(rng, M, K), words(rng, M) if bias else None, rng.integers(0, n_tables, M) if per_output else None, theta)
    return cir, cir.dense(layer, ops)


def check(ck, orc, cir, x, what):
    from thfhe import circuits as CI
    st = {}
    got = CI.evaluate_batch(ck, cir, x, stats=st)
    cen = cir.census()
    assert st["levels"] == cen["depth"] and st["rotations"] == cen["rotations"] * x.shape[0], (what, st, cen)
    for q in range(x.shape[0]):
        same(got[q], CI.evaluate_levels(ck, cir, x[q]), (what, "evaluate_levels", q))
        same(got[q], DDR.evaluate(orc, cir, x[q], multi_key=True, pmap=pmap), (what, "model", q))
    return got


@pytest.mark.parametrize("M", EDGES)
@pytest.mark.parametrize("name", [s[0] for s in SETS])
def test_tile_edges(keys, name, M):
    p, orc, ck = keys(name)
    assert ck.words == p.parties * p.n + 1 and ck.linear_tile() == (16, 16)
    rng = np.random.default_rng(3500 + M + p.N)
    for ik, K in enumerate(EDGES):
        v = EDGES.index(M) * len(EDGES) + ik + (0 if name == "MK2" else 5)
        theta, bias, per_output, style = (1, 2, 4)[v % 3], v % 2 == 0, (v // 2) % 2 == 0, STYLES[(v // 3) % 3]
        cir, outs = one_node(rng, p.N, M, K, theta, bias, per_output, style)
        assert len(outs) == M and all(len(o) == theta for o in outs)
        check(ck, orc, cir, words(rng, 1, cir.n_inputs, ck.words), (name, M, K, theta, bias, per_output, style))


def grouped(rng, N):
    """level 1: layer A (M = 3, K = 2, per-output tables) at two wire_offs and layer B (M = 2, K = 3, theta = 2) once, a NOT of a LUT_OUT wire;
    level 2: a NAND of two DENSE outputs and a LUT node; level 3: layer A again on the LUT node's and the NOT's wires"""
    from thfhe import circuits as CI
    cir = CI.Circuit()
    x = cir.inputs(6)
    t = [cir.table(words64(rng, N)) for _ in range(3)]
    A = cir.dense_layer(words(rng, 3, 2), words(rng, 3), [2, 0, 1])
    B = cir.dense_layer(words(rng, 2, 3), None, None, theta=2)
    a1 = cir.dense(A, [x[0], x[1]])
    a2 = cir.dense(A, [x[3], x[2]])
    b1 = cir.dense(B, [x[5], x[4], x[0]])
    n = cir.gate(NOT, a1[1][0])
    cir.gate(NAND, a1[0][0], b1[1][1])
    l = cir.lut(t[1], [a2[2][0]], weights=(3,), bias=12345)[0]
    a3 = cir.dense(A, [l, n])
    return cir, [a3[2][0], b1[0][1], n, a2[1][0], 0]


@pytest.mark.parametrize("name", [s[0] for s in SETS])
def test_groups_and_slices(keys, name):
    from thfhe import circuits as CI
    p, orc, ck = keys(name)
    rng = np.random.default_rng(3700 + p.N)
    Q, M = 3, 3
    cir, sel = grouped(rng, p.N)
    x = words(rng, Q, 6, ck.words)
    st = {}
    got = CI.evaluate_batch(ck, cir, x, stats=st)
    assert (st["levels"], st["launches"], st["rotations"], st["widest_level"], st["instances"]) == (3, 5, 13 * Q, 2 * Q, Q)
    for q in range(Q):
        same(got[q], CI.evaluate_levels(ck, cir, x[q]), ("evaluate_levels", q))
        same(got[q], DDR.evaluate(orc, cir, x[q], multi_key=True, pmap=pmap), ("model", q))
    try:
        for what, dag, lin in (("dag_slice 1", 1, 4096), ("linear_slice 1", 8192, 1), ("linear_slice 2M", 8192, 2 * M), ("linear_slice 3M", 8192, 3 * M)):
            ck.set_dag_slice(dag)
            ck.set_linear_slice(lin)
            same(CI.evaluate_batch(ck, cir, x), got, what)
    finally:
        ck.set_dag_slice(8192)
        ck.set_linear_slice(4096)
    same(CI.evaluate_batch(ck, cir, x, out_wires=sel), got[:, sel], "out_wires")
    # a second run on the same context: a smaller layer without per-output tables
    other = CI.Circuit()
    y = other.inputs(3)
    for tv in cir.tables:
        other.table(tv)
    C = other.dense_layer(words(rng, 2, 2), words(rng, 2))
    c1 = other.dense(C, [y[2], y[0]])
    other.dense(C, [c1[1][0], y[1]])
    x2 = words(rng, Q, 3, ck.words)
    got2 = CI.evaluate_batch(ck, other, x2)
    for q in range(Q):
        same(got2[q], CI.evaluate_levels(ck, other, x2[q]), ("second run, evaluate_levels", q))
    same(CI.evaluate_batch(ck, cir, x), got, "the first circuit again")


@pytest.mark.parametrize("name", [s[0] for s in SETS])
def test_dense_feeds_a_multi_value_tree(keys, name):
    from thfhe import circuits as CI
    p, orc, ck = keys(name)
    rng = np.random.default_rng(3800 + p.N)
    cir = CI.Circuit()
    a, b = cir.inputs(2)
    cir.table(words64(rng, p.N))
    g = cir.gate(NAND, a, b)
    d = cir.dense(cir.dense_layer(words(rng, 2, 3), words(rng, 2)), [g, b, a])
    m = cir.tree_mv(cir.mv_base(words64(rng, p.N)), rng.integers(-3, 4, (2, 4, 4)).astype(np.int32), [d[0][0]], [d[1][0]], lo_weights=(3,), hi_weights=(-5,),
                    lo_bias=1234567, hi_bias=-7654321, out_bias=int(rng.integers(-2**63, 2**63, dtype=np.int64)))
    cir.gate(NAND, m[0], m[1])
    Q = 2
    x = words(rng, Q, 2, ck.words)
    ck.pack_key_set(words64(rng, p.N, T_PK, (1 << BASEBIT) - 1, 2, p.N), T_PK, BASEBIT)
    st = {}
    got = CI.evaluate_batch(ck, cir, x, stats=st)
    assert st["levels"] == 4 and st["rotations"] == Q * (1 + 2 + (1 + 2) + 1)
    for q in range(Q):
        same(got[q], CI.evaluate_levels(ck, cir, x[q]), ("evaluate_levels", q))
