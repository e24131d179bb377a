"""The dense-layer node on a long-lived context (pytest -m gpu; DESIGN.md sections 2.1 and 4.25), in the idiom of tests/ctx_sequence.py: three call
families at two sizes -- the flat thfhe_linear_lut_bootstrap, a gate DAG with DENSE nodes (thfhe_dag_run_dense_batch) and a gates-only DAG
(thfhe_dag_run_batch) -- interleaved on ONE context in the orders defined there.  Every output word of every call must equal what the same call
returns as the FIRST call of a fresh context.  The three share lin.x, the PBS workspace, the table index array and the staging output, so this aims at
a sum, an index or a record that survives from a larger call, and at a pointer taken before the grow that replaces it."""
import numpy as np
import pytest

import ctx_sequence as CS
from support import N, words

pytestmark = pytest.mark.gpu
NAND, XOR, NOT = 0, 3, 11


def dense_circuit(rng):
    """gate -> two rows of one layer and one of another -> LUT node and NOT -> the first layer again"""
    from thfhe import circuits as CI
    cir = CI.Circuit()
    x = cir.inputs(5)
    t = [cir.table(words(rng, N)) for _ in range(3)]
    g = cir.gate(XOR, x[0], x[1])
    A = cir.dense_layer(words(rng, 5, 3), words(rng, 5), [2, 0, 1, 1, 2], theta=2)
    B = cir.dense_layer(words(rng, 2, 2), None, None)
    a1 = cir.dense(A, [x[4], g, x[2]])
    a2 = cir.dense(A, [x[3], x[3], x[0]])
    b1 = cir.dense(B, [g, x[1]])
    n = cir.gate(NOT, a2[4][1])
    l = cir.lut(t[0], [b1[1][0], a1[0][1]], weights=(2, -3), bias=777)[0]
    cir.dense(B, [n, l])
    return cir


def gate_circuit():
    from thfhe import circuits as CI
    cir = CI.Circuit()
    x = cir.inputs(4)
    a = cir.gate(NAND, x[0], x[1])
    b = cir.gate(XOR, x[2], a)
    cir.gate(10, a, b, x[3])          # MUX
    cir.gate(NOT, b)
    return cir


def catalogue():
    from thfhe import circuits as CI
    M, K = 7, 5
    idx = np.array([2, 0, 1, 1, 0, 2, 2], np.int32)

    def flat_make(rng, env, count):
        return dict(W=words(rng, M, K), b=words(rng, M), tv=words(rng, 3, N), x=words(rng, count, K, env.words))

    def dag_make(rng, env, count):
        return dict(cir=dense_circuit(rng), x=words(rng, count, 5, env.words))

    def gates_make(rng, env, count):
        return dict(cir=gate_circuit(), x=words(rng, count, 4, env.words))
    fresh = lambda env, I: None       # the reference is the call on a fresh context (World.reference)
    flat = CS.both_sizes("linear_lut_bootstrap-theta2-index", CS.SMALL, CS.LARGE, flat_make,
                         lambda ck, env, I: (ck.linear_lut_bootstrap(I["tv"], I["W"], I["x"], I["b"], theta=2, lut_index=idx),), fresh)
    dense = CS.both_sizes("dag_run_dense_batch", CS.SMALL_DAG, CS.LARGE_DAG, dag_make, lambda ck, env, I: (CI.evaluate_batch(ck, I["cir"], I["x"]),), fresh,
                          kind="dag-group")
    gates = CS.both_sizes("dag_run_batch", CS.SMALL_DAG, CS.LARGE_DAG, gates_make, lambda ck, env, I: (CI.evaluate_batch(ck, I["cir"], I["x"]),), fresh, kind="dag")
    return flat + dense + gates


@pytest.fixture(scope="module")
def world(O):
    env = CS.SkEnv(O)
    cat = catalogue()
    for op in cat:                    # every op's result as the first call of a context of its own
        ck = env.cloud_key()
        try:
            env.refs[op.name] = op.run(ck, env)
        finally:
            ck.close()
    return env, cat


@pytest.mark.parametrize("order", ["catalogue", "big-then-small", "small-big-small", "alternating", "shuffled-1"])
def test_order_on_one_context(world, order):
    env, cat = world
    seq = cat if order == "catalogue" else CS.orders(cat)[order]
    assert {op.name for op in seq} == {op.name for op in cat} and len(CS.families(cat)) == 3
    ck = env.cloud_key()
    try:
        for pos, op in enumerate(seq):
            CS.check(op.run(ck, env), env.refs[op.name], op, seq[pos - 1].name if pos else "context creation", pos)
    finally:
        ck.close()


def test_the_level_loop_agrees_with_the_fresh_context_results(world):
    # the references above are the engine's own; tie them to the flat calls once: the small DENSE run against evaluate_levels
    from thfhe import circuits as CI
    env, cat = world
    op = CS.by(cat, "dag_run_dense_batch", "small")
    I = op.inputs(env)
    ck = env.cloud_key()
    try:
        for q in range(I["x"].shape[0]):
            assert np.array_equal(CI.evaluate_levels(ck, I["cir"], I["x"][q]), env.refs[op.name][0][q])
    finally:
        ck.close()
