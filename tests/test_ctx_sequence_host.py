"""Conditions on the catalogue and the orders of the long-lived-context tests (tests/ctx_sequence.py), checked without a device: what the GPU
files rely on -- that every op runs in every order, that every family meets the three situations the orders exist for, that an op's inputs do not
depend on where it sits, and that every reference is computable from the CPU models alone.

Measured on the CPU (one run, 8 model threads): every reference of the single-key catalogue in 2.9 s, of MK2 in 1.6 s, of MK4-N2048 in 3.2 s,
of MK64-fft in 6.5 s, of CCS2 and KMS2 in 1 s together -- none needs a slow mark."""
import numpy as np
import pytest

import ctx_sequence as CS


@pytest.fixture(scope="module")
def catalogues(O):
    out = {}
    for name in ("sk", "MK2", "MK4-N2048", "MK64-fft"):
        env = CS.SkEnv(O) if name == "sk" else CS.MkEnv(O, name)
        out[name] = (env, CS.sk_catalogue(env) if name == "sk" else CS.mk_catalogue(env))
    return out


def sequences(cat):
    """every sequence that runs on one context of its own: the orders, and the cold pairs"""
    return list(CS.orders(cat).values()) + CS.cold(cat)


@pytest.mark.parametrize("name", ["sk", "MK2"])
def test_every_family_has_both_sizes_and_every_op_is_in_every_order(catalogues, name):
    env, cat = catalogues[name]
    assert len({op.name for op in cat}) == len(cat)
    for f in CS.families(cat):
        assert {op.size for op in cat if op.family == f} == {"small", "large"}, f
    for order, seq in CS.orders(cat).items():
        assert {op.name for op in seq} == {op.name for op in cat}, order
    assert len(CS.orders(cat)) == 5 and len(CS.SHUFFLE_SEEDS) == 2


@pytest.mark.parametrize("name", ["sk", "MK2"])
def test_every_family_meets_the_three_situations(catalogues, name):
    env, cat = catalogues[name]
    seqs = sequences(cat)
    first_large, small_after_other_large, large_after_own_small = set(), set(), set()
    for seq in seqs:
        if seq[0].size == "large":
            first_large.add(seq[0].family)
        for prev, op in zip(seq, seq[1:]):
            if op.size == "small" and prev.size == "large" and prev.family != op.family:
                small_after_other_large.add(op.family)
        for i, op in enumerate(seq):
            if op.size == "large" and any(q.family == op.family and q.size == "small" for q in seq[:i]):
                large_after_own_small.add(op.family)
    fam = set(CS.families(cat))
    assert first_large == fam, fam - first_large
    assert small_after_other_large == fam, fam - small_after_other_large
    assert large_after_own_small == fam, fam - large_after_own_small


@pytest.mark.parametrize("name", ["sk", "MK2", "MK4-N2048", "MK64-fft"])
def test_inputs_do_not_depend_on_the_position(O, catalogues, name):
    # the catalogue built twice, the inputs drawn in opposite orders: byte for byte the same
    env, cat = catalogues[name]
    env2 = CS.SkEnv(O) if name == "sk" else CS.MkEnv(O, name)
    cat2 = CS.sk_catalogue(env2) if name == "sk" else CS.mk_catalogue(env2)
    assert [op.name for op in cat] == [op.name for op in cat2]
    a = {op.name: op.inputs(env) for op in cat}
    b = {op.name: op.inputs(env2) for op in reversed(cat2)}
    for n in a:
        assert a[n].keys() == b[n].keys()
        for k in a[n]:
            x, y = np.asarray(a[n][k]), np.asarray(b[n][k])
            assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), (n, k)
    if name == "sk":
        assert all(x.tobytes() == y.tobytes() for x, y in zip(env.Cs, env2.Cs)) and env.pk.tobytes() == env2.pk.tobytes()
    else:
        assert env.pk.tobytes() == env2.pk.tobytes() and env.pk_small.tobytes() == env2.pk_small.tobytes()


@pytest.mark.parametrize("name", ["sk", "MK2", "MK4-N2048", "MK64-fft", "CCS2", "KMS2"])
def test_every_reference_is_computable_on_the_cpu(O, catalogues, name):
    if name in catalogues:
        env, cat = catalogues[name]
        cat = cat + ([CS.small_key_op(env)] if name != "sk" else [])
    else:
        env = CS.GateEnv(O, name)
        cat = CS.gate_sequence(env)
        assert [len(op.inputs(env)["x"]) for op in cat] == [2, 19, 2]
    CS.references(env, cat)
    for op in cat:
        ref = op.reference(env)
        assert len(ref) >= 1 and all(isinstance(r, np.ndarray) and r.size and r.dtype in (np.int32, np.int64) for r in ref), op.name
        assert any(len(np.unique(r)) > r.size // 2 for r in ref), op.name      # words, not a constant


def test_the_sizes_are_what_the_orders_assume(catalogues):
    env, cat = catalogues["sk"]
    for op in cat:
        n = len(next(iter(op.reference(env))))
        want = {"small": (CS.SMALL, CS.SMALL_TREE, CS.SMALL_DAG), "large": (CS.LARGE, CS.LARGE_TREE, CS.LARGE_DAG)}[op.size]
        assert n in want or op.family == "lhe_scatter", (op.name, n)      # a scatter returns its two tables
    assert CS.LARGE % 2 == 1 and CS.LARGE > 2 * 8 and CS.LARGE > 4 * 4 and CS.LARGE % 8 and CS.LARGE % 4
