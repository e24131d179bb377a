"""Leveled nodes in the gate-DAG executor on every decomposition length (pytest -m gpu): thfhe_dag_run_lhe_batch at
(l, Bgbit) = (1, 8), (2, 10), (3, 7), (4, 8) -- the first four shapes of support.py -- on 3 instances of random words, every output wire word for
word against the model (dag_lhe_reference.py) and against the flat calls in a row (circuits.evaluate_levels).  The TGSW samples and the tables are
random words, not valid ciphertexts; the contract is word equality.

One circuit per table kind (public / encrypted) holds every case: LOOKUP nodes at (d_tree, d_rot, theta) = (0, 2, 4), (2, 1, 2) and (1, 0, 1) with
row0 > 0 -- three specs on the first level; GATHER nodes at (0, 1) over inputs, (0, 3) over four gate outputs and the four wires of a many-LUT
node, (2, 2) over inputs, gate outputs and LUT_OUT wires, and a GATHER over two GATHER outputs; a WFA node with one state (a copy) and one with
3 states, theta = 2, n_out = 2 over two sets whose steps 0 and 2 read one bit."""
import numpy as np
import pytest

import dag_lhe_reference as DL
from support import N, SHAPES, differing, pmap, shape_env, shape_id, words

pytestmark = pytest.mark.gpu

LHE_SHAPES = SHAPES[:4]
COUNT = 3
SET_D = (2, 3, 1, 4)
NAND, XOR = 0, 3
TRANS3 = np.array([[[1, 2], [2, 0], [0, 1]], [[0, 0], [2, 1], [1, 2]], [[2, 1], [0, 2], [1, 1]]], np.int32)   # step 1: state 0 is a copy
STEP3 = np.array([16 * 1 + 2, 16 * 0 + 1, 16 * 1 + 2], np.int32)                                            # bit 2 of set 1 twice
START3 = np.array([2, 0], np.int32)


@pytest.fixture(scope="module")
def env(O):
    yield from shape_env(O, with_pack=True)


def build(rng, kind):
    """the circuit and the wires of interest"""
    from thfhe import circuits as CI
    enc = kind == "enc"
    cir = CI.Circuit()
    x = cir.inputs(10)
    g = [cir.gate(NAND if i & 1 else XOR, x[i], x[i + 1]) for i in range(4)]                 # wires 10 .. 13
    lut = cir.lut(cir.table(words(rng, N)), [x[4]], theta=4)                                  # wires 14 .. 17
    rows = lambda n: (words(rng, n, N), words(rng, n, N) if enc else None)
    b, a = rows(7)
    row0 = cir.lhe_table(b, a)
    lk = [cir.lhe_lookup(0, row0 + 1, 0, 2, theta=4), cir.lhe_lookup(1, row0 + 2, 2, 1, theta=2), cir.lhe_lookup(2, row0 + 5, 1, 0)]
    ga = cir.lhe_gather(2, x[0], 0, 1)
    gb = cir.lhe_gather(1, g[0], 0, 3)
    gc = cir.lhe_gather(3, x[2], 2, 2)
    gd = cir.lhe_gather(2, gb, 0, 1)          # candidates: the outputs of gb and gc
    fb, fa = rows(4)
    fin0 = cir.lhe_finals(fb, fa)
    one = (np.zeros((1, 1, 2), np.int32), np.array([16 * 0 + 2], np.int32), None, np.array([0], np.int32))   # bit 2 of its only set
    w1 = cir.lhe_wfa(one, [1], fin0 + 3, theta=2)
    w3 = cir.lhe_wfa((TRANS3, STEP3, None, START3), [0, 1], fin0, theta=2)
    assert gc == gb + 1
    return cir, dict(lookups=lk, gathers=[ga, gb, gc, gd], wfa1=w1, wfa3=w3, lut=lut)


_cache = {}


def case(env, shape, kind):
    """circuit, inputs, TGSW words per set, model wires int32[COUNT][n_wires][words]"""
    key = (shape, kind)
    if key not in _cache:
        p, K, orc, ck, pc, pk = env(shape)
        rng = np.random.default_rng(8100 + 10 * LHE_SHAPES.index(shape) + (kind == "enc"))
        cir, wires = build(rng, kind)
        x = words(rng, COUNT, cir.n_inputs, p.n + 1)
        sets = [words(rng, COUNT, d, 2 * p.l, 2, N) for d in SET_D]
        ref = np.stack(pmap(lambda q: DL.evaluate(orc, cir, x[q], [C[q] for C in sets], pk, p.ks_t, p.ks_basebit), range(COUNT)))
        _cache[key] = (cir, wires, x, sets, ref)
    return _cache[key]


class opened:
    """the TgswSets of a case"""
    def __init__(self, ck, sets, count=COUNT):
        self.ck, self.sets, self.count = ck, sets, count

    def __enter__(self):
        self.ts = [self.ck.tgsw_set(C[:self.count], C.shape[1]) for C in self.sets]
        return self.ts

    def __exit__(self, *exc):
        for t in self.ts:
            t.close()


def same(got, ref, what):
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.array_equal(got, ref), (what, differing(got, ref))


@pytest.mark.parametrize("kind", ["pub", "enc"])
@pytest.mark.parametrize("shape", LHE_SHAPES, ids=shape_id)
def test_every_wire_against_the_model_and_the_flat_calls(env, shape, kind):
    from thfhe import circuits as CI
    p, K, orc, ck, pc, pk = env(shape)
    cir, wires, x, sets, ref = case(env, shape, kind)
    with opened(ck, sets) as ts:
        st = {}
        got = CI.evaluate_batch(ck, cir, x, pack=pc, tgsw_sets=ts, stats=st)       # instances = the sets' count
        same(got, ref, "model")
        assert st["levels"] == 3 and st["rotations"] == 5 * COUNT                    # 4 gates + the LUT node; a leveled node counts no rotation
        for q in (0, COUNT - 1):
            same(CI.evaluate_levels(ck, cir, x[q], pack=pc, tgsw_sets=ts, instance=q), got[q], ("flat calls", q))
        same(CI.evaluate(ck, cir, x[0], pack=pc, tgsw_sets=ts), got[0], "one instance")
        pick = [wires["lookups"][0][3], wires["wfa3"][3], wires["gathers"][3], wires["lut"][2], wires["wfa1"][1]]   # LUT_OUT rows among them
        same(CI.evaluate_batch(ck, cir, x, out_wires=pick, pack=pc, tgsw_sets=ts), got[:, pick], "out_wires")


@pytest.mark.parametrize("shape", LHE_SHAPES, ids=shape_id)
def test_cut_groups_return_identical_words(env, shape):
    from thfhe import circuits as CI
    p, K, orc, ck, pc, pk = env(shape)
    cir, wires, x, sets, ref = case(env, shape, "enc")
    with opened(ck, sets) as ts:
        try:
            for cut in (1, 5):
                ck.set_dag_slice(cut)
                same(CI.evaluate_batch(ck, cir, x, pack=pc, tgsw_sets=ts), ref, ("dag slice", cut))
        finally:
            ck.set_dag_slice(28672)
        try:
            for cut in (16, 6):      # 16: a GATHER of 2^4 candidates holds one instance per slice; 6: a WFA of 3 states one, a LOOKUP of 2 workspace samples three
                ck.set_tree_slice(cut)
                same(CI.evaluate_batch(ck, cir, x, pack=pc, tgsw_sets=ts), ref, ("tree slice", cut))
        finally:
            ck.set_tree_slice(65536)


def test_without_leveled_nodes_the_entry_is_the_multi_value_one(env):
    p, K, orc, ck, pc, pk = env(LHE_SHAPES[0])
    rng = np.random.default_rng(8200)
    x = words(rng, 2, 4, p.n + 1)
    nodes = np.array([[NAND, 0, 1, -1, -1, -1], [XOR, 2, 4, -1, -1, -1], [11, 5, -1, -1, -1, -1]], np.int32)
    a, sa = ck.dag_run_lhe_batch(x, nodes)
    b, sb = ck.dag_run_mv_batch(x, nodes)
    same(a, b, "gates only")
    assert sa == sb


def test_the_checks_that_look_at_the_sets(env):
    import thfhe
    from thfhe import circuits as CI
    shape = LHE_SHAPES[0]
    p, K, orc, ck, pc, pk = env(shape)
    cir, wires, x, sets, ref = case(env, shape, "pub")
    other = env(LHE_SHAPES[1])[3]
    with opened(ck, sets) as ts, opened(ck, sets, 2) as short, opened(ck, [sets[0]] * 4) as wrong_d:
        with pytest.raises(thfhe.ThfheError, match="fewer samples"):
            CI.evaluate_batch(ck, cir, x, pack=pc, tgsw_sets=[short[0]] + ts[1:])
        with pytest.raises(thfhe.ThfheError, match="must equal the set's d"):
            CI.evaluate_batch(ck, cir, x, pack=pc, tgsw_sets=wrong_d)
        with pytest.raises(thfhe.ThfheError, match="another context"):
            CI.evaluate_batch(other, cir, words(np.random.default_rng(1), COUNT, cir.n_inputs, other.words), pack=pc, tgsw_sets=ts)
        with pytest.raises(thfhe.ThfheError, match="null ctx"):
            CI.evaluate_batch(ck, cir, x, pack=None, tgsw_sets=ts)     # a GATHER needs the packing context
        same(CI.evaluate_batch(ck, cir, x[:1], pack=pc, tgsw_sets=ts), ref[:1], "instances = 1")
        # step_bit against the spec's sets: set 1 of a one-set automaton; bit 2 of the 2-bit set 0; bit 3 of the 3-bit set 1
        for set_ids, sb in (([0], 16 * 1 + 0), ([0], 16 * 0 + 2), ([0, 1], 16 * 1 + 3), ([0, 1], -1)):
            bad = CI.Circuit()
            bad.inputs(1)
            bad.lhe_wfa((np.zeros((1, 1, 2), np.int32), np.array([sb], np.int32), None, np.array([0], np.int32)), set_ids,
                        bad.lhe_finals(np.zeros((1, N), np.int32)))
            with pytest.raises(thfhe.ThfheError, match="step_bit"):
                CI.evaluate_batch(ck, bad, x[:, :1], tgsw_sets=ts)


@pytest.mark.parametrize("op", [21, 22, 23], ids=["LOOKUP", "GATHER", "WFA"])
def test_the_gate_list_entries_refuse_the_three_opcodes(O, env, op):
    # thfhe_dag_run(_batch) and thfhe_mk_dag_run(_batch) look at their context before they plan, so only a live context shows that their classifiers
    # do not know opcodes 21 to 23; both contexts evaluate a gate afterwards
    import thfhe
    ck = env(LHE_SHAPES[0])[3]
    pm = O.make_params("MK2", n=64)
    sg = O.SIGMAS["MK2"]
    KM = O.MKKeys(pm, 5, sg["bk"], sg["ks"])
    mk = thfhe.MKCloudKey(thfhe.make_params(**pm.as_dict()), KM.bk, KM.ksk, device=0)
    try:
        rng = np.random.default_rng(8300 + op)
        for key in (ck, mk):
            x = words(rng, 3, key.words)
            bad = np.array([[NAND, 0, 1, -1], [op, -1, -1, -1]], np.int32)
            with pytest.raises(thfhe.ThfheError, match="error -1.*opcode not defined"):
                key.dag_run(x, bad)
            with pytest.raises(thfhe.ThfheError, match="error -1.*opcode not defined"):
                key.dag_run_batch(x[None], bad)
            vals, _ = key.dag_run(x, bad[:1])
            assert np.array_equal(vals[3], key.gates(NAND, x[0:1], x[1:2])[0])
    finally:
        mk.close()
