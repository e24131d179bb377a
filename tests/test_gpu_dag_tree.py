"""Encrypted-table, select and tree nodes in the gate-DAG executor on the MI355X (pytest -m gpu): thfhe_dag_run_tree_batch word for
word against the flat public calls (lut_bootstrap_enc, PackBoxes + lut_bootstrap_enc, tree_lut_bootstrap), against the host-driven level loop
(evaluate_levels) and, on a pick of nodes, against the CPU model (tests/dag_tree_reference.py); instances against single runs; slices that start
and end inside an instance; tree_mul_digits on all 64 digit pairs; the context checks; the plan's figures; SK-80 and SK-lib.  SK-128 at full size
unless a test says otherwise; word comparisons use random words (a bootstrap is a deterministic function of its operands' words)."""
import numpy as np
import pytest

import dag_tree_reference as DT
import lut_reference as R
from support import N, SIGMA, SIGMA_BK, sk128_cloud_key, sk128_pack, words

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ck(sk128):
    yield from sk128_cloud_key(sk128)


@pytest.fixture(scope="module")
def pack(sk128):
    yield from sk128_pack(sk128)


def run(ck, pc, cir, x):
    """thfhe_dag_run_tree_batch on int32[Q][n_inputs][words] -> (every wire int32[Q][n_wires][words], stats)."""
    from thfhe import circuits as Cc
    st = {}
    return Cc.evaluate_batch(ck, cir, x, stats=st, pack=pc), st


def check_against_levels_and_single_runs(ck, pc, cir, x, got):
    from thfhe import circuits as Cc
    for q in range(x.shape[0]):
        assert np.array_equal(got[q], Cc.evaluate_levels(ck, cir, x[q], pack=pc)), q
    if x.shape[0] > 1:
        for q in (0, x.shape[0] - 1):
            assert np.array_equal(run(ck, pc, cir, x[q:q + 1])[0][0], got[q]), q


# ---- one kind per circuit, word for word against the flat call ----------------------------------------------------------------------------

@pytest.mark.parametrize("instances", [1, 5])
def test_lut_enc_nodes_alone(sk128, ck, instances):
    from thfhe import circuits as Cc
    rng = np.random.default_rng(100 + instances)
    c = Cc.Circuit()
    x0, x1, x2 = c.inputs(3)
    ea, eb = words(rng, 2, N), words(rng, 2, N)
    e = [c.enc_table(ea[i], eb[i]) for i in range(2)]
    b1 = int(rng.integers(-2**31, 2**31))
    o1 = c.lut_enc(e[0], [x0, x1], weights=(2, -3), bias=b1, theta=2)
    o2 = c.lut_enc(e[1], [x2], theta=4)
    o3 = c.lut_enc(e[1], [x0, x1, x2], weights=(1, 1, -5), theta=1)
    o4 = c.lut_enc(e[0], [x1], theta=4)
    x = words(rng, instances, 3, ck.words)
    got, st = run(ck, None, c, x)                       # no packing context needed
    flat = lambda i, ins, **kw: ck.lut_bootstrap_enc(ea[i:i + 1], eb[i:i + 1], *[x[:, w] for w in ins], **kw)
    assert np.array_equal(got[:, o1], flat(0, [x0, x1], weights=(2, -3), bias=b1, theta=2))
    assert np.array_equal(got[:, o2], flat(1, [x2], theta=4))
    assert np.array_equal(got[:, o3], flat(1, [x0, x1, x2], weights=(1, 1, -5)))
    assert np.array_equal(got[:, o4], flat(0, [x1], theta=4))
    assert (st["levels"], st["launches"], st["rotations"]) == (1, 3, 4 * instances)     # one group per theta
    check_against_levels_and_single_runs(ck, None, c, x, got)


@pytest.mark.parametrize("instances", [1, 5])
def test_select_nodes_alone(sk128, ck, pack, instances):
    from thfhe import circuits as Cc
    from thfhe import threshold as T
    pc, pk = pack
    rng = np.random.default_rng(110 + instances)
    c = Cc.Circuit()
    cand = c.inputs(8)
    i0, i1 = c.inputs(2)
    bias = int(rng.integers(-2**31, 2**31))
    s1 = c.select([i0], cand[0], 4)
    s2 = c.select([i0, i1], cand[2], 4, weights=(1, 2), bias=bias)
    s3 = c.select([i1], cand[0], 8)
    s4 = c.select([i1], cand[4], 4)                     # s1's group
    x = words(rng, instances, 10, ck.words)
    got, st = run(ck, pc, c, x)

    def flat(first, p, ins, **kw):
        a, b = T.PackBoxes(pc, x[:, first:first + p].reshape(-1, ck.words), p)
        return ck.lut_bootstrap_enc(a, b, *[x[:, w] for w in ins], lut_index=np.arange(instances), **kw)[:, 0]
    assert np.array_equal(got[:, s1], flat(0, 4, [i0]))
    assert np.array_equal(got[:, s2], flat(2, 4, [i0, i1], weights=(1, 2), bias=bias))
    assert np.array_equal(got[:, s3], flat(0, 8, [i1]))
    assert np.array_equal(got[:, s4], flat(4, 4, [i1]))
    assert (st["levels"], st["launches"], st["rotations"]) == (1, 3, 4 * instances)     # three trees[] entries
    check_against_levels_and_single_runs(ck, pc, c, x, got)


@pytest.mark.parametrize("instances", [1, 5])
def test_tree_nodes_alone(sk128, ck, pack, instances):
    from thfhe import circuits as Cc
    pc, pk = pack
    rng = np.random.default_rng(120 + instances)
    c = Cc.Circuit()
    x0, x1, x2 = c.inputs(3)
    rows = words(rng, 10, N)
    ra, rb, rc8 = c.tree_rows(rows[:2]), c.tree_rows(rows[2:6]), c.tree_rows(rows[6:10])
    b_lo, b_hi = (int(v) for v in rng.integers(-2**31, 2**31, 2))
    t1 = c.tree(ra, [x0], [x1], 4, theta1=2)
    t2 = c.tree(rb, [x0, x2], [x1], 4, lo_weights=(1, -2), lo_bias=b_lo, hi_bias=b_hi)
    t3 = c.tree(rc8, [x2], [x0, x1], 8, hi_weights=(3, 1), theta1=2)
    t4 = c.tree(ra, [x1], [x2], 4, theta1=2)            # t1's group
    x = words(rng, instances, 3, ck.words)
    got, st = run(ck, pc, c, x)
    col = lambda ws: tuple(x[:, w] for w in ws)
    assert np.array_equal(got[:, t1], ck.tree_lut_bootstrap(pc, rows[:2], col([x0]), col([x1]), p_hi=4, theta=2))
    assert np.array_equal(got[:, t2], ck.tree_lut_bootstrap(pc, rows[2:6], col([x0, x2]), col([x1]), p_hi=4, weights_lo=(1, -2), bias_lo=b_lo, bias_hi=b_hi))
    assert np.array_equal(got[:, t3], ck.tree_lut_bootstrap(pc, rows[6:10], col([x2]), col([x0, x1]), p_hi=8, theta=2, weights_hi=(3, 1)))
    assert np.array_equal(got[:, t4], ck.tree_lut_bootstrap(pc, rows[:2], col([x1]), col([x2]), p_hi=4, theta=2))
    # rotations R + 1 per tree: 3 + 5 + 5 + 3; two launches per trees[] entry
    assert (st["levels"], st["launches"], st["rotations"], st["widest_level"]) == (1, 6, 16 * instances, 2 * instances)
    check_against_levels_and_single_runs(ck, pc, c, x, got)


# ---- every kind on one level ------------------------------------------------------------------------------------------------------------------

def mixed_circuit(rng):
    """Level 1: gates, a many-LUT node, LUT_ENC nodes, trees at p = 4 with theta1 = 1, 2, 4 and p = 8 with theta1 = 2.  Level 2: gates, a MUX, a LUT
    node, a LUT_ENC node, SELECTs over the many-LUT node's and the LUT_ENC node's outputs and over level-1 trees, and trees on level-1 results."""
    import thfhe
    from thfhe import circuits as Cc
    c = Cc.Circuit()
    x = c.inputs(6)
    tabs = [c.table(words(rng, N)) for _ in range(2)]
    ea, eb = words(rng, 2, N), words(rng, 2, N)
    e = [c.enc_table(ea[i], eb[i]) for i in range(2)]
    rows = words(rng, 4 + 2 + 1 + 4, N)
    r41, r42, r44, r82 = c.tree_rows(rows[:4]), c.tree_rows(rows[4:6]), c.tree_rows(rows[6:7]), c.tree_rows(rows[7:11])
    w = {}
    # level 1
    w["g1"] = c.gate(thfhe.NAND, x[0], x[1])
    w["g2"] = c.gate(thfhe.XOR, x[2], x[3])
    w["many"] = c.lut(tabs[0], [x[0], x[4]], weights=(1, 3), theta=4)
    w["e1"] = c.lut_enc(e[0], [x[1], x[2]], weights=(1, -1), theta=2)
    w["e2"] = c.lut_enc(e[1], [x[5]], theta=1)
    w["t41"] = c.tree(r41, [x[0]], [x[1]], 4, theta1=1)
    w["t42"] = c.tree(r42, [x[2]], [x[3]], 4, theta1=2)
    w["t42b"] = c.tree(r42, [x[4]], [x[5]], 4, theta1=2)
    w["t44"] = c.tree(r44, [x[1], x[3]], [x[5]], 4, lo_weights=(1, 1), theta1=4)
    w["t82"] = c.tree(r82, [x[3]], [x[0], x[2]], 8, hi_weights=(1, 2), theta1=2)
    w["n"] = c.gate(thfhe.NOT, w["t42"])
    # level 2
    w["g3"] = c.gate(thfhe.AND, w["g1"], w["t41"])
    w["m"] = c.gate(thfhe.MUX, w["g2"], w["e2"][0], w["n"])
    w["l2"] = c.lut(tabs[1], [w["many"][1], w["t44"]], weights=(2, 1), theta=2)
    w["e3"] = c.lut_enc(e[1], [w["e1"][1]], bias=99, theta=2)
    w["s1"] = c.select([w["t42b"]], w["many"][0], 4)
    w["s2"] = c.select([x[0], w["g1"]], w["e1"][0], 2, weights=(1, 1))
    w["s3"] = c.select([x[5]], w["t41"], 4)                 # t41, t42, t42b, t44: consecutive wires
    w["t42c"] = c.tree(r42, [w["t82"]], [w["e2"][0]], 4, theta1=2)
    w["t82b"] = c.tree(r82, [w["many"][3]], [w["t41"], x[1]], 8, hi_weights=(1, 2), theta1=2)
    return c, w


def test_mixed_circuit_levels_model_and_stats(sk128, ck, pack):
    from thfhe import circuits as Cc
    p, K, orc = sk128
    pc, pk = pack
    rng = np.random.default_rng(130)
    c, w = mixed_circuit(rng)
    Q = 3
    x = words(rng, Q, 6, ck.words)
    got, st = run(ck, pc, c, x)
    check_against_levels_and_single_runs(ck, pc, c, x, got)
    cen = c.census()
    assert cen["depth"] == 2 and len(c.levels()) == 3
    # level 1: gates, LUT theta 4, LUT_ENC theta 1 and 2, TREE x 4 entries (two launches each); level 2: gates, MUX, LUT theta 2, LUT_ENC theta 2,
    # SELECT x 2 entries (s1 and s3 share one), TREE x 2 entries
    assert st["levels"] == cen["depth"] and st["rotations"] == cen["rotations"] * Q and st["launches"] == (1 + 1 + 2 + 8) + (1 + 1 + 1 + 1 + 2 + 4)
    assert cen["rotations"] == 2 + 1 + 2 + (5 + 3 + 3 + 2 + 5) + 1 + 2 + 1 + 1 + 3 + (3 + 5)
    # the CPU model on a pick of four nodes of instance 1 -- the p = 4 / theta1 = 2 tree on level-2 operands, the SELECT over the many-LUT outputs, the
    # SELECT over the LUT_ENC outputs and the level-2 LUT_ENC node -- with every row they read: 18 oracle rotations and one gate
    picks = [w["t42c"], w["s1"], w["s2"], w["e3"][0]]
    ref = DT.evaluate(orc, c, x[1], pk, p.ks_t, p.ks_basebit, only=[g - c.n_inputs for g in picks])
    done = [i for i in range(c.n_wires()) if ref[i].any() and i >= c.n_inputs]
    assert set(picks) <= set(done) and len(done) >= 10
    assert np.array_equal(got[1][done], ref[done])


def test_slices_inside_instances(sk128, ck, pack):
    # 5 instances; 7 nodes per slice cuts every group inside an instance; 12 candidates per slice = 3 SELECT / TREE nodes at p = 4, 1 at p = 8, so the
    # two-node p = 4 / theta1 = 2 group of level 1 (10 jobs) takes four slices
    pc, pk = pack
    rng = np.random.default_rng(140)
    c, w = mixed_circuit(rng)
    x = words(rng, 5, 6, ck.words)
    whole, st = run(ck, pc, c, x)
    try:
        ck.set_dag_slice(7)
        ck.set_tree_slice(12)
        sliced, st2 = run(ck, pc, c, x)
        ck.set_tree_slice(1)          # below p: one node per slice
        ck.set_dag_slice(3)
        single, _ = run(ck, pc, c, x[:2])
    finally:
        ck.set_dag_slice(28672)
        ck.set_tree_slice(65536)
    assert np.array_equal(sliced, whole) and np.array_equal(single, whole[:2]) and st2 == st


# ---- a circuit that decrypts ------------------------------------------------------------------------------------------------------------------

def test_tree_mul_digits_all_pairs(sk128, ck, pack):
    from thfhe import circuits as Cc, lut
    p, K, orc = sk128
    pc, pk = pack
    c = Cc.Circuit()
    a, b = c.inputs(2)
    lo, hi = Cc.tree_mul_digits(c, a, b)
    A, B = np.repeat(np.arange(8), 8), np.tile(np.arange(8), 8)
    x = np.stack([R.encrypt_words(K, lut.encode(A, 8), SIGMA, 3000), R.encrypt_words(K, lut.encode(B, 8), SIGMA, 3001)], axis=1)
    got, st = run(ck, pc, c, x)
    assert st == dict(c.census(), levels=1, launches=2, rotations=640, widest_level=128, instances=64)
    assert np.array_equal(lut.decode(K.phases(got[:, lo]), 8), (A * B) % 8)
    assert np.array_equal(lut.decode(K.phases(got[:, hi]), 8), (A * B) // 8)
    for q in range(64):
        want = lut.decode(Cc.simulate(c, lut.encode([A[q], B[q]], 8)), 8)
        assert (want[lo], want[hi]) == ((A[q] * B[q]) % 8, (A[q] * B[q]) // 8)
        assert np.array_equal(got[q], Cc.evaluate_levels(ck, c, x[q], pack=pc)), q


# ---- context checks ---------------------------------------------------------------------------------------------------------------------------

def test_context_checks(sk128, ck, pack):
    import thfhe
    from thfhe import circuits as Cc, keygen
    from thfhe import threshold as T
    p, K, orc = sk128
    pc, pk = pack
    rng = np.random.default_rng(150)
    c = Cc.Circuit()
    x0, x1 = c.inputs(2)
    t = c.tree(c.tree_rows(words(rng, 4, N)), [x0], [x1], 4)
    s = Cc.Circuit()
    s.select([s.inputs(3)[2]], 0, 2)
    x = words(rng, 2, 2, ck.words)
    want, _ = run(ck, pc, c, x)
    for cir, xin in ((c, x), (s, words(rng, 1, 3, ck.words))):
        with pytest.raises(thfhe.ThfheError, match="error -1.*null ctx"):
            run(ck, None, cir, xin)
        bare = T.PolyContext(0)
        with pytest.raises(thfhe.ThfheError, match="error -1.*no packing key"):
            run(ck, bare, cir, xin)
        bare.set_pack_key(keygen.gen_pack_key(rng, K.lwe_key[:10], K.rlwe_key[0], 8, 2, SIGMA_BK), 8, 2)
        with pytest.raises(thfhe.ThfheError, match="error -1.*dimension"):
            run(ck, bare, cir, xin)
        bare.close()
    if thfhe.lib().thfhe_device_count() > 1:   # a packing context on another device
        other = T.PolyContext(1)
        other.set_pack_key(pk, p.ks_t, p.ks_basebit)
        with pytest.raises(thfhe.ThfheError, match="error -1.*same device"):
            run(ck, other, c, x)
        other.close()
    # a plan with only LUT_ENC nodes takes no packing context, and a bare one is not looked at
    e = Cc.Circuit()
    e.lut_enc(e.enc_table(words(rng, N), words(rng, N)), [e.inputs(1)[0]], theta=2)
    xe = words(rng, 2, 1, ck.words)
    bare = T.PolyContext(0)
    assert np.array_equal(run(ck, None, e, xe)[0], run(ck, bare, e, xe)[0])
    bare.close()
    # host rejections leave the context usable; zero instances is a valid call
    with pytest.raises(thfhe.ThfheError, match="error -1.*row0"):
        ck.dag_run_tree_batch(x, [[thfhe.TREE, 0, 1, -1, 0, 1]], trees=c.tree_specs, tv1=np.stack(c.tv1), pack=pc)
    assert run(ck, pc, c, x[:0])[0].shape == (0, 3, ck.words)
    assert np.array_equal(run(ck, pc, c, x)[0], want)
    # the gate-only entries still refuse the three opcodes (they look at the context first, so this needs one)
    for row in ([thfhe.LUT_ENC, 0, -1, -1], [thfhe.SELECT, 0, -1, -1], [thfhe.TREE, 0, 1, -1]):
        with pytest.raises(thfhe.ThfheError, match="error -1.*opcode"):
            ck.dag_run_batch(x, [[thfhe.NAND, 0, 1, -1], row])


# ---- named sets -------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["SK-80", "SK-lib"])
def test_named_sets_tree_and_select(O, name):
    # one TREE (p = 4, theta1 = 2) and one SELECT (p = 4) over four fresh digits, keys as tests/test_gpu_lut_named_sets.py builds them; words against
    # the flat calls, decrypt-exact at p = 4 (the modulus at which that file's tree case, with key-switched candidates, decrypts on both sets)
    import thfhe
    from thfhe import circuits as Cc, keygen, lut
    from thfhe import threshold as T
    sig, p = O.SIGMAS[name], O.make_params(name)
    K = O.SKKeys(p, 0x5EED0000 + p.n, sig["bk"], sig["ks"])
    pk = keygen.gen_pack_key(np.random.default_rng(0x7EE0000 + p.n), K.lwe_key, K.rlwe_key[0], p.ks_t, p.ks_basebit, sig["bk"])
    key = thfhe.CloudKey(thfhe.make_params(name), K.bk, K.ksk, device=0)
    pc = T.PolyContext(0)
    try:
        pc.set_pack_key(pk, p.ks_t, p.ks_basebit)
        rng = np.random.default_rng(160 + p.n)
        F = rng.integers(0, 4, (4, 4))
        rows = lut.tree_test_vectors(lambda h, l: F[h, l], 4, 4, 4, theta=2)
        c = Cc.Circuit()
        cand = c.inputs(4)
        lo_w, hi_w = c.inputs(2)
        t = c.tree(c.tree_rows(rows), [lo_w], [hi_w], 4, theta1=2)
        s = c.select([hi_w], cand[0], 4)
        Q = 9
        V, LO, HI = rng.integers(0, 4, (Q, 4)), rng.integers(0, 4, Q), rng.integers(0, 4, Q)
        m = np.concatenate([V, LO[:, None], HI[:, None]], axis=1)
        x = R.encrypt_words(K, lut.encode(m.reshape(-1), 4), sig["lwe"], 3100).reshape(Q, 6, p.n + 1)
        got = Cc.evaluate_batch(key, c, x, pack=pc)
        assert np.array_equal(got[:, t], key.tree_lut_bootstrap(pc, rows, x[:, lo_w], x[:, hi_w], p_hi=4, theta=2))
        a, b = T.PackBoxes(pc, x[:, :4].reshape(-1, p.n + 1), 4)
        assert np.array_equal(got[:, s], key.lut_bootstrap_enc(a, b, x[:, hi_w], lut_index=np.arange(Q))[:, 0])
        assert np.array_equal(lut.decode(K.phases(got[:, t]), 4), F[HI, LO])
        assert np.array_equal(lut.decode(K.phases(got[:, s]), 4), V[np.arange(Q), HI])
    finally:
        key.close()
        pc.close()
