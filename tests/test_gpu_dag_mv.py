"""Multi-value nodes in the gate-DAG executor on the MI355X (pytest -m gpu): thfhe_dag_run_mv_batch word for word against the flat
public calls (mv_lut_bootstrap, tree_lut_bootstrap_mvk, PackBoxes + lut_bootstrap_enc) and the host-driven level loop (evaluate_levels), which
makes those calls level by level; instances against single runs; slices of one and of five nodes; the plan's figures; sbox_digits decrypting; and
thfhe_dag_run_tree_batch, now a wrapper of the same body, on a plan without the new nodes.  The gate-list entries (thfhe_dag_run(_batch), thfhe_mk_dag_run(_batch))
refuse the two opcodes with live contexts.  SK-128 at full size; word comparisons use random
words (a bootstrap is a deterministic function of its operands' words)."""
import numpy as np
import pytest

import lut_reference as R
from support import N, SIGMA, differing, sk128_cloud_key, sk128_pack, words

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ck(sk128):
    yield from sk128_cloud_key(sk128)


@pytest.fixture(scope="module")
def pack(sk128):
    yield from sk128_pack(sk128)


def run(ck, pc, cir, x):
    """the native executor on int32[Q][n_inputs][words] -> (every wire int32[Q][n_wires][words], stats)"""
    from thfhe import circuits as Cc
    st = {}
    return Cc.evaluate_batch(ck, cir, x, stats=st, pack=pc), st


def mixed_circuit(rng):
    """Level 1: a gate, a theta = 2 LUT node, a TREE node, three MV nodes on two specs (two tables of the first), a TREE_MV node.  Level 2: a SELECT fed
    by the first MV node's four wires, a TREE_MV node of the first one's group on level-1 outputs, a NOT."""
    from thfhe import NAND, NOT
    from thfhe import circuits as Cc
    c = Cc.Circuit()
    x0, x1, x2, x3 = c.inputs(4)
    t = dict(tab=words(rng, N), rows=words(rng, 2, N), base=words(rng, 2, N), wA=words(rng, 2, 4, 8), wB=words(rng, 5, 4),
             wT=words(rng, 2, 3, 4, 8), bias=int(rng.integers(-2**31, 2**31)))
    b0, b1 = c.mv_base(t["base"][0]), c.mv_base(t["base"][1])
    w = dict(g=c.gate(NAND, x0, x1), l=c.lut(c.table(t["tab"]), [x0], theta=2), t=c.tree(c.tree_rows(t["rows"]), [x1], [x2], 4, theta1=2))
    w["mvA"] = c.mv(b0, t["wA"][0], [x0, x1], weights=(2, -3), bias=t["bias"])
    w["mvB"] = c.mv(b1, t["wB"], [x3])
    w["mvA2"] = c.mv(b0, t["wA"][1], [x2, x3], weights=(2, -3), bias=t["bias"])
    w["tm"] = c.tree_mv(b0, t["wT"][0], [x0], [x1, x2], hi_weights=(1, 2))
    w["sel"] = c.select([w["g"]], w["mvA"][0], 4)
    w["tm2"] = c.tree_mv(b0, t["wT"][1], [w["l"][1]], [w["tm"][2], w["mvB"][4]], hi_weights=(1, 2))
    w["n"] = c.gate(NOT, w["tm"][0])
    return c, t, w


@pytest.mark.parametrize("instances", [1, 3])
def test_mixed_dag_equals_the_flat_calls(sk128, ck, pack, instances):
    from thfhe import circuits as Cc
    from thfhe import threshold as T
    pc, pk = pack
    rng = np.random.default_rng(6100)
    c, t, w = mixed_circuit(rng)
    assert c.has_mv_nodes() and len(c.mv_specs) == 3 and [len(s[6]) for s in c.mv_specs] == [2, 1, 2]
    x = words(rng, instances, 4, ck.words)
    got, st = run(ck, pc, c, x)
    col = lambda *ws: [np.ascontiguousarray(got[:, i]) for i in ws]
    # the nodes against their flat calls, directly
    mvA = ck.mv_lut_bootstrap(t["wA"], *col(0, 1), tv0=t["base"][0], weights=(2, -3), bias=t["bias"])
    assert w["mvA"] == list(range(w["mvA"][0], w["mvA"][0] + 4))
    assert np.array_equal(got[:, w["mvA"]], mvA)
    assert np.array_equal(got[:, w["mvB"]], ck.mv_lut_bootstrap(t["wB"], *col(3), tv0=t["base"][1]))
    mvA2 = ck.mv_lut_bootstrap(t["wA"], *col(2, 3), tv0=t["base"][0], weights=(2, -3), bias=t["bias"], table_index=np.ones(instances, np.int32))
    assert np.array_equal(got[:, w["mvA2"]], mvA2)
    tm = ck.tree_lut_bootstrap_mvk(pc, t["wT"][0], tuple(col(0)), tuple(col(1, 2)), tv0=t["base"][0], weights_hi=(1, 2))
    assert np.array_equal(got[:, w["tm"]], tm)
    tm2 = ck.tree_lut_bootstrap_mvk(pc, t["wT"], tuple(col(w["l"][1])), tuple(col(w["tm"][2], w["mvB"][4])), tv0=t["base"][0], weights_hi=(1, 2),
                                    table_index=np.ones(instances, np.int32))
    assert np.array_equal(got[:, w["tm2"]], tm2)
    # the SELECT takes the MV node's q = 4 consecutive wires as its candidates
    a, b = T.PackBoxes(pc, mvA.reshape(-1, ck.words), 4)
    assert np.array_equal(got[:, w["sel"]], ck.lut_bootstrap_enc(a, b, *col(w["g"]), lut_index=np.arange(instances))[:, 0])
    assert np.array_equal(got[:, w["n"]], (0 - got[:, w["tm"][0]].astype(np.int64)).astype(np.int32))
    # every wire against the level loop over the flat calls, and instances against single runs
    for q in range(instances):
        assert np.array_equal(got[q], Cc.evaluate_levels(ck, c, x[q], pack=pc)), q
        assert np.array_equal(got[q], Cc.evaluate(ck, c, x[q], pack=pc)), q
    # the plan: 2 levels; level 1 = gate, LUT, TREE (2), MV spec A, MV spec B, TREE_MV (2); level 2 = SELECT, TREE_MV (2); the NOT launches nothing it
    # counts.  Rotations: 1 + 1 + 3 + 3 + 4, then 1 + 4.
    assert (st["levels"], st["launches"], st["rotations"]) == (2, 11, 17 * instances)
    assert c.census()["rotations"] == 17 and c.census()["mvs"] == 3 and c.census()["tree_mvs"] == 2
    # slices of one node and of five nodes over all instances, the groups' starts and ends inside an instance
    for s in (1, 5):
        try:
            ck.set_dag_slice(s)
            assert np.array_equal(run(ck, pc, c, x)[0], got), s
        finally:
            ck.set_dag_slice(28672)
    try:   # tree_slice below q and k q: one node per slice
        ck.set_tree_slice(3)
        assert np.array_equal(run(ck, pc, c, x)[0], got)
    finally:
        ck.set_tree_slice(65536)


def test_sbox_digits_decrypts(sk128, ck, pack):
    # 8 of the 64 inputs of test_gpu_tree_mvk's decrypting case (the same table, keys and encryption seeds), as 8 instances of the one-node circuit
    from thfhe import circuits as Cc
    from thfhe import lut
    p, K, orc = sk128
    pc, pk = pack
    table = np.random.default_rng(5500).integers(0, 16, 64)
    hi, lo = np.repeat(np.arange(8), 8), np.tile(np.arange(8), 8)
    xh, xl = R.encrypt_words(K, lut.encode(hi, 8), SIGMA, 5501), R.encrypt_words(K, lut.encode(lo, 8), SIGMA, 5502)
    c = Cc.Circuit()
    wh, wl = c.inputs(2)
    bits = Cc.sbox_digits(c, wh, wl, table)
    pick = np.array([0, 9, 18, 27, 36, 45, 54, 63])
    x = np.stack([xh[pick], xl[pick]], axis=1)
    got, st = run(ck, pc, c, x)
    assert (st["levels"], st["launches"], st["rotations"]) == (1, 2, 5 * 8)
    dec = lut.decode(K.phases(got[:, bits].reshape(-1, p.n + 1)), 2).reshape(8, 4)
    assert np.array_equal((dec << np.arange(4)).sum(1), table[pick])
    _, w = lut.tree_mvk_factors([lambda h, l, j=j: (table[8 * h + l] >> j) & 1 for j in range(4)], 8, 8, 2)
    assert np.array_equal(got[:, bits], ck.tree_lut_bootstrap_mvk(pc, w, xl[pick], xh[pick], tv0=c.mv_bases[0]))


def test_tree_batch_without_the_new_nodes_is_unchanged(sk128, ck, pack):
    # a plan of the earlier kinds through thfhe_dag_run_tree_batch (the wrapper) and through thfhe_dag_run_mv_batch with its families absent: the
    # words of the flat calls, as before
    from thfhe import NAND
    from thfhe import circuits as Cc
    pc, pk = pack
    rng = np.random.default_rng(6300)
    c = Cc.Circuit()
    x0, x1, x2 = c.inputs(3)
    g = c.gate(NAND, x0, x1)
    l = c.lut(c.table(words(rng, N)), [x0, x2], weights=(1, -2), theta=4)
    tr = c.tree(c.tree_rows(words(rng, 4, N)), [x1], [x2], 4)
    e = c.lut_enc(c.enc_table(words(rng, N), words(rng, N)), [g], theta=2)
    s = c.select([tr], l[0], 4)
    assert c.has_tree_nodes() and not c.has_mv_nodes()
    x = words(rng, 2, 3, ck.words)
    got, st = run(ck, pc, c, x)
    for q in range(2):
        assert np.array_equal(got[q], Cc.evaluate_levels(ck, c, x[q], pack=pc)), q
    enc = c.enc_tables
    out, st2 = ck.dag_run_mv_batch(x, c.nodes(), c.specs, Cc._tables(ck, c), np.stack([t[0] for t in enc]), np.stack([t[1] for t in enc]), c.tree_specs,
                                   np.stack(c.tv1), pack=pc)
    assert np.array_equal(out, got[:, 3:]) and st2 == {k: st[k] for k in st2}
    assert s == c.n_wires() - 1 and e[1] == s - 1


@pytest.fixture(scope="module")
def small(O):
    """SK-128 at n = 16 and a packing key of random words (only words are compared); open_small: a fresh CloudKey and packing context on them"""
    p = O.make_params("SK-128", n=16)
    s = O.SIGMAS["SK-128"]
    K = O.SKKeys(p, 0x5EED0016, s["bk"], s["ks"])
    return p, K, words(np.random.default_rng(6500), p.n, p.ks_t, (1 << p.ks_basebit) - 1, 2, N)


def open_small(small):
    import thfhe
    from thfhe import threshold as T
    p, K, pk = small
    key = thfhe.CloudKey(thfhe.make_params(**p.as_dict()), K.bk, K.ksk, device=0)
    pc = T.PolyContext(0)
    pc.set_pack_key(pk, p.ks_t, p.ks_basebit)
    return key, pc


def test_tree_workspace_in_every_call_order(O, small):
    """The tree calls, the flat multi-value call and the grouped kinds of a DAG run size one set of grow-only buffers: a rows tree (R = 4 rotations
    per sample, one sample per slice), a k = 2 multi-value tree, a q = 3 multi-value call and a DAG run with a SELECT, a TREE feeding a TREE_MV and an
    MV group, on fresh contexts in three orders -- a call sized after a smaller one gives the words it gives first (the DAG run first: the packing
    reserve of a context nothing has sized), and the flat calls the words of the public calls they stand for."""
    import mv_lut_reference as MV
    from test_gpu_tree_lut import compose as rows_compose
    from test_gpu_tree_mvk import compose as mvk_compose
    from thfhe import circuits as Cc
    p, K, pk = small
    orc = O.Oracle(p, K.bk, K.ksk)
    rng = np.random.default_rng(6501)
    lo, hi = words(rng, 3, p.n + 1), words(rng, 3, p.n + 1)
    wlo, blo, whi, bhi = (3,), 1234567, (-5,), -7654321
    tv1, idx_a = words(rng, 2, 4, N), np.array([0, 1, 1], np.int32)                       # (a) p_hi = 8, theta = 2, two tables
    tv0, w, idx_b = words(rng, N), words(rng, 2, 2, 4, 2), np.array([1, 0, 1], np.int32)   # (b) p_hi = 4, p_lo = 2, k = 2, two tables
    w3 = words(rng, 3, 4)                                                                  # (c) p = 4, q = 3
    cir = Cc.Circuit()                                                                     # (d)
    a, b = cir.inputs(2)
    m = cir.mv(cir.mv_base(words(rng, N)), words(rng, 4, 4), [a], weights=wlo, bias=blo)
    cir.select([b], m[0], 4, weights=whi, bias=bhi)
    t = cir.tree(cir.tree_rows(words(rng, 2, N)), [a], [b], 4, lo_weights=wlo, hi_weights=whi, lo_bias=blo, hi_bias=bhi, theta1=2)
    cir.tree_mv(cir.mv_base(words(rng, N)), words(rng, 2, 4, 4), [t], [b], lo_weights=wlo, hi_weights=whi, lo_bias=blo, hi_bias=bhi)
    x = np.stack([lo[:2], hi[:2]])   # [instance][wire][words]

    def call_a(key, pc):
        key.set_tree_slice(8)   # one sample per slice
        try:
            return key.tree_lut_bootstrap(pc, tv1, lo, hi, p_hi=8, weights_lo=wlo, bias_lo=blo, theta=2, weights_hi=whi, bias_hi=bhi, table_index=idx_a)
        finally:
            key.set_tree_slice(65536)

    calls = dict(a=call_a,
                 b=lambda key, pc: key.tree_lut_bootstrap_mvk(pc, w, lo, hi, tv0=tv0, weights_lo=wlo, bias_lo=blo, weights_hi=whi, bias_hi=bhi, table_index=idx_b),
                 c=lambda key, pc: key.mv_lut_bootstrap(w3, lo, tv0=tv0, weights=wlo, bias=blo),
                 d=lambda key, pc: Cc.evaluate_batch(key, cir, x, pack=pc))
    first = None
    for order in ("abcd", "dcba", "bdac"):
        key, pc = open_small(small)
        try:
            got = {name: calls[name](key, pc) for name in order}
            if first is None:
                first = got
                assert got["a"].shape == (3, p.n + 1) and got["b"].shape == (3, 2, p.n + 1) and got["c"].shape == (3, 3, p.n + 1)
                assert got["d"].shape == (2, cir.n_wires(), p.n + 1) and cir.n_wires() == 2 + 4 + 1 + 1 + 2
                flat = rows_compose(key, pc, tv1, [lo], [hi], 8, 2, wlo, blo, whi, bhi, idx_a)
                assert np.array_equal(got["a"], flat), ("a", differing(got["a"], flat))
                flat = mvk_compose(key, pc, tv0, w, [lo], [hi], wlo, blo, whi, bhi, idx_b)
                assert np.array_equal(got["b"], flat), ("b", differing(got["b"], flat))
                flat = np.stack([MV.mv_lut(orc, [lo[g]], wlo, blo, tv0, w3) for g in range(3)])
                assert np.array_equal(got["c"], flat), ("c", differing(got["c"], flat))
            for name in order:
                assert np.array_equal(got[name], first[name]), (order, name, differing(got[name], first[name]))
        finally:
            key.close()
            pc.close()


def test_mv_and_tree_mv_groups_slice_by_their_own_rule(small):
    """An MV group of 5 nodes and a TREE_MV group (k = 2, q = 4) of 3 nodes, two instances: the words of the unsliced run with tree_slice = k q (one
    TREE_MV node and, q = 4, two MV nodes per slice) and with two nodes per slice of either group."""
    from thfhe import circuits as Cc
    p, K, pk = small
    rng = np.random.default_rng(6502)
    cir = Cc.Circuit()
    ins = cir.inputs(3)
    b0, wm, wt = cir.mv_base(words(rng, N)), words(rng, 2, 4, 4), words(rng, 2, 2, 4, 4)
    for j in range(5):
        cir.mv(b0, wm[j % 2], [ins[j % 3]], weights=(3,), bias=1234567)
    for j in range(3):
        cir.tree_mv(b0, wt[j % 2], [ins[j]], [ins[(j + 1) % 3]], hi_weights=(-5,))
    x = words(rng, 2, 3, p.n + 1)
    key, pc = open_small(small)
    try:
        st = {}
        ref = Cc.evaluate_batch(key, cir, x, stats=st, pack=pc)
        assert (st["levels"], st["launches"], st["rotations"]) == (1, 3, (5 + 3 * 3) * 2)   # launch groups: MV, the level 1 and the selections of TREE_MV
        for setter, value, default in ((key.set_tree_slice, 8, 65536), (key.set_dag_slice, 2, 28672)):
            setter(value)
            try:
                got = Cc.evaluate_batch(key, cir, x, pack=pc)
            finally:
                setter(default)
            assert np.array_equal(got, ref), (setter.__name__, differing(got, ref))
    finally:
        key.close()
        pc.close()


@pytest.mark.parametrize("op", [19, 20], ids=["MV", "TREE_MV"])
def test_the_gate_list_entries_refuse_the_two_opcodes(O, sk128, ck, op):
    # thfhe_dag_run(_batch) and thfhe_mk_dag_run(_batch) look at their context before they plan, so only a live context shows that their classifiers
    # do not know opcodes 19 and 20; both contexts evaluate a gate afterwards
    import thfhe
    pm = O.make_params("MK2", n=64)
    sg = O.SIGMAS["MK2"]
    KM = O.MKKeys(pm, 5, sg["bk"], sg["ks"])
    mk = thfhe.MKCloudKey(thfhe.make_params(**pm.as_dict()), KM.bk, KM.ksk, device=0)
    try:
        rng = np.random.default_rng(6400 + op)
        for key in (ck, mk):
            x = words(rng, 3, key.words)
            bad = np.array([[thfhe.NAND, 0, 1, -1], [op, 0, 1, 2 if op == 20 else -1]], np.int32)
            with pytest.raises(thfhe.ThfheError, match="error -1.*opcode not defined"):
                key.dag_run(x, bad)
            with pytest.raises(thfhe.ThfheError, match="error -1.*opcode not defined"):
                key.dag_run_batch(x[None], bad)
            vals, _ = key.dag_run(x, bad[:1])
            assert np.array_equal(vals[3], key.gates(thfhe.NAND, x[0:1], x[1:2])[0])
    finally:
        mk.close()
