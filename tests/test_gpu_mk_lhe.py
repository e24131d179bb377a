"""Leveled CMux and table lookup on the 64-bit ring of degree 2048 on the device: thfhe_mk_lhe_cmux and
thfhe_mk_lhe_lookup(_wo_keyswitch) against tests/mk_lhe_reference.py, word for word with no tolerance.  One context with n = 8 serves every case;
random int64 words serve as the sets wherever words are compared (a set need not be a valid encryption), and one real-key case decodes."""
import numpy as np
import pytest

import mk_lhe_cases as CS
import mk_lhe_reference as M
from support import differing

pytestmark = pytest.mark.gpu
N, L, BGBIT = CS.N, CS.L, CS.BGBIT


@pytest.fixture(scope="module")
def env():
    import thfhe
    p, K, orc = CS.keys()
    ck = thfhe.MKCloudKey(thfhe.make_params(**CS.KW), K.bk, K.ksk, device=0)
    yield K, orc, ck
    ck.close()


def ks(orc, recs):
    return np.stack([orc.keyswitch(r) for r in recs.reshape(-1, N + 1)]).reshape(recs.shape[:-1] + (-1,))


def test_cmux_every_bit(env):
    K, orc, ck = env
    d, count = 3, 3
    rng = np.random.default_rng(41)
    w = CS.words64(rng, count, d, 4, L, N)
    S = CS.model_set(w, d)
    d1, d0 = CS.words64(rng, count, 2, N), CS.words64(rng, count, 2, N)
    with ck.tgsw_set(w, d) as ts:
        assert (ts.count, ts.d) == (count, d)
        for bit in range(d):
            got_a, got_b = ck.lhe_cmux(ts, bit, d1[:, 0], d1[:, 1], d0[:, 0], d0[:, 1])
            want = np.stack([M.cmux(S, s, bit, d1[s], d0[s]) for s in range(count)])
            assert np.array_equal(got_a, want[:, 0]) and np.array_equal(got_b, want[:, 1]), (bit, differing(got_b, want[:, 1]))
        # fewer samples than the set holds: its first ones
        got_a, got_b = ck.lhe_cmux(ts, 1, d1[:2, 0], d1[:2, 1], d0[:2, 0], d0[:2, 1])
        assert np.array_equal(got_b, np.stack([M.cmux(S, s, 1, d1[s], d0[s])[1] for s in range(2)]))


@pytest.mark.parametrize("d_tree,d_rot", CS.LOOKUPS, ids=lambda v: str(v))
def test_lookup_words(env, d_tree, d_rot):
    """Public and encrypted tables, two tables with a table_index, first = 1, every theta the box allows; before and after the key switch."""
    K, orc, ck = env
    case = CS.word_case(d_tree, d_rot)
    count, idx = 3, np.array([1, 0, 1], np.int32)
    with ck.tgsw_set(case["words"], case["d"]) as ts:
        for theta in CS.thetas(d_rot):
            # a public table, every sample on table 0
            got = ck.lhe_lookup_wo_keyswitch(ts, case["tab_b"][0], d_tree=d_tree, d_rot=d_rot, theta=theta)
            want = np.stack([CS.records(case["acc"](s, 0, False), theta) for s in range(count)])
            assert np.array_equal(got, want), ("public", theta, differing(got, want))
            # encrypted tables, two of them behind an index
            got = ck.lhe_lookup_wo_keyswitch(ts, case["tab_b"], d_tree=d_tree, d_rot=d_rot, theta=theta, tab_a=case["tab_a"], table_index=idx)
            want = np.stack([CS.records(case["acc"](s, int(idx[s]), True), theta) for s in range(count)])
            assert np.array_equal(got, want), ("enc", theta, differing(got, want))
            # from the second sample on, public tables behind an index, through the context's key switch
            got = ck.lhe_lookup(ts, case["tab_b"], d_tree=d_tree, d_rot=d_rot, theta=theta, table_index=idx[1:], first=1)
            want = ks(orc, np.stack([CS.records(case["acc"](s, int(idx[s]), False), theta) for s in (1, 2)]))
            assert got.shape == (2, theta, CS.KW["n"] + 1) and np.array_equal(got, want), ("first", theta, differing(got, want))
        assert ck.lhe_lookup(ts, case["tab_b"][0], d_tree=d_tree, d_rot=d_rot, first=3).shape == (0, 1, CS.KW["n"] + 1)   # count 0


def test_lookup_6_10(env):
    K, orc, ck = env
    case = CS.word_case(6, 10, count=1, n_tables=1)
    with ck.tgsw_set(case["words"], 16) as ts:
        got = ck.lhe_lookup_wo_keyswitch(ts, case["tab_b"], d_tree=6, d_rot=10, theta=2, tab_a=case["tab_a"])
        want = CS.records(case["acc"](0, 0, True), 2)[None]
        assert np.array_equal(got, want), differing(got, want)
        got = ck.lhe_lookup(ts, case["tab_b"], d_tree=6, d_rot=10)
        want = ks(orc, CS.records(case["acc"](0, 0, False), 1)[None])
        assert np.array_equal(got, want), differing(got, want)


def test_slices_cut_between_samples(env):
    """tree_slice = 4 candidates: (2, 1) has a workspace of two accumulators per sample, so three samples run as slices of 2 + 1."""
    K, orc, ck = env
    case = CS.word_case(2, 1)
    idx = np.array([1, 0, 1], np.int32)
    want = np.stack([CS.records(case["acc"](s, int(idx[s]), True), 2) for s in range(3)])
    ck.set_tree_slice(4)
    try:
        with ck.tgsw_set(case["words"], 3) as ts:
            got = ck.lhe_lookup_wo_keyswitch(ts, case["tab_b"], d_tree=2, d_rot=1, theta=2, tab_a=case["tab_a"], table_index=idx)
            assert np.array_equal(got, want), differing(got, want)
            ck.set_tree_slice(1)   # one sample per slice
            got = ck.lhe_lookup(ts, case["tab_b"], d_tree=2, d_rot=1, theta=2, tab_a=case["tab_a"], table_index=idx)
            assert np.array_equal(got, ks(orc, want))
    finally:
        ck.set_tree_slice(16384)


def test_real_keys_decode(env):
    """table[address] for all 8 addresses of a (1, 2) lookup on an encrypted table, decoded after the key switch; the words are the model's."""
    K, orc, ck = env
    values, w, ta, tb, tab = CS.real_case(1, 2)
    S = CS.model_set(w, 3)
    with ck.tgsw_set(w, 3) as ts:
        got = ck.lhe_lookup(ts, tb, d_tree=1, d_rot=2, tab_a=ta)
        assert CS.decode32(K.phase(got[:, 0])).tolist() == values.tolist()
        want = np.stack([M.lookup(S, orc, s, 1, 2, 1, ta, tb) for s in range(8)])
        assert np.array_equal(got, want), differing(got, want)
        pub = ck.lhe_lookup_wo_keyswitch(ts, tab, d_tree=1, d_rot=2)
        assert CS.decode32(K.ring_phase(pub[:, 0])).tolist() == values.tolist()


def test_sets_come_and_go_between_gates(env):
    """create -> lookup -> destroy -> create on one context, a NAND batch in between: the same words every time."""
    import thfhe
    K, orc, ck = env
    case = CS.word_case(1, 2)
    a, b = np.array([0, 1, 0, 1]), np.array([0, 0, 1, 1])
    xa, xb = K.encrypt(a, 21), K.encrypt(b, 22)
    look = lambda ts: ck.lhe_lookup(ts, case["tab_b"], d_tree=1, d_rot=2, theta=4, tab_a=case["tab_a"], table_index=np.array([0, 1, 1], np.int32))
    ts = ck.tgsw_set(case["words"], 3)
    first = look(ts)
    nand = ck.gates(thfhe.NAND, xa, xb)
    assert K.decrypt(nand).tolist() == [True, True, True, False]
    assert np.array_equal(look(ts), first)
    ts.close()
    assert np.array_equal(ck.gates(thfhe.NAND, xa, xb), nand)
    with ck.tgsw_set(case["words"], 3) as ts2:
        assert np.array_equal(look(ts2), first)
    want = ks(orc, np.stack([CS.records(case["acc"](s, t, True), 4) for s, t in enumerate((0, 1, 1))]))
    assert np.array_equal(first, want)


def test_refusals_that_need_a_context(env):
    import thfhe
    K, orc, ck = env
    case = CS.word_case(1, 2)
    rng = np.random.default_rng(43)
    other = thfhe.MKCloudKey(thfhe.make_params(**CS.KW), K.bk, K.ksk, device=0)
    try:
        with ck.tgsw_set(case["words"], 3) as ts:
            with pytest.raises(thfhe.ThfheError, match="another context"):
                other.lhe_lookup(ts, case["tab_b"][0], d_tree=1, d_rot=2)
            d = CS.words64(rng, 3, N)
            with pytest.raises(thfhe.ThfheError, match="another context"):
                other.lhe_cmux(ts, 0, d, d, d, d)
            with pytest.raises(thfhe.ThfheError, match="d_tree \\+ d_rot"):
                ck.lhe_lookup(ts, case["tab_b"][0], d_tree=0, d_rot=2)
            with pytest.raises(thfhe.ThfheError, match="not all in the set"):
                ck.lhe_lookup(ts, case["tab_b"][0], d_tree=1, d_rot=2, first=2, count=2)
            with pytest.raises(thfhe.ThfheError, match="bit must be"):
                ck.lhe_cmux(ts, 3, d, d, d, d)
    finally:
        other.close()
    for kw, what in ((dict(l=2, Bgbit=7), "batched rotation path"), (dict(parties=2), "parties = 1"), (dict(N=1024, l=2, Bgbit=7), "N = 2048")):
        p = thfhe.make_params(**dict(CS.KW, n=2, **kw))
        bk = CS.words64(rng, p.parties, p.n, 4, p.l, p.N)
        ksk = np.zeros((p.parties, p.N, p.ks_t, (1 << p.ks_basebit) - 1, p.n + 1), np.int32)
        c2 = thfhe.MKCloudKey(p, bk, ksk, device=0)
        try:
            with pytest.raises(thfhe.ThfheError, match=what):
                c2.tgsw_set(CS.words64(rng, 1, 4, p.l, p.N), 1)
        finally:
            c2.close()
