"""The multi-value two-digit tree on the 3-gen multi-key engine on the MI355X (pytest -m gpu):
thfhe_mk_tree_lut_bootstrap_mvk word for word against the three flat calls it stands for (thfhe_mk_mv_lut_bootstrap_wo_keyswitch ->
thfhe_mk_pack_boxes -> thfhe_mk_lut_bootstrap_enc) and against the model composed from the CPU oracle's pieces (tests/mk_tree_mv_reference.py), at
every ring degree, whole and one sample per slice, on packing keys of random words; k = 1 against tree_lut_bootstrap_mv; the refused calls; and one
full-size case on MK4 with a generated packing key, fresh inputs and every (hi, lo) of two bit functions decrypted and fed to the gates.

The model's packing sums cost (non-zero digits) x 2N words per candidate, so on the larger rings the model is asked for every sample only where a
sample has few candidates, and for one sample (of the second table) otherwise; the flat calls are compared on every sample of every shape."""
import ctypes as C
import time

import numpy as np
import pytest

import mk_lut_reference as R
import mk_pack_reference as MP
import mk_tree_mv_reference as TM
from support import differing, pmap
from test_gpu_mk_dag_tree import BASEBIT, T_PK
from test_gpu_mk_tree import _flat as _flat_rows

pytestmark = pytest.mark.gpu

# section 4.19's measured figures for MK4, torus units: the rotation's own noise and the multi-key key switch's
SIGMA_BR_MK4, SIGMA_KS_MK4 = 2.4e-3, 2.1e-2
SHAPES = ((4, 4, 1), (2, 8, 3), (8, 4, 2), (64, 2, 1), (4, 2, 16))   # (p_hi, p_lo, k)


def _keys(O, name, seed, **over):
    import thfhe
    p = O.make_params(name, **over)
    s = O.SIGMAS[name]
    K = O.MKKeys(p, seed, s["bk"], s["ks"])
    ck = thfhe.MKCloudKey(thfhe.make_params(**p.as_dict()), K.bk, K.ksk, device=0)
    return p, K, ck


def _flat(ck, tv0, w, lo, hi, wlo, blo, whi, bhi, idx, ob):
    """the three flat calls in a row; w int32[n_tables][k][p_hi][p_lo]"""
    n_tables, k, p_hi, p_lo = w.shape
    count = lo.shape[0]
    cand = ck.mv_lut_bootstrap_wo_keyswitch(w.reshape(n_tables, k * p_hi, p_lo), lo, tv0=tv0, weights=wlo, bias=blo, table_index=idx, out_bias=ob)
    ta, tb = ck.pack_boxes(cand.reshape(count * k * p_hi, -1), p_hi)
    out = ck.lut_bootstrap_enc(ta, tb, np.repeat(hi, k, axis=0), weights=whi, bias=bhi, lut_index=np.arange(count * k))
    return out[:, 0].reshape(count, k, -1)


@pytest.mark.parametrize("name,over,digits", [
    ("MK2", dict(n=30), (2, 1)),
    ("MK4-N2048", dict(n=10, parties=2), (1, 2)),
    ("MK64-fft", dict(n=4, parties=2), (1, 1)),
])
def test_tree_equals_the_flat_calls_and_the_model(O, name, over, digits):
    from thfhe import lut
    p, K, ck = _keys(O, name, 53, **over)
    try:
        orc = O.MKOracle(p, K.bk, K.ksk)
        rng = np.random.default_rng(p.N + 3)
        t, basebit = digits
        pk = rng.integers(-2**63, 2**63, (p.N, t, (1 << basebit) - 1, 2, p.N), dtype=np.int64)
        ck.pack_key_set(pk, t, basebit)
        ck.set_profiling(True)
        count = 5
        for p_hi, p_lo, k in SHAPES:
            tag = (name, p_hi, p_lo, k)
            tabs = rng.integers(0, 2, (2, k, p_hi, p_lo))
            parts = [lut.tree_mvk_factors([lambda h, l, T=T: T[h, l] for T in tab], p_hi, p_lo, 2, N=p.N, torus_bits=64) for tab in tabs]
            tv0, w = parts[0][0], np.stack([f for _, f in parts])
            lo = R.encrypt_words(K, rng.integers(-2**31, 2**31, count), O.SIGMAS[name]["lwe"], 50 + p_hi)
            hi = R.encrypt_words(K, rng.integers(-2**31, 2**31, count), O.SIGMAS[name]["lwe"], 60 + p_hi)
            idx = np.array([0, 1, 1, 0, 1], np.int32)
            wlo, blo, whi, bhi = (3,), int(rng.integers(-2**31, 2**31)), (-5,), int(rng.integers(-2**31, 2**31))
            ob = int(rng.integers(-2**63, 2**63))
            kw = dict(tv0=tv0, weights_lo=wlo, bias_lo=blo, weights_hi=whi, bias_hi=bhi, table_index=idx, out_bias=ob)
            got = ck.tree_lut_bootstrap_mvk(w, lo, hi, **kw)
            assert got.shape == (count, k, p.parties * p.n + 1)
            ms = ck.last_timings()
            assert all(np.isfinite(v) and v >= 0 for v in ms.values()) and len(ms) == 4
            flat = _flat(ck, tv0, w, lo, hi, wlo, blo, whi, bhi, idx, ob)
            assert np.array_equal(got, flat), (tag, differing(got, flat))
            samples = range(count) if k * p_hi * (p.N // 1024)**2 <= 64 else [1]
            ref = pmap(lambda g: TM.tree_mvk(orc, pk, t, basebit, tv0, w[idx[g]], [lo[g]], [hi[g]], wlo, blo, whi, bhi, ob), samples)
            for g, r in zip(samples, ref):
                assert np.array_equal(got[g], r), (tag, g, differing(got[g], r))
            ck.set_tree_slice(k * p_hi)       # one sample per slice
            try:
                sliced = ck.tree_lut_bootstrap_mvk(w, lo, hi, **kw)
            finally:
                ck.set_tree_slice(16384)
            assert np.array_equal(sliced, got), (tag, "sliced")
            # no table_index: table 0 for every sample
            zero = ck.tree_lut_bootstrap_mvk(w[:1], lo, hi, **{**kw, "table_index": None})
            assert np.array_equal(zero, _flat(ck, tv0, w, lo, hi, wlo, blo, whi, bhi, np.zeros(count, np.int32), ob)), (tag, "table 0")
            if k == 1:
                one = ck.tree_lut_bootstrap_mv(w[:, 0], lo, hi, **kw)
                assert one.shape == (count, p.parties * p.n + 1) and np.array_equal(one, got[:, 0]), (tag, "mv")
    finally:
        ck.close()


def test_both_packing_kernels_give_the_trees_words(O):
    # 5 samples x 64 candidates = 320 records per slice: the tree through the wide rows kernel and through the direct one
    from thfhe import lut
    p, K, ck = _keys(O, "MK2", 53, n=30)
    try:
        rng = np.random.default_rng(9)
        pk = rng.integers(-2**63, 2**63, (p.N, 3, 3, 2, p.N), dtype=np.int64)
        ck.pack_key_set(pk, 3, 2)
        tabs = rng.integers(0, 2, (16, 4, 2))
        tv0, w = lut.tree_mvk_factors([lambda h, l, T=T: T[h, l] for T in tabs], 4, 2, 2, N=p.N, torus_bits=64)
        lo = R.encrypt_words(K, rng.integers(-2**31, 2**31, 5), O.SIGMAS["MK2"]["lwe"], 51)
        hi = R.encrypt_words(K, rng.integers(-2**31, 2**31, 5), O.SIGMAS["MK2"]["lwe"], 61)
        outs = {}
        for thr, kernel in ((1, "mk_pack_rows_wide_kernel"), (0, "mk_pack_rows_kernel")):
            ck.set_pack_wide_threshold(thr)
            assert ck.pack_kernel_name(5 * 64) == kernel
            outs[thr] = ck.tree_lut_bootstrap_mvk(w, lo, hi, tv0=tv0)
        assert np.array_equal(outs[0], outs[1]), differing(outs[0], outs[1])
    finally:
        ck.close()


def test_refused_calls_leave_the_context_usable(O):
    import thfhe
    from thfhe import lut
    p, K, ck = _keys(O, "MK2", 53, n=30)
    try:
        rng = np.random.default_rng(5)
        x = R.encrypt_words(K, rng.integers(-2**31, 2**31, 2), O.SIGMAS["MK2"]["lwe"], 70)
        fs = [lambda h, l: h ^ l, lambda h, l: h & l]
        tv0, w = lut.tree_mvk_factors(fs, 4, 4, 2, N=p.N, torus_bits=64)
        with pytest.raises(thfhe.ThfheError, match="no packing key"):
            ck.tree_lut_bootstrap_mvk(w, x, x, tv0=tv0)
        small = rng.integers(-2**63, 2**63, (p.parties * p.n, 2, 3, 2, p.N), dtype=np.int64)
        ck.pack_key_set(small, 2, 2)
        with pytest.raises(thfhe.ThfheError, match="D = N"):
            ck.tree_lut_bootstrap_mvk(w, x, x, tv0=tv0)
        pk = rng.integers(-2**63, 2**63, (p.N, 2, 3, 2, p.N), dtype=np.int64)
        ck.pack_key_set(pk, 2, 2)
        with pytest.raises(thfhe.ThfheError, match="k p_hi"):                 # k p_hi = 128
            ck.tree_lut_bootstrap_mvk(np.zeros((2, 64, 2), np.int32), x, x, tv0=tv0)
        with pytest.raises(thfhe.ThfheError, match="p_hi"):
            ck.tree_lut_bootstrap_mvk(np.zeros((2, 3, 4), np.int32), x, x, tv0=tv0)
        with pytest.raises(thfhe.ThfheError, match="table_index"):
            ck.tree_lut_bootstrap_mvk(w[None], x, x, tv0=tv0, table_index=[0, 1])
        # theta = 2 on either level: the Python layer always says 1, so the entry itself is asked
        i32p, i64p = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
        out = np.zeros((2, 2, ck.words), np.int32)
        for lo_theta, hi_theta in ((2, 1), (1, 2)):
            sl = thfhe.LutSpec(1, (C.c_int32 * 3)(1, 0, 0), 0, lo_theta)
            sh = thfhe.LutSpec(1, (C.c_int32 * 3)(1, 0, 0), 0, hi_theta)
            rc = thfhe.lib().thfhe_mk_tree_lut_bootstrap_mvk(ck.h, C.byref(sl), C.byref(sh), 4, 4, 2, tv0.ctypes.data_as(i64p), w.ctypes.data_as(i32p), 1, None, 0,
                                                              x.ctypes.data_as(i32p), None, None, x.ctypes.data_as(i32p), None, None, out.ctypes.data_as(i32p), 2)
            assert rc == -1 and b"theta must be 1" in thfhe.lib().thfhe_last_error()
        assert ck.tree_lut_bootstrap_mvk(w, x[:0], x[:0], tv0=tv0).shape == (0, 2, p.parties * p.n + 1)
        got = ck.tree_lut_bootstrap_mvk(w, x, x, tv0=tv0)
        assert np.array_equal(got, _flat(ck, tv0, w[None], x, x, (1,), 0, (1,), 0, np.zeros(2, np.int32), 0))
    finally:
        ck.close()


def test_tree_workspace_in_every_call_order(O):
    """The tree calls share one grow-only workspace rule: a rows tree (R = 4 rotations per sample, one sample per slice), a k = 2 multi-value tree
    and a gate-DAG run with a TREE and a TREE_MV group, on fresh contexts in three orders -- a call sized after a smaller one gives the words it
    gives first, and the flat trees the words of the flat calls they stand for."""
    import thfhe
    from thfhe import circuits as CIR, lut
    p = O.make_params("MK2", n=30)
    s = O.SIGMAS["MK2"]
    K = O.MKKeys(p, 53, s["bk"], s["ks"])
    rng = np.random.default_rng(0x5EED0071)
    pk = rng.integers(-2**63, 2**63, (p.N, T_PK, (1 << BASEBIT) - 1, 2, p.N), dtype=np.int64)
    lo = R.encrypt_words(K, rng.integers(-2**31, 2**31, 3), s["lwe"], 71)
    hi = R.encrypt_words(K, rng.integers(-2**31, 2**31, 3), s["lwe"], 72)
    wlo, blo, whi, bhi = (3,), 1234567, (-5,), -7654321
    # (a) the rows tree: p_hi = 8, theta_lo = 2, two tables
    tabs = rng.integers(0, 4, (2, 8, 4))
    tv1 = np.stack([lut.tree_test_vectors(lambda h, l, T=T: T[h, l], 8, 4, 4, 2, p.N, torus_bits=64) for T in tabs])
    idx_a = np.array([0, 1, 1], np.int32)
    # (b) the multi-value tree: p_hi = 4, p_lo = 2, k = 2, two tables
    bits = rng.integers(0, 2, (2, 2, 4, 2))
    parts = [lut.tree_mvk_factors([lambda h, l, T=T: T[h, l] for T in tab], 4, 2, 2, N=p.N, torus_bits=64) for tab in bits]
    tv0, w = parts[0][0], np.stack([f for _, f in parts])
    idx_b, ob = np.array([1, 0, 1], np.int32), int(rng.integers(-2**63, 2**63))
    # (c) a TREE node (p_hi = 4, theta_lo = 2) feeding a TREE_MV node (k = 2), two instances; random tables: only words are compared
    cir = CIR.Circuit()
    a, b = cir.inputs(2)
    t = cir.tree(cir.tree_rows(rng.integers(-2**63, 2**63, (2, p.N), dtype=np.int64)), [a], [b], 4, lo_weights=wlo, hi_weights=whi, lo_bias=blo, hi_bias=bhi,
                 theta1=2)
    cir.tree_mv(cir.mv_base(rng.integers(-2**63, 2**63, p.N, dtype=np.int64)), rng.integers(-3, 4, (2, 4, 4)).astype(np.int32), [t], [b], lo_weights=wlo,
                hi_weights=whi, lo_bias=blo, hi_bias=bhi, out_bias=ob)
    x = np.stack([lo[:2], hi[:2]])   # [instance][wire][words]

    def call_a(ck):
        ck.set_tree_slice(8)   # one sample per slice
        try:
            return ck.tree_lut_bootstrap(tv1, lo, hi, p_hi=8, weights_lo=wlo, bias_lo=blo, theta=2, weights_hi=whi, bias_hi=bhi, table_index=idx_a)
        finally:
            ck.set_tree_slice(16384)

    def call_b(ck):
        return ck.tree_lut_bootstrap_mvk(w, lo, hi, tv0=tv0, weights_lo=wlo, bias_lo=blo, weights_hi=whi, bias_hi=bhi, table_index=idx_b, out_bias=ob)

    calls = dict(a=call_a, b=call_b, c=lambda ck: CIR.evaluate_batch(ck, cir, x))
    first = None
    for order in ("abc", "cba", "bca"):
        ck = thfhe.MKCloudKey(thfhe.make_params(**p.as_dict()), K.bk, K.ksk, device=0)
        try:
            ck.pack_key_set(pk, T_PK, BASEBIT)
            ck.set_profiling(False)
            got = {name: calls[name](ck) for name in order}
            if first is None:
                first = got
                assert got["a"].shape == (3, p.parties * p.n + 1) and got["b"].shape == (3, 2, p.parties * p.n + 1) and got["c"].shape[:2] == (2, 5)
                flat = _flat_rows(ck, tv1, lo, hi, 8, 2, wlo, blo, whi, bhi, idx_a)
                assert np.array_equal(got["a"], flat), ("a", differing(got["a"], flat))
                flat = _flat(ck, tv0, w, lo, hi, wlo, blo, whi, bhi, idx_b, ob)
                assert np.array_equal(got["b"], flat), ("b", differing(got["b"], flat))
            for name in order:
                assert np.array_equal(got[name], first[name]), (order, name, differing(got[name], first[name]))
        finally:
            ck.close()


def test_mv_and_tree_mv_groups_slice_by_their_own_member(O):
    """An MV group (q = 4) of 5 nodes and a TREE_MV group (k = 2, q = 4) of 3 nodes, two instances, in one gate-DAG run: the words of the unsliced
    run with mv_slice = q (one MV node per slice, the TREE_MV group whole), with tree_slice = k q (one TREE_MV node per slice, the MV group whole)
    and with dag_slice = 2 (two nodes per slice of either group)."""
    import thfhe
    from thfhe import circuits as CIR
    p = O.make_params("MK2", n=30)
    s = O.SIGMAS["MK2"]
    K = O.MKKeys(p, 59, s["bk"], s["ks"])
    rng = np.random.default_rng(0x5EED0072)
    pk = rng.integers(-2**63, 2**63, (p.N, T_PK, (1 << BASEBIT) - 1, 2, p.N), dtype=np.int64)
    cir = CIR.Circuit()
    ins = cir.inputs(3)
    b0 = cir.mv_base(rng.integers(-2**63, 2**63, p.N, dtype=np.int64))
    wm, wt = rng.integers(-2**31, 2**31, (2, 4, 4)).astype(np.int32), rng.integers(-3, 4, (2, 2, 4, 4)).astype(np.int32)
    ob = int(rng.integers(-2**63, 2**63))
    for j in range(5):
        cir.mv(b0, wm[j % 2], [ins[j % 3]], weights=(3,), bias=1234567, out_bias=ob)
    for j in range(3):
        cir.tree_mv(b0, wt[j % 2], [ins[j]], [ins[(j + 1) % 3]], hi_weights=(-5,), out_bias=ob)
    x = np.stack([R.encrypt_words(K, rng.integers(-2**31, 2**31, 3), s["lwe"], 90 + i) for i in range(2)])   # [instance][wire][words]
    ck = thfhe.MKCloudKey(thfhe.make_params(**p.as_dict()), K.bk, K.ksk, device=0)
    try:
        ck.pack_key_set(pk, T_PK, BASEBIT)
        st = {}
        ref = CIR.evaluate_batch(ck, cir, x, stats=st)
        assert (st["levels"], st["launches"], st["rotations"]) == (1, 3, (5 + 3 * 3) * 2)   # launch groups: MV, the level 1 and the selections of TREE_MV
        for setter, value, default in ((ck.set_mv_slice, 4, 4096), (ck.set_tree_slice, 8, 16384), (ck.set_dag_slice, 2, 8192)):
            setter(value)
            try:
                got = CIR.evaluate_batch(ck, cir, x)
            finally:
                setter(default)
            assert np.array_equal(got, ref), (setter.__name__, differing(got, ref))
    finally:
        ck.close()


@pytest.fixture(scope="module")
def mk4_full(O):
    """Full-size MK4 with the oracle's keys and a packing key from Z to Z of 12 one-bit digits (12 288 rows, 192 MiB), its ring products on the device."""
    import thfhe
    from thfhe import keygen
    p = O.make_params("MK4")
    s = O.SIGMAS["MK4"]
    K = O.MKKeys(p, 0x5EED0004, s["bk"], s["ks"])
    ck = thfhe.MKCloudKey(thfhe.make_params("MK4"), K.bk, K.ksk, device=0)
    Z = K.rlwe_keys.sum(axis=0)
    t0 = time.perf_counter()
    pk = keygen.gen_mk_pack_key(np.random.default_rng(0x5EED0014), Z, K.rlwe_keys, 12, 1, s["bk"], device=0)
    print(f"MK4 packing key (12, 1): {pk.shape[0] * 12} rows generated in {time.perf_counter() - t0:.2f} s")
    ck.pack_key_set(pk, 12, 1)
    yield p, s, K, ck, pk, Z
    ck.close()


def test_mk4_full_size_tree_decrypts_every_pair_and_feeds_the_gates(O, mk4_full):
    import thfhe
    from thfhe import lut
    p, s, K, ck, pk, Z = mk4_full
    orc = O.MKOracle(p, K.bk, K.ksk)
    fs = [lambda h, l: int(l > h), lambda h, l: (h ^ l) & 1]                       # taps of norm <= sqrt 2 and 2
    tv0, w, ob = lut.tree_mvk_bool_factors(fs, 4, 4, N=p.N, torus_bits=64)
    norms = np.sqrt((w.astype(np.float64)**2).sum(axis=-1))                        # [k][p_hi]
    assert norms.max() <= 2.0
    pairs = np.array([(h, l) for h in range(4) for l in range(4)])
    hi = R.encrypt_words(K, lut.encode(pairs[:, 0], 4), s["lwe"], 0x5EED0051)
    lo = R.encrypt_words(K, lut.encode(pairs[:, 1], 4), s["lwe"], 0x5EED0052)
    want = np.array([[f(h, l) for f in fs] for h, l in pairs]).astype(bool)
    # the model first, where the oracle is fast enough: one sample's three rotations of 2 040 CMuxes each, its words and its bits
    g = 6
    ref = TM.tree_mvk(orc, pk, 12, 1, tv0, w, [lo[g]], [hi[g]], out_bias=ob)
    assert K.decrypt_bits(ref).tolist() == want[g].tolist()
    got = ck.tree_lut_bootstrap_mvk(w, lo, hi, tv0=tv0, out_bias=ob)
    assert got.shape == (16, 2, p.parties * p.n + 1)
    assert np.array_equal(got[g], ref), (g, differing(got[g], ref))
    # every output decrypts; none is left out of the count
    flat = got.reshape(32, -1)
    err = (K.phases(flat).astype(np.int64) - np.where(want.reshape(-1), 1 << 29, -(1 << 29))) / 2.0**32
    rounding = np.sqrt(float((Z.astype(np.float64)**2).sum()) / 12) * 2.0**-12
    key = np.sqrt(p.N * p.N * 12 * p.parties * 0.5) * s["bk"]           # half of the one-bit digits are non-zero
    c2 = np.array([[norms[j, h]**2 for j in range(2)] for h, _ in pairs]).mean()   # the selected candidate's taps, mean square over the outputs
    pred = np.sqrt((c2 + 1) * SIGMA_BR_MK4**2 + rounding**2 + key**2 + SIGMA_KS_MK4**2)
    print(f"MK4 multi-value tree p = 4 x 4, k = 2: measured std {err.std():.3e} over {len(err)} outputs, max |err| {np.abs(err).max():.3e}; "
          f"predicted {pred:.3e} (mean |c|^2 {c2:.2f}, rounding {rounding:.2e}, key {key:.2e}); half-step / predicted {0.125 / pred:.1f}")
    assert np.array_equal(K.decrypt_bits(flat).reshape(16, 2), want)
    assert 0.5 * pred <= err.std() <= 2 * pred
    # the two outputs of every sample into the multi-key NAND
    nand = ck.gates(thfhe.NAND, got[:, 0], got[:, 1])
    assert np.array_equal(K.decrypt_bits(nand), ~(want[:, 0] & want[:, 1]))
