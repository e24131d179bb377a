"""Leveled CMux and lookup on the 64-bit ring of degree 2048, host side (no GPU): the argument checks of the C ABI that
run before any device work, the numpy model (tests/mk_lhe_reference.py) pinned to the oracle, MKSecretKeySet.tgsw_encrypt, the real-key cases of
tests/test_gpu_mk_lhe.py on the model (every address decodes before the device is asked), the noise next to the formula, and the crafted case
at the transform's exactness bound."""
import ctypes as C

import numpy as np
import pytest

import mk_lhe_cases as CS
import mk_lhe_reference as M

N, L, BGBIT = CS.N, CS.L, CS.BGBIT


# ---- ABI ---------------------------------------------------------------------------------------------------------------------------------

def _p64(a):
    return a.ctypes.data_as(C.POINTER(C.c_int64))


def test_abi_refuses_bad_arguments_before_the_context_is_looked_at():
    import thfhe
    L_ = thfhe.lib()
    err = lambda: L_.thfhe_last_error().decode()
    w, o32, idx = np.zeros(16, np.int64), np.zeros(16, np.int32), np.zeros(4, np.int32)
    p, q, h = _p64(w), thfhe._p32(o32), C.c_void_p()
    fake = C.c_void_p(8)   # a set pointer that is never dereferenced: every refusal below comes before the set is looked at
    create = L_.thfhe_mk_tgsw_set_create
    assert create(None, None, 1, 3, C.byref(h)) == -1 and "null argument" in err()
    assert create(None, p, 1, 3, None) == -1 and "null argument" in err()
    for d in (0, -1, 17):
        assert create(None, p, 1, d, C.byref(h)) == -1 and "d must be 1 .. 16" in err()
    for count in (0, (1 << 24) + 1):
        assert create(None, p, count, 3, C.byref(h)) == -1 and "count must be 1 .. 2^24" in err()
    assert create(None, p, 1, 3, C.byref(h)) == -1 and "null ctx" in err()
    assert not h.value
    L_.thfhe_mk_tgsw_set_destroy(None)   # a no-op
    cmux = L_.thfhe_mk_lhe_cmux
    for k in range(6):
        a = [p] * 6
        a[k] = None
        assert cmux(None, fake, 0, *a, 1) == -1 and "null argument" in err()
    for bit in (-1, 16):
        assert cmux(None, fake, bit, p, p, p, p, p, p, 1) == -1 and "bit must be" in err()
    assert cmux(None, None, 0, p, p, p, p, p, p, 1) == -1 and "null tgsw set" in err()
    for name in ("thfhe_mk_lhe_lookup", "thfhe_mk_lhe_lookup_wo_keyswitch"):
        fn = getattr(L_, name)
        ok = dict(first=0, count=1, d_tree=1, d_rot=2, theta=1, tab_a=None, tab_b=p, n_tables=1, index=None, out=q)

        def call(set_=fake, **kw):
            v = dict(ok, **kw)
            return fn(None, set_, v["first"], v["count"], v["d_tree"], v["d_rot"], v["theta"], v["tab_a"], v["tab_b"], v["n_tables"], v["index"], v["out"])
        assert call(tab_b=None) == -1 and "null argument" in err()
        assert call(out=None) == -1 and "null argument" in err()
        for v in (-1, 7):
            assert call(d_tree=v) == -1 and "d_tree must be 0 .. 6" in err()
        for v in (-1, 12):
            assert call(d_rot=v) == -1 and "d_rot must be 0 .. 11" in err()
        for v in (0, 3, 8):
            assert call(theta=v) == -1 and "theta must be 1, 2 or 4" in err()
        assert call(d_rot=11, theta=2) == -1 and "box" in err()            # box = 1
        assert call(d_rot=10, theta=4) == -1 and "box" in err()            # box = 2
        assert call(n_tables=0) == -1 and "n_tables" in err()
        assert call(d_tree=6, n_tables=4097) == -1 and "n_tables" in err()
        idx[:] = (0, 1, 2, 0)
        assert call(count=4, n_tables=2, index=thfhe._p32(idx)) == -1 and "table_index" in err().replace(" ", "_")
        assert call(set_=None) == -1 and "null tgsw set" in err()


def test_python_layer_checks_shapes():
    import thfhe
    from thfhe import keygen, lut
    p2 = thfhe.make_params(**dict(CS.KW, parties=2))
    with pytest.raises(ValueError, match="parties = 1"):
        keygen.MKSecretKeySet._one_party(type("K", (), {"params": p2})(), "tgsw_encrypt")
    t = lut.lhe_table(np.arange(8), 1, 2, N=N, torus_bits=64)
    assert t.dtype == np.int64 and t.shape == (2, N) and t[1, 3 * 512] == 7 and t[0, 512] == 1
    assert lut.lhe_table(np.arange(1 << 11), 0, 11, N=N, torus_bits=64).shape == (1, N)
    with pytest.raises(ValueError):
        lut.lhe_table(np.arange(1 << 11), 0, 11)          # N = 1024 stops at d_rot = 10
    with pytest.raises(ValueError):
        lut.lhe_table(np.arange(8), 1, 2, torus_bits=48)
    assert lut.lhe_table(np.arange(8), 1, 2).dtype == np.int32   # the 32-bit ring's tables are what they were


# ---- the model against the oracle ------------------------------------------------------------------------------------------------------------

def test_product_equals_polymul_small64():
    from thfhe import keygen
    rng = np.random.default_rng(5)
    for n in (8, N):
        small, torus = rng.integers(-256, 257, n), CS.words64(rng, n)
        assert np.array_equal(M.negacyclic(small, torus), keygen.polymul_small64(torus[None], small)[0])
    ext = np.array([-256] * N), np.full(N, -2**63, np.int64)
    assert np.array_equal(M.negacyclic(*ext), keygen.polymul_small64(ext[1][None], ext[0])[0])


def test_cmux_equals_the_oracles_mux_rotate(O):
    """cmux(C, X^a acc, acc) == MKOracle.mux_rotate(0, i, a, acc) of an oracle whose bk is the set (n = d), on random words."""
    d = 3
    rng = np.random.default_rng(6)
    p = O.make_params(**dict(CS.KW, n=d))
    bk = CS.words64(rng, 1, d, 4, L, N)
    orc = O.MKOracle(p, bk, np.zeros(O.mk_ksk_shape(p), np.int32))
    S = M.Set(bk[0], d, L, BGBIT)
    for i, a in ((0, 1), (1, N - 1), (2, N), (0, N + 1), (1, 2 * N - 1), (2, 1536)):
        acc = CS.words64(rng, 2, N)
        want = orc.mux_rotate(0, i, a, acc.reshape(-1)).reshape(2, N)
        assert np.array_equal(M.cmux(S, 0, i, M.monomial(acc, a), acc), want), (i, a)
    # the digit rule at its edges: every word whose digits are the extreme values of a level
    edge = np.array([0, -1, 2**63 - 1, -2**63, 1 << 27, (1 << 27) - 1, CS.BI.digit_word(64, L, BGBIT)], np.int64)
    dg = M.decompose(edge, L, BGBIT)
    parts, pw = M.digit_parts(BGBIT)
    assert (parts, pw) == (2, 9) and dg.shape == (L * parts, edge.shape[0])
    assert dg.min() >= -(1 << (pw - 1)) and dg.max() <= 1 << (pw - 1)
    for k, v in enumerate(edge):
        whole = CS.BI.decompose(np.array([v], np.int64), 64, L, BGBIT)[:, 0]
        assert [int(dg[lv * parts, k] + (dg[lv * parts + 1, k] << pw)) for lv in range(L)] == whole.tolist()


# ---- keys ----------------------------------------------------------------------------------------------------------------------------------

def test_tgsw_encrypt_rows_decode_to_the_gadget():
    p, K, orc = CS.keys()
    bits = np.array([0, 1, 1, 0, 1], np.int64)
    w = K.tgsw_encrypt(bits, seed=99)
    assert w.shape == (5, 4, L, N) and w.dtype == np.int64
    assert np.array_equal(w, K.tgsw_encrypt(bits, seed=99)) and not np.array_equal(w, K.tgsw_encrypt(bits, seed=98))
    tol = 2.0**-50   # row noise ~ sigma_bk sqrt(1 + |r|^2 + |z|^2) = 2^-57
    for lv in range(L):
        g = 1 << (64 - (lv + 1) * BGBIT)
        body = K.tlwe_phase(w[:, 3, lv], w[:, 0, lv])       # (mask part_4, body part_1): bit * g on coefficient 0
        want = np.zeros((5, N), np.int64)
        want[:, 0] = bits * g
        assert np.abs((body - want) / 2.0**64).max() < tol
        mask = K.tlwe_phase(w[:, 2, lv], w[:, 1, lv])       # (mask part_3, body part_2): -z * bit * g
        zg = (-K.rlwe_keys[0][None, :] * bits[:, None] * g).astype(np.int64)
        assert np.abs((mask - zg) / 2.0**64).max() < tol
    a, b = K.ring_encrypt(np.arange(2 * N, dtype=np.int64).reshape(2, N) << 40, seed=3)
    assert np.abs((K.tlwe_phase(a, b) - (np.arange(2 * N).reshape(2, N) << 40)) / 2.0**64).max() < 2.0**-58


# ---- real keys on the model -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("d_tree,d_rot", [(1, 2), (2, 1)])
def test_model_decodes_every_address(d_tree, d_rot, capsys):
    p, K, orc = CS.keys()
    values, w, ta, tb, tab = CS.real_case(d_tree, d_rot)
    d = d_tree + d_rot
    S = CS.model_set(w, d)
    errs = []
    for enc in (False, True):
        for s in range(1 << d):
            acc = M.lookup_acc(S, s, d_tree, d_rot, ta if enc else None, tb if enc else tab)
            ph = K.tlwe_phase(acc[0], acc[1])
            errs.append((ph[0] - CS.encode64(values[s])) / 2.0**64)
            rec = CS.records(acc, 1)
            assert CS.decode32(K.ring_phase(rec))[0] == values[s], (enc, s)                        # before the key switch
            assert CS.decode32(K.phase(orc.keyswitch(rec[0])))[0] == values[s], (enc, s)           # ... and after
    z2 = float((K.rlwe_keys[0].astype(np.float64) ** 2).sum())
    row = CS.SIGMA_BK * np.sqrt(1.0 + 2 * 0.113546097609674 * N + z2)      # a TGSW row: e + r (*) e_B - z (*) e', E|r|^2 = 2 P(+-1) N
    sigma1 = np.sqrt(2 * L * N * (1 << BGBIT) ** 2 / 12.0) * row
    pred, got = np.sqrt(d) * sigma1, float(np.std(errs))
    with capsys.disabled():
        print(f"\n[mk lhe noise] ({d_tree}, {d_rot}) |z|^2 = {z2:.0f}: sigma_1 = 2^{np.log2(sigma1):.2f}, predicted sqrt(d) sigma_1 = 2^{np.log2(pred):.2f}, "
              f"measured over {len(errs)} lookups 2^{np.log2(got):.2f}, ratio {got / pred:.2f}")
    assert got < 2.0**-28   # four bits inside the 32 bits of the extracted word; the ratio to the formula is reported, not asserted


def test_device_real_key_case_decodes_on_the_model():
    """What tests/test_gpu_mk_lhe.py::test_real_keys_decode asks the device: decoded here first."""
    p, K, orc = CS.keys()
    values, w, ta, tb, tab = CS.real_case(1, 2)
    S = CS.model_set(w, 3)
    got = [CS.decode32(K.phase(M.lookup(S, orc, s, 1, 2, 1, ta, tb)))[0] for s in range(8)]
    assert got == values.tolist()


# ---- the exactness bound -----------------------------------------------------------------------------------------------------------------------

def test_bound_case_reaches_the_bound():
    """The crafted CMux reaches 0.997 of 2 l parts N 2^(part bits - 1) 2^15 = 2^37, the quantity thfhe_mk_ctx_create checks."""
    assert CS.BOUND == 1 << 37
    w, d1, d0 = CS.bound_cmux_case()
    dg = M.decompose(M._sub(d1, d0), L, BGBIT)
    assert set(np.unique(dg).tolist()) == {-256, -255}      # every digit part at its extreme
    reached = CS.bound_reached(w[0, 0], M._sub(d1, d0))
    assert reached == 137036300288 and reached > 0.99 * CS.BOUND
    # the rotation kernel's crafted step: X^(2N - box) ACC - ACC of the table is the same word everywhere, on both polynomials
    tab = CS.bound_rot_table(512)
    acc = np.stack([tab, tab])
    diff = M._sub(M.monomial(acc, 2 * N - 512), acc)
    assert np.all(diff == CS.BI.digit_word(64, L, BGBIT))
    assert CS.bound_reached(w[0, 0], diff) == reached


def test_bound_case_sees_one_flipped_bit():
    """A unit error in one limb sum of the crafted step changes a compared word: every limb for thfhe_mk_lhe_cmux, whose outputs are the 64-bit
    words; limbs 2 and 3 for the lookup, whose records are the upper 32 bits (limbs 0 and 1 of an accumulator lie below the extracted word and
    below the 36 bits the next step's digits read)."""
    w, d1, d0 = CS.bound_cmux_case()
    rng = np.random.default_rng(8)
    words = np.concatenate([w, CS.words64(rng, 1, 1, 4, L, N)], axis=1)     # bit 0 crafted, bit 1 random: the step that follows
    S = CS.model_set(words, 2)
    tab = CS.bound_rot_table(512)
    acc0 = np.stack([tab, tab])
    step0 = M.cmux(S, 0, 0, M.monomial(acc0, 2 * N - 512), acc0)
    good = CS.records(M.cmux(S, 0, 1, M.monomial(step0, 2 * N - 1024), step0), 1)
    assert np.array_equal(good, M.lookup_wo_keyswitch(S, 0, 0, 2, 1, tab, tab))
    for h in (2, 3):
        bad = step0.copy()
        bad[1, N - 1] += np.int64(1) << (16 * h)
        assert not np.array_equal(CS.records(M.cmux(S, 0, 1, M.monomial(bad, 2 * N - 1024), bad), 1), good), h
