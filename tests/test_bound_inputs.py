"""CPU checks of the bound-level input recipe (tests/bound_inputs.py): the extreme key words and digit words decompose as claimed for every
parameter set and swept shape, the crafted bootstraps reach the limb sum they are meant to reach, and the oracle's schoolbook and NTT
paths agree on them, so the GPU comparison in test_gpu_exactness_bound.py is against exact values."""
import numpy as np
import pytest

import bound_inputs as B
from test_gpu_param_sweep import MK_SHAPES, SK_SHAPES


def _gadgets(O):
    """(torus bits, l, Bgbit) of every parameter set in oracle_lib and every shape of the GPU parameter sweep; the KMS gadgets too."""
    import thfhe
    out = {(p["torus_bits"], p["l"], p["Bgbit"]) for p in O.PARAM_SETS.values()}
    out |= {(32, l, bg) for _, l, bg, _, _ in SK_SHAPES} | {(64, l, bg) for _, _, l, bg, _, _ in MK_SHAPES}
    for k in thfhe.KMS_PARAM_SETS.values():
        out |= {(64, k["l_gsw"], k["bg_gsw"]), (64, k["l_lev"], k["bg_lev"]), (64, k["l_uni"], k["bg_uni"])}
    return sorted(out)


def test_extreme_key_words():
    assert B.extreme_key_word(32) == 0x7FFF8000
    assert B.split_limbs32(B.extreme_key_word(32)) == (-2**15, 2**15)
    assert B.extreme_key_word(64) == 0x7FFF7FFF7FFF8000
    assert B.split_limbs64(B.extreme_key_word(64)) == [-2**15, -2**15, -2**15, 2**15]


def test_digit_words_decompose_to_extreme_digits(O):
    for bits, l, Bgbit in _gadgets(O):
        x = B.digit_word(bits, l, Bgbit)
        d = B.decompose(np.full(4, x), bits, l, Bgbit)
        e = B.extreme_digit(Bgbit)
        assert np.all(d == e), (bits, l, Bgbit)
        parts, pw = B.digit_parts(Bgbit)
        cut = B.cut_parts(e, parts, pw)
        assert sum(v << (pw * w) for w, v in enumerate(cut)) == e
        if parts == 1:
            assert e == -2**(Bgbit - 1)
        else:   # every lower part at -2^(pw-1); the top part as low as the digit range allows
            assert cut[:-1] == [-2**(pw - 1)] * (parts - 1)
            assert e - 2**(pw * (parts - 1)) < -2**(Bgbit - 1) <= e
        # the bootstrap reaches it: body mu, X^N acc - acc = -2 mu
        assert B.wrap(-2 * B.crafted_mu(bits, l, Bgbit), bits) == x
    assert B.crafted_mu(32, 3, 7) == 0x40810000
    # a lone -2^25 is not extreme for the three 9-bit parts of a 26-bit digit
    assert B.cut_parts(-2**25, 3, 9) == [0, 0, -128]


@pytest.mark.parametrize("l, Bgbit", [(2, 10), (3, 7), (3, 10), (1, 8), (2, 7), (3, 6)])
def test_single_key_recipe_reaches_the_bound(O, l, Bgbit):
    p = O.make_params("SK-128", n=4, l=l, Bgbit=Bgbit)
    K = O.SKKeys(p, 0xB0 + l, 2.0**-25, 2.0**-15)
    for full in (True, False):
        bk, x, mu, step = B.sk_case(p, K.bk, full)
        orc = O.Oracle(p, bk, K.ksk)
        assert B.sk_reached(orc, p, bk, x, mu, step) == B.bound(2 * l, p.N, Bgbit) // (1 if full else 2)
        acc = B.sk_acc_before(orc, p, x, mu, step)
        assert np.all(acc[1] == mu) and np.all(acc[0] == (mu if full else 0))   # full: step 0 copied the body into the mask
        assert np.array_equal(orc.bootstrap_wo_keyswitch(x, mu), orc.bootstrap_wo_keyswitch(x, mu, schoolbook=True))
    # l Bgbit = 32: only the half recipe
    p = O.make_params("SK-128", n=2, l=4, Bgbit=8)
    K = O.SKKeys(p, 5, 2.0**-25, 2.0**-15)
    bk, x, mu, step = B.sk_case(p, K.bk, False)
    orc = O.Oracle(p, bk, K.ksk)
    assert B.sk_reached(orc, p, bk, x, mu, step) == B.bound(8, p.N, 8) // 2


@pytest.mark.parametrize("name, frac", [("MK2", 1.0), ("MK8", 1.0), ("MK4-N2048", 1.0), ("MK16", 0.83), ("MK128", 0.83), ("MK256", 0.99),
                                        ("MK64-fft", 0.99)])
def test_multi_key_recipe_reaches_the_bound(O, name, frac):
    p = O.make_params(name, n=2, parties=2)
    K = O.MKKeys(p, 0xB1, 2.0**-30.70, 2.0**-13.52)
    bk, x, mu = B.mk_case(p, K.bk, [0, 1], full=True)
    orc = O.MKOracle(p, bk, K.ksk)
    bd = B.bound(2 * p.l, p.N, p.Bgbit)
    for k in range(2):
        acc, steps = B.mk_rotate(orc, p, bk, x[k], mu)
        assert len(steps) == 1 and frac * bd <= steps[0][2] <= bd, (steps, bd)
        assert frac < 1.0 or steps[0][2] == bd
        assert np.array_equal(orc.bootstrap_wo_keyswitch(x[k], mu), orc.bootstrap_wo_keyswitch(x[k], mu, schoolbook=True))


def test_ccs_oracle_exact_on_extreme_keys(O):
    # the CCS products with every bootstrap-key, public-key and common-key word at 0x7FFF8000 on a mask word of 2^31: schoolbook == NTT
    p = O.make_params("CCS2", n=2)
    s = O.SIGMAS["CCS2"]
    K = O.CCSKeys(p, 7, s["bk"], s["ks"])
    for a in (K.bk, K.pk, K.crs):
        a[...] = B.extreme_key_word(32)
    orc = O.CCSOracle(p, K)
    x = np.zeros(p.parties * p.n + 1, np.int32)
    x[0] = x[p.n + 1] = -2**31
    mu = B.crafted_mu(32, p.l, p.Bgbit)
    assert np.array_equal(orc.bootstrap_wo_keyswitch(x, mu), orc.bootstrap_wo_keyswitch(x, mu, schoolbook=True))


def test_ccs_recipe_reaches_the_stage2_bound(O):
    # (P + 1) l 2^(Bgbit-1) = 3072: the largest stage-2 sum thfhe_ccs_ctx_create admits, reached exactly
    p = O.make_params("CCS2", n=3, parties=3)
    s = O.SIGMAS["CCS2"]
    K = O.CCSKeys(p, 0xB2, s["bk"], s["ks"])
    bk, pk, crs, x, mu, step = B.ccs_case(p, K.bk, K.pk, K.crs)
    K.bk[...], K.pk[...], K.crs[...] = bk, pk, crs
    orc = O.CCSOracle(p, K)
    s1, s2 = B.ccs_reached(orc, p, bk, pk, crs, x, mu, step)
    assert s1 == B.bound(p.l, p.N, p.Bgbit) and s2 == B.bound(12, p.N, p.Bgbit) == 3072 * p.N * 2**15
    assert np.array_equal(orc.bootstrap_wo_keyswitch(x, mu), orc.bootstrap_wo_keyswitch(x, mu, schoolbook=True))


def test_kms_recipes_reach_the_bound(O):
    import thfhe
    from thfhe import keygen
    p = thfhe.make_kms_params("KMS4", n=3, parties=2)
    K = keygen.KMSSecretKeySet(p, seed=11)
    bd = B.bound(2 * p.l_gsw, p.N, p.bg_gsw)
    gsw, bara, acc = B.kms_rlwe_case(p, K.gsw, 1)
    assert B.gsw_reached(acc, p.N, gsw[1, 0], p.l_gsw, p.bg_gsw) == bd
    orc = O.KMSOracle(p, gsw, K.uni, K.pk, K.crs, K.ksk)
    assert np.array_equal(orc.rlwe_rotate(1, bara, acc), orc.rlwe_rotate(1, bara, acc, schoolbook=True))
    gsw, bara = B.kms_tlev_case(p, K.gsw, 0)
    orc = O.KMSOracle(p, gsw, K.uni, K.pk, K.crs, K.ksk)
    init = np.zeros((2, p.N), np.int64)
    init[1, 0] = 1 << (64 - p.bg_lev)
    acc = orc.rlwe_rotate(0, np.where(np.arange(p.n) == 0, bara, 0).astype(np.int32), init)
    assert np.all(acc[0] == B.crafted_mu(64, p.l_gsw, p.bg_gsw))
    assert 0.999 * bd <= B.gsw_reached(acc, p.N, gsw[0, 1], p.l_gsw, p.bg_gsw) < bd
    assert np.array_equal(orc.tlev_rotate(0, bara), orc.tlev_rotate(0, bara, schoolbook=True))


# ---- leveled table lookup and encrypted-table bootstrap (the crafting facts test_gpu_exactness_bound.py relies on) ------------------
LHE_SHAPES = [(1, 8), (2, 10), (3, 7), (3, 10), (4, 8)]   # (l, Bgbit) of the leveled cases in test_gpu_exactness_bound.py


def _lhe_params(O, l, Bgbit):
    return O.make_params("SK-128", n=4, l=l, Bgbit=Bgbit)


@pytest.mark.parametrize("l, Bgbit", LHE_SHAPES)
def test_leveled_cmux_recipe_reaches_the_bound(O, l, Bgbit):
    import lhe_reference as LR
    p = _lhe_params(O, l, Bgbit)
    N, T, e = p.N, B.digit_word(32, l, Bgbit), B.extreme_digit(Bgbit)
    assert e == -2**(Bgbit - 1)
    C, d1, d0 = B.lhe_cmux_case(p)
    # fact 1: T at all N coefficients decomposes to e at every level
    assert np.all(B.decompose(d1[:N], 32, l, Bgbit) == e) and np.all(B.decompose(d1[N:], 32, l, Bgbit) == e)
    # fact 2: against the constant extreme key word the 2l rows give the bound exactly; the l body rows alone give half
    assert np.all(C == B.extreme_key_word(32)) and not d0.any()
    bd = B.bound(2 * l, N, Bgbit)
    assert B.lhe_reached(p, C, LR._sub(d1, d0)) == bd
    assert B.lhe_reached(p, C, np.concatenate([np.zeros(N, np.int32), d1[N:]])) == B.bound(l, N, Bgbit) == bd // 2
    # ... and from non-zero operands with the same difference
    w = np.random.default_rng(l * 100 + Bgbit).integers(-2**31, 2**31, 2 * N, dtype=np.int64).astype(np.int32)
    assert np.array_equal(LR._sub(LR._add(w, d1), w), d1)
    # (3, 10) is the largest of the five sums: 6 x 1024 x 2^9 x 2^15 = 2^36.6
    assert bd <= 6 * 1024 * 2**9 * 2**15 and (bd == 6 * 1024 * 2**9 * 2**15) == ((l, Bgbit) == (3, 10))


@pytest.mark.parametrize("l, Bgbit", LHE_SHAPES)
def test_leveled_rotation_tables_reach_the_bound(O, l, Bgbit):
    import lut_reference as R
    p = _lhe_params(O, l, Bgbit)
    N, T = p.N, B.digit_word(32, l, Bgbit)
    C = np.full((2 * l, 2, N), B.extreme_key_word(32), np.int32)
    assert B.lhe_rot_table(p, 512).tolist() == [B.wrap(-T, 32)] * 512 + [0] * 512
    assert B.lhe_rot_table(p, 256)[::256].tolist() == [B.wrap(-2 * T, 32), B.wrap(-T, 32), 0, B.wrap(T, 32)]
    for s in (512, 256, 128, 1):
        tab = B.lhe_rot_table(p, s)
        # fact 3: X^(2N - s) ACC - ACC equals T at all N coefficients (oracle_mul_by_monomial32)
        rot = R.monomial(tab, 2 * N - s, N)
        assert np.all(R.to_i32(rot.astype(np.int64) - tab) == B.wrap(T, 32)), s
        diff = B.lhe_rot_diff(tab, tab, 2 * N - s)
        assert np.all(diff == B.wrap(T, 32))
        if s >= 256:
            assert B.lhe_reached(p, C, diff) == B.bound(2 * l, N, Bgbit)
            assert B.lhe_reached(p, C, B.lhe_rot_diff(None, tab, 2 * N - s)) == B.bound(2 * l, N, Bgbit) // 2   # public table: zero mask


@pytest.mark.parametrize("l, Bgbit", LHE_SHAPES)
def test_random_words_stay_far_below_the_leveled_bound(O, l, Bgbit):
    # why test_gpu_lhe_shapes.py cannot stand in for the crafted cases: random TGSW words against random differences leave the peak limb sum
    # more than 5 bits below the bound (a statement about the reference inputs; the sum is sqrt(2 l N) incoherent terms, not 2 l N coherent ones)
    p = _lhe_params(O, l, Bgbit)
    rng = np.random.default_rng(50 + l * 16 + Bgbit)
    words = lambda *shape: rng.integers(-2**31, 2**31, size=shape, dtype=np.int64).astype(np.int32)
    for _ in range(3):
        assert B.lhe_reached(p, words(2 * l, 2, p.N), words(2 * p.N)) < B.bound(2 * l, p.N, Bgbit) // 32


@pytest.mark.parametrize("l, Bgbit", [(2, 10), (3, 7), (3, 10), (4, 8)])
def test_encrypted_table_recipe_reaches_the_bound_at_step_0(O, l, Bgbit):
    import tree_lut_reference as TR
    p = _lhe_params(O, l, Bgbit)
    K = O.SKKeys(p, 0xB0 + l, 2.0**-25, 2.0**-15)
    bk, x, mu = B.lut_enc_case(p, K.bk)
    assert B.digit_word(32, l, Bgbit) % 2 == 0 and B.wrap(-2 * mu, 32) == B.digit_word(32, l, Bgbit)
    for theta in (1, 2, 4):   # bara_0 = N (mod 2N) whatever theta is
        assert (O.lib().oracle_modswitch(int(x[0]), p.N // theta) * theta) % (2 * p.N) == p.N
    assert B.lut_enc_reached(p, bk, mu) == B.bound(2 * l, p.N, Bgbit)
    orc = O.Oracle(p, bk, K.ksk)
    tv = np.full(p.N, mu, np.int32)
    u = TR.lut_enc_wo_keyswitch(orc, x, tv, tv, 4)
    assert u.shape == (4, p.N + 1)
    # the oracle's schoolbook path agrees on the crafted step: the accumulator (mu, mu) through CMux 0 at bara = N
    acc = np.full((2, p.N), mu, np.int32)
    assert np.array_equal(orc.mux_rotate(0, p.N, acc), orc.mux_rotate(0, p.N, acc, schoolbook=True))


# ---- multi-value bootstrap at the bound (the crafting facts test_gpu_mv_bound.py relies on) -----------------------------------------------------
# (l, Bgbit, full) of test_gpu_mv_bound.py: the shapes of test_single_key_at_the_bound, and l = 1 for the <1, ...> instantiations
MV_SHAPES = [(1, 8, True), (2, 10, True), (3, 7, True), (3, 10, True), (4, 8, False)]
MV_IDS = ["l1-Bg8", "SK-80", "SK-128", "l3-Bg10", "l4-Bg8-half"]
MV_PQ = [(2, 1), (64, 9), (8, 64)]       # (taps, outputs): the smallest; the most taps, q off the eight waves; the most outputs
MV_TABLES = 2


def _mv_case(O, l, Bgbit, full):
    """(params, keys, crafted key, record, mu, crafted step, oracle) of one multi-value bound case"""
    p = O.make_params("SK-128", n=4, l=l, Bgbit=Bgbit)
    K = O.SKKeys(p, 0xB0 + l, 2.0**-25, 2.0**-15)
    bk, x, mu, step = B.sk_case(p, K.bk, full)
    return p, K, bk, x, mu, step, O.Oracle(p, bk, K.ksk)


@pytest.mark.parametrize("l, Bgbit, full", MV_SHAPES, ids=MV_IDS)
def test_multi_value_recipe_reaches_the_bound(O, l, Bgbit, full):
    import lut_reference as R
    import mv_lut_reference as MV
    p, K, bk, x, mu, step, orc = _mv_case(O, l, Bgbit, full)
    assert B.sk_reached(orc, p, bk, x, mu, step) == B.bound(2 * l, p.N, Bgbit) // (1 if full else 2)
    # one input of weight 1 and bias 0: the prologue leaves the record alone, barb = 0, and tv0 = mu everywhere is the gate's accumulator
    xs = R.prologue([x], (1,), 0)
    assert np.array_equal(xs, x) and O.lib().oracle_modswitch(int(x[p.n]), p.N) == 0
    acc = MV.rotate(orc, xs, np.full(p.N, mu, np.int32))
    assert np.array_equal(acc, B.sk_acc_after(orc, p, x, mu))              # the model's rotation (NTT) = the oracle's schoolbook steps
    assert np.array_equal(R.extract_at(acc, 0, p.N), orc.bootstrap_wo_keyswitch(x, mu))   # ... = the accumulator of the oracle's own bootstrap


@pytest.mark.parametrize("l, Bgbit, full", MV_SHAPES, ids=MV_IDS)
def test_multi_value_records_see_one_lsb(O, l, Bgbit, full):
    """What the compared records of test_gpu_mv_bound.py expose of the accumulator: the mask column, all N coefficients (the peak at N - 1 is
    observed there), through the unit-tap output 0 of every factor table -- bit 0 of any mask coefficient moves exactly one word of it by one --
    and of the body the coefficients at the tap positions N - box/2 - k box only."""
    import mv_lut_reference as MV
    p, K, bk, x, mu, step, orc = _mv_case(O, l, Bgbit, full)
    N = p.N
    acc = B.sk_acc_after(orc, p, x, mu)
    for pt, q in MV_PQ:
        w = B.mv_factors(np.random.default_rng(0xF0 + pt), MV_TABLES, q, pt)
        taps = B.mv_tap_positions(N, pt)
        for t in range(MV_TABLES):
            assert np.count_nonzero(w[t, 0]) == 1 and w[t, 0].sum() == 1
            ref = MV.combine(acc, w[t], N)
            assert ref.shape == (q, N + 1)
            for c in (N - 1, 0, 517):                   # mask coefficients: the peak and two others
                bad = acc.copy()
                bad[c] ^= 1
                got = MV.combine(bad, w[t], N)
                delta = got[0].astype(np.int64) - ref[0]
                assert np.count_nonzero(delta) == 1 and abs(int(delta[np.flatnonzero(delta)[0]])) == 1, (pt, q, t, c)
                assert not delta[N]
            used = np.flatnonzero(np.any(w[t] != 0, axis=0))
            for c in (taps[used[0]], taps[used[-1]]):   # body coefficients a (non-zero) tap reads
                bad = acc.copy()
                bad[N + c] ^= 1
                assert not np.array_equal(MV.combine(bad, w[t], N), ref), (pt, q, t, c)
            bad = acc.copy()                            # ... and one no tap reads: not exposed
            assert N - 1 not in taps
            bad[N + N - 1] ^= 1
            assert np.array_equal(MV.combine(bad, w[t], N), ref)


# ---- layered automata at the bound (the crafting facts test_gpu_wfa_bound.py relies on) ---------------------------------------------------------
WFA_KINDS = [(kind, variant) for kind in ("enc", "pub") for variant in ("zero d0", "random d0")]


def _wfa_diff(fa, fb, t0, t1):
    """d1 - d0 of a transition, int32[2N]; fa None: zero masks"""
    import lhe_reference as LR
    N = fb.shape[1]
    z = np.zeros(N, np.int32)
    return LR._sub(np.concatenate([z if fa is None else fa[t1], fb[t1]]), np.concatenate([z if fa is None else fa[t0], fb[t0]]))


@pytest.mark.parametrize("l, Bgbit", LHE_SHAPES)
def test_automaton_recipe_reaches_the_bound(O, l, Bgbit):
    import lhe_reference as LR
    import wfa_reference as WR
    p = _lhe_params(O, l, Bgbit)
    N, T = p.N, B.wrap(B.digit_word(32, l, Bgbit), 32)
    for n_states in (5, 4, 1):
        C, fin, trans = B.wfa_case(p, n_states)
        assert np.all(C == B.extreme_key_word(32)) and fin.shape == (n_states, 2 * N)
        assert trans.tolist() == [[q & ~1, q | 1] for q in range(n_states - 1)] + [[n_states - 1] * 2]
        assert not fin[0::2].any() and np.all(fin[1::2] == T)
    C, _, trans = B.wfa_case(p, B.WFA_STATES)
    for kind, variant in WFA_KINDS:
        fa, fb = B.wfa_bound_finals(p, kind, variant, 0xA0 + l)
        if variant == "random d0":      # every pair has words of its own: a state read at another state's index shows
            assert len({fb[q].tobytes() for q in range(B.WFA_STATES)}) == B.WFA_STATES
        rows = 2 * l if kind == "enc" else l
        V = WR.layer0(p, [C[None]], trans[None], [0], fa, fb)
        z = np.zeros(N, np.int32)
        state = lambda q: np.concatenate([z if fa is None else fa[q], fb[q]])
        for q, (t0, t1) in enumerate(trans.tolist()):
            if t0 == t1:
                assert q == B.WFA_STATES - 1 and np.array_equal(V[q], state(t0))
                continue
            diff = _wfa_diff(fa, fb, t0, t1)
            assert np.all(diff[N:] == T) and np.all(diff[:N] == (T if kind == "enc" else 0))
            assert B.lhe_reached(p, C, diff) == B.bound(rows, N, Bgbit), (kind, variant, q)
            assert np.array_equal(V[q], LR.cmux(p, C, state(t1), state(t0))), (kind, variant, q)


@pytest.mark.parametrize("l, Bgbit", LHE_SHAPES)
def test_automaton_records_see_one_lsb(O, l, Bgbit):
    """What the compared records of test_gpu_wfa_bound.py (theta = 4, start = every state) expose of a layer-0 state: the mask column, all N
    coefficients (the peak at N - 1 is observed there), and of the body the theta extracted coefficients 0 .. 3 only.  In the automaton whose
    crafted step is followed by a random step, every state the crafted step wrote is the d0 of one CMux of the step above, so bit 0 of its words
    is added into an output undecomposed."""
    import lut_reference as R
    import wfa_reference as WR
    p = _lhe_params(O, l, Bgbit)
    N, S, theta = p.N, B.WFA_STATES, 4
    Cs = B.wfa_bound_bits(p)
    records = lambda V: np.stack([np.stack([R.extract_at(V[q], j, N) for j in range(theta)]) for q in range(S)])
    for name, (trans, step_bit) in B.wfa_bound_automata(p).items():
        for kind, variant in WFA_KINDS:
            fa, fb = B.wfa_bound_finals(p, kind, variant, 0xA0 + l)
            V = WR.layer0(p, [Cs], trans, step_bit, fa, fb)
            ref = records(V)
            for q in range(S):
                for c, seen in ((N - 1, True), (300, True), (N + 0, True), (N + theta - 1, True), (N + theta, False), (2 * N - 1, False)):
                    bad = [v.copy() for v in V]
                    bad[q][c] ^= 1
                    got = records(bad)
                    assert np.array_equal(got, ref) != seen, (name, kind, variant, q, c)
                    assert np.array_equal(np.delete(got, q, axis=0), np.delete(ref, q, axis=0))
            if name != "then-random":
                continue
            # one LSB in the layer the crafted step wrote, before the random step reads it
            V1 = WR.layer0(p, [Cs], trans[1:], step_bit[1:], fa, fb)
            assert np.array_equal(ref, records(WR.layer0(p, [Cs], trans[:1], step_bit[:1], np.stack(V1)[:, :N], np.stack(V1)[:, N:])))
            for q in (0, 3):
                for c in (N - 1, 300):
                    bad = np.stack(V1)
                    bad[q, c] ^= 1
                    got = records(WR.layer0(p, [Cs], trans[:1], step_bit[:1], bad[:, :N], bad[:, N:]))
                    assert not np.array_equal(got, ref), (kind, variant, q, c)
