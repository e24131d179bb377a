"""The FP64 product paths on the MI355X at the exactness bound of DESIGN.md section 3 (pytest -m gpu).

Random keys and ciphertexts keep every limb sum 6 - 8 bits below rows * N * 2^(digit bits - 1) * 2^15, so a kernel that lost a few bits of
transform accuracy would pass every other GPU test.  Here tests/bound_inputs.py crafts key tables and records whose crafted CMux has the
extreme digit in every row at every coefficient against a key whose every word has all 16-bit limbs at magnitude 2^15: the limb sum at
coefficient N - 1 is the bound itself (or the stated fraction of it).  Each case asserts the sum it reached, the kernel that ran, and
every output word against the oracle.  The inputs are not valid ciphertexts; the contract is word equality.  n and the party count are
reduced: the bound depends on neither.  The leveled CMux and rotation kernels (section 4.15) and the encrypted-table instantiations of the
blind rotations (section 4.11) take mask and body from the caller, so their cases load all 2l rows directly -- l = 4, Bgbit = 8 at the full bound."""
import numpy as np
import pytest

import bound_inputs as B
import lut_reference as R
from support import KERNELS, mk_rotate_dev, words

pytestmark = pytest.mark.gpu

SK_KERNELS = [k[1:] for k in KERNELS]   # (coop threshold, ring4 threshold, kernel that does the batch of 12 rotations)


@pytest.mark.parametrize("l, Bgbit, full", [(2, 10, True), (3, 7, True), (3, 10, True), (4, 8, False)],
                         ids=["SK-80", "SK-128", "l3-Bg10", "l4-Bg8-half"])
def test_single_key_at_the_bound(O, l, Bgbit, full):
    # full: step 0 copies the body into the mask, step 1 carries -Bg/2 in all 2l rows (the bound exactly); l = 4, Bgbit = 8 has l Bgbit = 32,
    # so only the l body rows of step 0 are loaded (half the bound)
    import thfhe
    kw = dict(O.PARAM_SETS["SK-128"], n=4, l=l, Bgbit=Bgbit)
    p = O.make_params(**kw)
    K = O.SKKeys(p, 0xB0 + l, 2.0**-25, 2.0**-15)
    bk, x, mu, step = B.sk_case(p, K.bk, full)
    orc = O.Oracle(p, bk, K.ksk)
    reached = B.sk_reached(orc, p, bk, x, mu, step)
    assert reached == B.bound(2 * l, p.N, Bgbit) // (1 if full else 2)
    ref = orc.bootstrap_wo_keyswitch(x, mu)
    xs = np.tile(x, (12, 1))
    ck = thfhe.CloudKey(thfhe.make_params(**kw), bk, K.ksk, device=0)
    try:
        tv = np.full(p.N, mu, np.int32)
        ref_lut = R.lut_bootstrap(orc, [x], (1,), 0, tv, 4, keyswitch=False)
        for coop, ring4, name in SK_KERNELS:
            ck.set_coop_threshold(coop)
            ck.set_ring4_threshold(ring4)
            assert ck.rotation_kernel_name(len(xs)) == name.format(l=l)
            got = ck.bootstrap_wo_keyswitch(xs, mu)
            for g in range(len(xs)):
                assert np.array_equal(got[g], ref), (coop, ring4, g, np.nonzero(got[g] != ref)[0][:8])
            # the LUT instantiations of the same kernels (template flag), four outputs per rotation
            u = ck.lut_bootstrap_wo_keyswitch(tv, xs, theta=4)
            for g in range(len(xs)):
                assert np.array_equal(u[g], ref_lut), (coop, ring4, g)
    finally:
        ck.close()


MK_CASES = [  # (set, kernels by pair threshold, lowest reached fraction of the bound)
    ("MK2", {256: "mk_blind_rotate_coop_kernel<2>", 0: "mk_blind_rotate_pair_kernel<2>"}, 1.0),
    ("MK4", {256: "mk_blind_rotate_coop_kernel<3>", 0: "mk_blind_rotate_pair_kernel<3>"}, 1.0),
    ("MK8", {256: "mk_blind_rotate_coop_kernel<4>"}, 1.0),
    ("MK4-N2048", {256: "mk_blind_rotate_coop2k_kernel<3>", 0: "mk_blind_rotate_pair2k_kernel<3>"}, 1.0),
    # three 9-bit parts (-256, -256, -127): the top part cannot reach 2^8 inside a 26-bit digit
    ("MK16", {256: "mk_blind_rotate_coop2k_kernel<3>", 0: "mk_blind_rotate_pair2k_kernel<3>"}, 0.83),
    ("MK256", {256: "kms_tlev_rotate_kernel", 0: "kms_tlev_rotate_pair_kernel"}, 0.99),
    ("MK64-fft", {256: "r4k_rotate_kernel"}, 0.99),           # 6 row parts x 4096 x 2^8 x 2^15 = 2^37.6
    ("MK512", {256: "r4k_rotate_kernel"}, 0.99),
]


@pytest.mark.parametrize("name, kernels, frac", MK_CASES, ids=[c[0] for c in MK_CASES])
def test_multi_key_at_the_bound(O, name, kernels, frac):
    # the 3-gen CMux with mask and body both loaded (party 0's and the last party's crafted step, one record each): every raw 64-bit
    # accumulator word (thfhe_mk_rotate_partial_dev) and every output word of the bootstrap against the oracle
    import thfhe
    kw = dict(O.PARAM_SETS[name], n=2, parties=2)
    p = O.make_params(**kw)
    K = O.MKKeys(p, 0xB1, 2.0**-30.70, 2.0**-13.52)
    bk, x, mu = B.mk_case(p, K.bk, [0, p.parties - 1], full=True)
    orc = O.MKOracle(p, bk, K.ksk)
    bd = B.bound(2 * p.l, p.N, p.Bgbit)
    accs = []
    for k in range(len(x)):
        acc, steps = B.mk_rotate(orc, p, bk, x[k], mu)
        assert [s[:2] for s in steps] == [([0, p.parties - 1][k], 1)]
        assert steps[0][2] >= frac * bd and steps[0][2] <= bd, (steps, bd)
        accs.append(acc)
    ref_u = np.stack([orc.keyswitch(orc.bootstrap_wo_keyswitch(r, mu)) for r in x])
    ck = thfhe.MKCloudKey(thfhe.make_params(**kw), bk, K.ksk, device=0)
    try:
        for thr, kname in kernels.items():
            ck.set_pair_threshold(thr)
            assert ck.rotation_kernel_name(len(x)) == kname
            got = mk_rotate_dev(ck, p, x, mu)
            for k in range(len(x)):
                assert np.array_equal(got[k], accs[k]), (kname, k, np.argwhere(got[k] != accs[k])[:8])
            assert np.array_equal(ck.bootstrap(x, mu), ref_u), kname
    finally:
        ck.close()


def test_kms_lev_rlwe_mul_at_the_bound(O):
    # mk_lev_rlwe_mul on accumulators whose every word decomposes to -Bg/2 at every lev level, against a TLev whose every word has all four
    # limbs at 2^15: the l_lev-row sums of e and f sit at l_lev N 2^(bg-1) 2^15 exactly
    from thfhe import keygen, kms
    import thfhe
    p = thfhe.make_kms_params("KMS2", n=3)
    K = keygen.KMSSecretKeySet(p, seed=11)
    orc = O.KMSOracle(p, K.gsw, K.uni, K.pk, K.crs, K.ksk)
    ck = kms.KMSCloudKey(p, K.gsw, K.uni, K.pk, K.crs, K.ksk, device=0)
    try:
        acc = np.full((2, p.parties + 1, p.N), B.digit_word(64, p.l_lev, p.bg_lev), np.int64)
        lev = np.full((2, p.l_lev, 2, p.N), B.extreme_key_word(64), np.int64)
        rows = B.decompose(acc[0, 0], 64, p.l_lev, p.bg_lev)
        assert B.peak_limb_sum([(rows[s], lev[0, s, 0]) for s in range(p.l_lev)], 64) == B.bound(p.l_lev, p.N, p.bg_lev)
        party = p.parties - 1
        got = ck.lev_rlwe_mul(party, acc, lev)
        for g in range(2):
            assert np.array_equal(got[g], orc.lev_rlwe_mul(party, acc[g], lev[g])), g
    finally:
        ck.close()


CCS_CASES = [  # (set, overrides, kernel); (P + 1) l 2^(Bgbit-1) = 3072 is the most thfhe_ccs_ctx_create admits
    ("CCS2", dict(n=3, parties=3), "ccs_blind_rotate_kernel"),                  # 4 x 3 x 2^8 = 3072
    ("CCS4", dict(n=3, l=4, Bgbit=7, parties=11), "ccs_blind_rotate_wide_kernel"),   # 12 x 4 x 2^6 = 3072, more than 8 parties
    ("CCS16", dict(n=3, parties=3), "ccs_blind_rotate_wide_kernel"),             # the 16-party gadget (l = 12, Bgbit 2): more than 8 levels
]


@pytest.mark.parametrize("name, over, kernel", CCS_CASES, ids=[c[0] + "-P%d" % c[1]["parties"] for c in CCS_CASES])
def test_ccs_at_the_bound(O, name, over, kernel):
    # CCS CMux with every accumulator polynomial at the extreme digit: stage 1 at l N 2^(Bgbit-1) 2^15 per polynomial, stage 2 at
    # (P + 1) l N 2^(Bgbit-1) 2^15 into the body, exactly; a last CMux on the oracle's own key reads the low bits the crafted one wrote, so
    # the key-switched outputs (the engine's only CCS output) still see an error in the low limb
    import thfhe
    p = O.make_params(name, **over)
    s = O.SIGMAS[name]
    K = O.CCSKeys(p, 0xB2, s["bk"], s["ks"])
    bk, pk, crs, x, mu, step = B.ccs_case(p, K.bk, K.pk, K.crs)
    K.bk[...], K.pk[...], K.crs[...] = bk, pk, crs
    orc = O.CCSOracle(p, K)
    s1, s2 = B.ccs_reached(orc, p, bk, pk, crs, x, mu, step)
    assert s1 == B.bound(p.l, p.N, p.Bgbit) and s2 == B.bound((p.parties + 1) * p.l, p.N, p.Bgbit)
    ref = orc.keyswitch(orc.bootstrap_wo_keyswitch(x, mu))
    ck = thfhe.CCSCloudKey(thfhe.make_params(**p.as_dict()), bk, pk, crs, K.ksk, device=0)
    try:
        assert ck.rotation_kernel_name() == kernel
        got = ck.bootstrap(np.stack([x, x]), mu)
        for g in range(2):
            assert np.array_equal(got[g], ref), (g, np.nonzero(got[g] != ref)[0][:8])
    finally:
        ck.close()


@pytest.fixture(scope="module")
def kms_keys():
    import thfhe
    from thfhe import keygen
    out = {}
    for name in ("KMS2", "KMS4"):
        p = thfhe.make_kms_params(name, n=3, parties=2)
        out[name] = (p, keygen.KMSSecretKeySet(p, seed=11))
    return out


KMS_FRAC = {"KMS2": 0.73, "KMS4": 0.999}   # KMS2: 13-bit gsw digits cut into parts (-64, -31) of 7 bits; KMS4: whole 8-bit digits (the TLev step
# misses the bound only at coefficient 0, where the trivial gadget word sits)


@pytest.mark.parametrize("name", ["KMS2", "KMS4"])
@pytest.mark.parametrize("pair", [256, 0], ids=["single", "paired"])
def test_kms_rotations_at_the_bound(O, kms_keys, name, pair):
    # rlwe_rotate on the accumulator (mu, mu), tlev_rotate and bootstrap_wo_keyswitch with the crafted TLev step (kms_tlev_case), every
    # 64-bit word of the rotations against the oracle; the reached fraction of 2 l_gsw N 2^(part bits - 1) 2^15 asserted per case
    from thfhe import kms
    p, K = kms_keys[name]
    bd = B.bound(2 * p.l_gsw, p.N, p.bg_gsw)
    # RLWE rotation (mk_single_blind_rotate), last party
    gsw, bara, acc = B.kms_rlwe_case(p, K.gsw, 1)
    assert KMS_FRAC[name] * bd <= B.gsw_reached(acc, p.N, gsw[1, 0], p.l_gsw, p.bg_gsw) <= bd
    orc = O.KMSOracle(p, gsw, K.uni, K.pk, K.crs, K.ksk)
    ref = orc.rlwe_rotate(1, bara, acc)
    ck = kms.KMSCloudKey(p, gsw, K.uni, K.pk, K.crs, K.ksk, device=0)
    try:
        ck.set_pair_threshold(pair)
        assert ck.rotation_kernel_name(2) == ("kms_tlev_rotate_kernel" if pair else "kms_tlev_rotate_pair_kernel")
        got = ck.rlwe_rotate(1, np.stack([bara, bara]), np.stack([acc, acc]))
        for g in range(2):
            assert np.array_equal(got[g], ref), g
    finally:
        ck.close()
    # TLev rotation (mk_ith_blind_rotate) and the whole bootstrap, party 0
    gsw, bara = B.kms_tlev_case(p, K.gsw, 0)
    orc = O.KMSOracle(p, gsw, K.uni, K.pk, K.crs, K.ksk)
    init = np.zeros((2, p.N), np.int64)
    init[1, 0] = 1 << (64 - p.bg_lev)
    step0 = np.where(np.arange(p.n) == 0, bara, 0).astype(np.int32)
    assert KMS_FRAC[name] * bd <= B.gsw_reached(orc.rlwe_rotate(0, step0, init), p.N, gsw[0, 1], p.l_gsw, p.bg_gsw) <= bd
    x = np.zeros(p.parties * p.n + 1, np.int32)
    x[:2] = -2**31                              # bara = -N == N (mod 2N) at party 0's steps 0 and 1
    bara = kms.modswitch(x[None], p.N)[0, :p.n]
    assert np.all(bara[:2] % (2 * p.N) == p.N) and not bara[2:].any()
    ref_lev = orc.tlev_rotate(0, bara)
    ref_u = orc.bootstrap_wo_keyswitch(x)
    ck = kms.KMSCloudKey(p, gsw, K.uni, K.pk, K.crs, K.ksk, device=0)
    try:
        ck.set_pair_threshold(pair)
        assert ck.rotation_kernel_name(2 * p.l_lev) == ("kms_tlev_rotate_kernel" if pair else "kms_tlev_rotate_pair_kernel")
        lev = ck.tlev_rotate(0, np.stack([bara, bara]))
        for g in range(2):
            assert np.array_equal(lev[g], ref_lev), g
        u = ck.bootstrap_wo_keyswitch(np.stack([x, x]))
        for g in range(2):
            assert np.array_equal(u[g], ref_u), g
    finally:
        ck.close()


# ---- leveled table lookup (sk_lhe_cmux_kernel<L, PUB>, sk_lhe_rotate_kernel<L>) and the kLutEnc blind rotations ----
# The leveled calls take the TGSW words and both TLWE inputs from the caller: every word of C is extreme_key_word and the difference the CMux
# decomposes is digit_word in mask and body, so all 2l rows are extreme with no key step before -- l = 4, Bgbit = 8 included.
LHE_SHAPES = [(1, 8), (2, 10), (3, 7), (3, 10), (4, 8)]
LHE_IDS = ["l1-Bg8", "SK-80", "SK-128", "l3-Bg10", "l4-Bg8-full"]
BATCH = 12      # identical samples: more than one workgroup per CU pair, every one compared


class _Lhe:
    """One context of the shape (n = 4), its oracle and oracle parameters; close() in a finally."""

    def __init__(self, O, l, Bgbit):
        import thfhe
        kw = dict(O.PARAM_SETS["SK-128"], n=4, l=l, Bgbit=Bgbit)
        self.p = O.make_params(**kw)
        K = O.SKKeys(self.p, 0xB0 + l, 2.0**-25, 2.0**-15)
        self.K, self.orc = K, O.Oracle(self.p, K.bk, K.ksk)
        self.ck = thfhe.CloudKey(thfhe.make_params(**kw), K.bk, K.ksk, device=0)

    def close(self):
        self.ck.close()


def _same_as(got, ref, what):
    """every sample of got (leading axis) equals the one model record set"""
    for g in range(got.shape[0]):
        assert np.array_equal(got[g], ref), (what, g, np.argwhere(got[g] != ref)[:8].tolist())


@pytest.mark.parametrize("l, Bgbit", LHE_SHAPES, ids=LHE_IDS)
def test_lhe_cmux_at_the_bound(O, l, Bgbit):
    # thfhe_lhe_cmux (sk_lhe_cmux_kernel<l, false>, diff_digits_z) with all 2l rows at the extreme digit against extreme key words: first from
    # (d1, d0) = (T, 0), then from (w + T, w) with random words w -- the same digits out of non-zero operands, and an output that adds d0 = w
    import lhe_reference as LR
    E = _Lhe(O, l, Bgbit)
    try:
        p, N = E.p, E.p.N
        C, d1, d0 = B.lhe_cmux_case(p)
        w = words(np.random.default_rng(0xC0 + l), 2 * N)
        with E.ck.tgsw_set(np.tile(C, (BATCH, 1, 1, 1)), 1) as ts:
            for what, (x1, x0) in (("zero d0", (d1, d0)), ("random d0", (LR._add(w, d1), w))):
                assert B.lhe_reached(p, C, LR._sub(x1, x0)) == B.bound(2 * l, N, Bgbit)
                ref = LR.cmux(p, C, x1, x0)
                t1, t0 = np.tile(x1, (BATCH, 1)), np.tile(x0, (BATCH, 1))
                a, b = E.ck.lhe_cmux(ts, 0, t1[:, :N], t1[:, N:], t0[:, :N], t0[:, N:])
                _same_as(np.concatenate([a, b], axis=1), ref, what)
    finally:
        E.close()


@pytest.mark.parametrize("l, Bgbit", LHE_SHAPES, ids=LHE_IDS)
def test_lhe_rotate_at_the_bound(O, l, Bgbit):
    # thfhe_lhe_lookup at d_tree = 0 (sk_lhe_rotate_kernel<l>, rotated_digits_z), theta = 4, the table in mask and body (full bound) and public
    # (zero mask: half).  (a) d_rot 1: step 0 on the spectra loaded before the loop.  (b) d_rot 2, C_0 = 0: the crafted step is step 1, on
    # spectra that arrived through the one-step-ahead requests of step 0 (at l = 4: the fourth row re-requested on entry).  (c) d_rot 2, crafted
    # step 0, then a step on random words that reads the low bits the crafted one wrote.
    import lhe_reference as LR
    E = _Lhe(O, l, Bgbit)
    try:
        p, N = E.p, E.p.N
        bd = B.bound(2 * l, N, Bgbit)
        CK = np.full((2 * l, 2, N), B.extreme_key_word(32), np.int32)
        rnd = words(np.random.default_rng(0xD0 + l), 2 * l, 2, N)
        cases = [  # (name, TGSW samples of the address bits, table shift s, crafted step)
            ("rot1", np.stack([CK]), 512, 0),
            ("rot2-step1", np.stack([np.zeros_like(CK), CK]), 512, 1),
            ("rot2-step0-then-random", np.stack([CK, rnd]), 256, 0),
        ]
        ks_done = False
        for name, Cs, s, step in cases:
            d_rot = Cs.shape[0]
            box = N >> d_rot
            tab = B.lhe_rot_table(p, s)
            assert box << step == s     # the crafted step rotates by the table's segment length, and the steps before it leave ACC alone
            assert not Cs[:step].any()
            kw = dict(d_tree=0, d_rot=d_rot, theta=4)
            with E.ck.tgsw_set(np.tile(Cs, (BATCH, 1, 1, 1, 1)), d_rot) as ts:
                for kind, tab_a, frac in (("enc", tab, 1), ("pub", None, 2)):
                    assert B.lhe_reached(p, Cs[step], B.lhe_rot_diff(tab_a, tab, 2 * N - s)) == bd // frac
                    ref = LR.lookup_wo_keyswitch(p, Cs, tab_a, tab, 0, d_rot, 4)
                    u = E.ck.lhe_lookup_wo_keyswitch(ts, tab, tab_a=tab_a, **kw)
                    assert u.shape == (BATCH, 4, N + 1)
                    _same_as(u, ref, (name, kind))
                    if not ks_done:   # the key-switched call once per shape
                        ks_done = True
                        _same_as(E.ck.lhe_lookup(ts, tab, tab_a=tab_a, **kw), np.stack([E.orc.keyswitch(r) for r in ref]), (name, kind, "keyswitch"))
    finally:
        E.close()


@pytest.mark.parametrize("l, Bgbit", LHE_SHAPES, ids=LHE_IDS)
def test_lhe_public_first_level_at_the_bound(O, l, Bgbit):
    # thfhe_lhe_lookup at (d_tree 1, d_rot 0, theta 1).  Public table with leaves (0, T): sk_lhe_cmux_kernel<l, true>, which issues only the l
    # body rows, all extreme -- l N 2^(Bgbit-1) 2^15.  Its encrypted twin, leaves (0, 0) and (T, T): sk_lhe_cmux_kernel<l, false> through the tree
    # path's strides at the full 2l-row bound.  The N+1-word record carries every coefficient of the output mask column (the peak at coefficient
    # N - 1 is observed there) but of the body coefficient 0 only.
    import lhe_reference as LR
    E = _Lhe(O, l, Bgbit)
    try:
        p, N = E.p, E.p.N
        CK = np.full((1, 2 * l, 2, N), B.extreme_key_word(32), np.int32)
        T = np.full(N, B.digit_word(32, l, Bgbit), np.int64).astype(np.uint32).view(np.int32)
        tab = np.stack([np.zeros(N, np.int32), T])[None]      # [1 table][2 leaves][N]
        with E.ck.tgsw_set(np.tile(CK, (BATCH, 1, 1, 1, 1)), 1) as ts:
            for kind, tab_a, rows in (("pub", None, l), ("enc", tab, 2 * l)):
                diff = np.concatenate([np.zeros(N, np.int32) if tab_a is None else T, T])     # leaf 1 - leaf 0
                assert B.lhe_reached(p, CK[0], diff) == B.bound(rows, N, Bgbit)
                ref = LR.lookup_wo_keyswitch(p, CK, None if tab_a is None else tab_a[0], tab[0], 1, 0, 1)
                u = E.ck.lhe_lookup_wo_keyswitch(ts, tab, tab_a=tab_a, d_tree=1, d_rot=0, theta=1)
                assert u.shape == (BATCH, 1, N + 1)
                _same_as(u, ref, kind)
    finally:
        E.close()


@pytest.mark.parametrize("l, Bgbit", LHE_SHAPES[1:], ids=LHE_IDS[1:])
def test_encrypted_table_bootstrap_at_the_bound(O, l, Bgbit):
    # thfhe_lut_bootstrap_enc (the kLutEnc instantiations of the ring, four-wave ring and cooperative kernels): the accumulator starts as the
    # loaded table (mu, mu), so step 0 -- bara = N, key all extreme words -- has -2 mu = T in mask and body: the full 2l-row bound at step 0,
    # l = 4, Bgbit = 8 included
    import thfhe
    import tree_lut_reference as TR
    kw = dict(O.PARAM_SETS["SK-128"], n=4, l=l, Bgbit=Bgbit)
    p = O.make_params(**kw)
    K = O.SKKeys(p, 0xB0 + l, 2.0**-25, 2.0**-15)
    bk, x, mu = B.lut_enc_case(p, K.bk)
    assert B.lut_enc_reached(p, bk, mu) == B.bound(2 * l, p.N, Bgbit)
    orc = O.Oracle(p, bk, K.ksk)
    tv = np.full(p.N, mu, np.int32)
    ref = TR.lut_enc_wo_keyswitch(orc, x, tv, tv, 4)
    xs = np.tile(x, (BATCH, 1))
    ck = thfhe.CloudKey(thfhe.make_params(**kw), bk, K.ksk, device=0)
    try:
        for coop, ring4, name in SK_KERNELS:
            ck.set_coop_threshold(coop)
            ck.set_ring4_threshold(ring4)
            assert ck.rotation_kernel_name(len(xs)) == name.format(l=l)
            u = ck.lut_bootstrap_enc_wo_keyswitch(tv, tv, xs, theta=4)
            assert u.shape == (BATCH, 4, p.N + 1)
            _same_as(u, ref, (coop, ring4))
    finally:
        ck.close()
