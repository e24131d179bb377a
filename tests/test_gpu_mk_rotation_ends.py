"""The two ends of the 3-gen multi-key rotation at their rounding edges (pytest -m gpu).  Every record here has an
ALL-ZERO MASK: all bara are 0, no CMux runs, the rotation kernels have to hand their start through untouched, and numpy alone gives the expected
words (tests/conv_edges.py; its conditions are checked on the CPU by test_conv_edges_host.py).

  (a) every rotation amount of N = 1024, 2048 and 4096 through lut_bootstrap_wo_keyswitch on each rotation shape: the theta-rounded mod-switch
      (lut_prologue_kernel), the index and sign algebra of mk_lut_acc_init_kernel, the pass through the rotation kernel (the pair kernels' lone
      last job included: every call has an odd job count) and mk_extract_at_kernel, with the ties and wrap-arounds of the mod-switch;
  (b) the same through lut_bootstrap_enc_wo_keyswitch (mk_lut_acc_init_enc_kernel: mask and body start from caller words);
  (c) - (f) the Torus64 -> Torus32 conversion on words that tell it from an exact-integer truncation -- uniform random words never do -- in
      mk_extract_at_kernel, mk_extract_mv_kernel<1024 | 2048 | 4096>, mk_extract_kernel (thfhe_mk_extract_dev) and the extract16_64 fused into
      the N = 1024 coop and pair kernels; (f) also drives mk_prologue_kernel's six gates onto the mod-switch's interval ends;
  (g) the ten rows of the KMS engine's own gate table.

kms_extract_kernel and cb_extract_levels_kernel convert accumulators that come out of rotations under real keys: no entry point sets their words,
and they stay covered by random words only."""
import numpy as np
import pytest

import conv_edges as E
import mk_lut_reference as R
import mk_mv_lut_reference as MV

pytestmark = pytest.mark.gpu

SETS = {"MK2": dict(n=4), "MK4-N2048": dict(n=3, parties=2), "MK256": dict(n=3, parties=2), "MK64-fft": dict(n=2, parties=2)}
KERNELS = {  # id -> (set, pair threshold, kernel, jobs per call at most: odd, and on the one-job-per-workgroup side of the threshold where it counts)
    "coop": ("MK2", 256, "mk_blind_rotate_coop_kernel<2>", 255),
    "pair": ("MK2", 0, "mk_blind_rotate_pair_kernel<2>", 1001),
    "coop2k": ("MK4-N2048", 256, "mk_blind_rotate_coop2k_kernel<3>", 255),
    "pair2k": ("MK4-N2048", 0, "mk_blind_rotate_pair2k_kernel<3>", 1001),
    "tlev": ("MK256", 256, "kms_tlev_rotate_kernel", 255),
    "r4k": ("MK64-fft", 256, "r4k_rotate_kernel", 1001),
}
BY_DEGREE = ["coop", "coop2k", "r4k"]   # one rotation shape per ring degree, each at the context's default threshold


@pytest.fixture(scope="module")
def env(O):
    """kernel id -> (params, context) with the id's pair threshold set; one context per parameter set, closed at the end"""
    import thfhe
    made = {}

    def get(kid):
        name, threshold = KERNELS[kid][:2]
        if name not in made:
            p = O.make_params(name, **SETS[name])
            s = O.SIGMAS[name]
            K = O.MKKeys(p, 0x5EED0000 + len(made), s["bk"], s["ks"])
            made[name] = (p, thfhe.MKCloudKey(thfhe.make_params(**p.as_dict()), K.bk, K.ksk, device=0))
        made[name][1].set_pair_threshold(threshold)
        return made[name]
    yield get
    for p, ck in made.values():
        ck.close()


def odd_calls(total, limit):
    """slices that cut `total` jobs into calls of an odd job count <= limit, as even in size as that allows"""
    k = -(-total // limit)
    k += (k - total) % 2          # a sum of k odd numbers has k's parity
    q, r = divmod((total - k) // 2, k)
    sizes = [1 + 2 * (q + (i < r)) for i in range(k)]
    assert sum(sizes) == total and max(sizes) <= limit and all(s % 2 for s in sizes)
    ends = np.cumsum(sizes)
    return [slice(int(e - s), int(e)) for s, e in zip(sizes, ends)]


def zero_mask(p, bodies):
    """records (0, .., 0, body)"""
    x = np.zeros((len(bodies), p.parties * p.n + 1), np.int32)
    x[:, -1] = bodies
    return x


def operands_for(wanted, weights, bias, rng):
    """body words of len(weights) operands whose weighted sum plus bias is `wanted` mod 2^32; weights = (2^K, .., 2, 1).  The low operands are
    random words with the one bit fixed that keeps the rest divisible; the first takes the quotient and random bits above it."""
    r = (E.to_i32(wanted).astype(np.int64) - bias) & 0xFFFFFFFF
    out = []
    for k, w in reversed(list(enumerate(weights))):
        sh = w.bit_length() - 1
        assert w == 1 << sh and (k == len(weights) - 1 or weights[k + 1] == w >> 1)
        v = rng.integers(0, 1 << 32, len(r))
        if k:
            v = (v & ~np.int64(1)) | ((r >> sh) & 1)
        else:
            v = (r >> sh) + ((v & ((1 << sh) - 1)) << (32 - sh))
        r = (r - (v << sh)) & 0xFFFFFFFF
        out.append(E.to_i32(v))
    assert not r.any()
    return out[::-1]


def reference(N, theta, bar, tv_b, tv_a=None, convert=E.t64tot32):
    """extraction at coefficients 0 .. theta-1 of (X^{-bar} tv_a, X^{-bar} tv_b), per job (tv_a None: a zero mask): int32[jobs][theta][N+1]"""
    body = E.start64(tv_b, bar, N)
    mask = np.zeros_like(body) if tv_a is None else E.start64(tv_a, bar, N)
    acc = np.stack([mask, body], axis=1)
    return np.stack([E.extract_at64(acc, j, N, convert) for j in range(theta)], axis=1)


def call_lut(ck, kind, tabs, recs, **kw):
    if kind == "enc":
        return ck.lut_bootstrap_enc_wo_keyswitch(tabs[0], tabs[1], *recs, **kw)
    return ck.lut_bootstrap_wo_keyswitch(tabs[1], *recs, **kw)


# ---- (a), (b) every rotation amount ---------------------------------------------------------------------------------------------------------

def every_amount(env, kid, theta, kind, weights=(1,), bias=0):
    p, ck = env(kid)
    name, limit, N = KERNELS[kid][2], KERNELS[kid][3], p.N
    rng = np.random.default_rng([N, theta, int(kind == "enc"), len(weights), sorted(KERNELS).index(kid)])
    body = E.amount_words(N, theta, rng)
    body = body[rng.permutation(len(body))]                       # neighbouring jobs of a workgroup get unrelated amounts
    bar = np.array(R.bars(body, N, theta), np.int64)
    seen = set((bar % (2 * N)).tolist())
    assert seen == set(range(0, 2 * N, theta))                    # every amount, and nothing off the theta grid
    recs = [zero_mask(p, b) for b in operands_for(body, weights, bias, rng)]
    assert np.array_equal(np.stack([R.prologue([r[g] for r in recs], weights, bias) for g in range(len(body))]), zero_mask(p, body))
    tabs = rng.integers(-2**63, 2**63, (2, 3, N), dtype=np.int64)   # three tables: (masks, bodies); the plaintext entry takes the bodies
    idx = rng.integers(0, 3, len(body)).astype(np.int32)
    covered = set()
    for sl in odd_calls(len(body), limit):
        count = sl.stop - sl.start
        assert ck.rotation_kernel_name(count) == name
        u = call_lut(ck, kind, tabs, [r[sl] for r in recs], weights=weights, bias=bias, theta=theta, lut_index=idx[sl])
        ref = reference(N, theta, bar[sl], tabs[1][idx[sl]], tabs[0][idx[sl]] if kind == "enc" else None)
        assert u.shape == ref.shape == (count, theta, N + 1)
        bad = np.argwhere(u != ref)
        assert bad.size == 0, ("barb, output, word of the first mismatches", [(int(bar[sl.start + g]), int(j), int(q)) for g, j, q in bad[:6]])
        covered |= set((bar[sl] % (2 * N)).tolist())
    assert covered == seen


@pytest.mark.parametrize("kid,theta", [(k, 1) for k in KERNELS] + [("coop", 2), ("pair2k", 2), ("r4k", 2), ("pair", 4), ("tlev", 4), ("r4k", 4)])
def test_every_amount_random_tables(env, kid, theta):
    every_amount(env, kid, theta, "plain")


@pytest.mark.parametrize("kid,weights", [("coop", (2, 1)), ("pair", (4, 2, 1))])
def test_every_amount_from_a_weighted_sum_that_wraps(env, kid, weights):
    # lut_prologue_kernel's two- and three-input forms: random operands, so the sum wraps many times over, and a bias above 2^31
    every_amount(env, kid, 1, "plain", weights, 0x9E3779B1)


@pytest.mark.parametrize("kid", ["pair", "coop2k", "r4k"])
def test_every_amount_encrypted_tables(env, kid):
    every_amount(env, kid, 1, "enc")


# ---- (c) edge words through mk_extract_at_kernel ----------------------------------------------------------------------------------------------

def spread_amounts(N, rng, count=64):
    """`count` amounts of Z_2N with the ends of both halves among them, as body words that mod-switch to them at theta = 1"""
    fixed = [0, 1, N - 1, N, N + 1, 2 * N - 1]
    rest = rng.choice(np.setdiff1d(np.arange(2 * N), fixed), count - len(fixed), replace=False)
    amounts = rng.permutation(np.concatenate([fixed, rest]))
    return E.to_i32(amounts * E.mod_step(N, 1))


@pytest.mark.parametrize("kind", ["plain", "enc"])
@pytest.mark.parametrize("theta", [1, 4])
@pytest.mark.parametrize("kid", BY_DEGREE)
def test_edge_words_through_the_extraction(env, kid, theta, kind):
    p, ck = env(kid)
    N = p.N
    rng = np.random.default_rng([N, theta, int(kind == "enc")])
    body = spread_amounts(N, rng)
    bar = np.array(R.bars(body, N, theta), np.int64)
    if theta == 1:
        assert {0, 1, N - 1, N, N + 1, 2 * N - 1} <= set((bar % (2 * N)).tolist())
    # every table at another cyclic offset, so that an edge word meets both extraction signs (the list holds every word's negation as well).  A
    # plaintext table gives one converted non-zero word per output -- its tables hold only the words that tell the two conversions apart.
    words = E.edge_words() if kind == "enc" else E.biting_words()
    tabs = np.stack([[E.tiled(words, N, 131 * t + 53 * m) for t in range(3)] for m in range(2)])
    idx = (np.arange(len(body)) % 3).astype(np.int32)
    if kind == "plain":   # ... dealt over the coefficients the jobs extract, so that 64 jobs meet every binade with both signs
        for g in range(len(body)):
            tabs[1, idx[g], (bar[g] + np.arange(theta)) % N] = words[(g * theta + np.arange(theta)) % len(words)]
    ref = reference(N, theta, bar, tabs[1][idx], tabs[0][idx] if kind == "enc" else None)
    raw = reference(N, theta, bar, tabs[1][idx], tabs[0][idx] if kind == "enc" else None, convert=lambda w: w)
    assert E.binades_told_apart(raw) >= set(E.BINADES)             # the comparison below could have failed in every binade
    assert ck.rotation_kernel_name(len(body)) == KERNELS[kid][2]
    u = call_lut(ck, kind, tabs, [zero_mask(p, body)], theta=theta, lut_index=idx)
    bad = np.argwhere(u != ref)
    assert bad.size == 0, ("job, output, word, Torus64 word of the first mismatches", [(int(g), int(j), int(q), int(raw[g, j, q])) for g, j, q in bad[:6]])


# ---- (d) edge words through mk_extract_mv_kernel ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("out_bias", [0, int(E.edge_words()[5])], ids=["no-bias", "edge-bias"])
@pytest.mark.parametrize("kid", BY_DEGREE)
def test_edge_words_through_the_multi_value_epilogue(env, kid, out_bias):
    p, ck = env(kid)
    N = p.N
    rng = np.random.default_rng([N, int(out_bias != 0)])
    body = spread_amounts(N, rng)
    bar = np.array(R.bars(body, N, 1), np.int64)
    x = zero_mask(p, body)
    less_bias = lambda w: E.to_i64(int(v) - out_bias for v in w)     # out_bias is added before the conversion: the sums are the edge words again
    # the sums wanted: words that tell the two conversions apart, dealt over the places the jobs' taps meet (body coefficients N/4 and 3N/4 of
    # X^{-barb} tv0), so that 64 jobs meet every binade with both signs
    bw = E.biting_words()
    one, two = E.tiled(bw, N, 17), E.tiled(bw, N // 2, 29)
    for g, b in enumerate(bar.tolist()):
        one[[(N // 4 + b) % N, (3 * N // 4 + b) % N]] = bw[[2 * g % len(bw), (2 * g + 1) % len(bw)]]
        two[(N // 4 + b) % (N // 2)] = bw[g % len(bw)]
    cases = [("one tap", E.MV_TAPS_ONE, less_bias(one)), ("two taps", E.MV_TAPS_TWO, E.two_tap_base(less_bias(two), rng, N))]
    assert not np.isin(cases[1][2], E.edge_words()).any()          # two taps: only the Torus64 combination lands on an edge word
    for what, taps, tv0 in cases:
        acc = np.concatenate([np.zeros((len(bar), N), np.int64), E.start64(tv0, bar, N)], axis=1)
        ref = np.stack([MV.combine64(a, taps, 2, N, out_bias) for a in acc])
        raw = np.stack([MV.combine64(a, taps, 2, N, out_bias, convert=lambda s: s) for a in acc])
        assert E.binades_told_apart(raw) >= set(E.BINADES), what
        if what == "two taps":   # (a single tap +-1 without a bias converts to the same word in either order: the conversion is odd)
            assert not np.array_equal(ref, np.stack([MV.convert_then_combine(a, taps, 2, N, out_bias) for a in acc]))
        u = ck.mv_lut_bootstrap_wo_keyswitch(taps, x, tv0=tv0, out_bias=out_bias)
        assert u.shape == ref.shape == (len(bar), 4, N + 1)
        bad = np.argwhere(u != ref)
        assert bad.size == 0, (what, "job, output, word, Torus64 sum", [(int(g), int(j), int(q), int(raw[g, j, q])) for g, j, q in bad[:6]])


# ---- (e) thfhe_mk_extract_dev ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kid", BY_DEGREE)
def test_extract_dev_on_edge_words(env, kid):
    import thfhe
    p, ck = env(kid)
    N, count = p.N, 3
    w = E.edge_words()
    acc = np.stack([[E.tiled(w, N, 211 * g + 97 * m) for m in range(2)] for g in range(count)])   # int64[count][2][N], every word an edge word
    ref = E.extract_at64(acc, 0, N)
    assert E.binades_told_apart(E.extract_at64(acc, 0, N, convert=lambda v: v)) >= set(E.BINADES)
    d_acc, d_u = thfhe.DeviceBuffer(ck, acc.nbytes), thfhe.DeviceBuffer(ck, 4 * count * (N + 1))
    try:
        d_acc.upload(acc)
        thfhe._check(thfhe.lib().thfhe_mk_extract_dev(ck.h, d_acc.ptr, d_u.ptr, count))
        ck.sync()
        u = d_u.download((count, N + 1))
    finally:
        d_acc.free()
        d_u.free()
    bad = np.argwhere(u != ref)
    assert bad.size == 0, ("accumulator, word", bad[:6].tolist())


# ---- (f) the fused extraction and the gate prologue ---------------------------------------------------------------------------------------------

def bootstrap_mus():
    """test-vector constants that tell the two conversions apart: two per binade and sign, then both saturating ends"""
    mu = np.concatenate([E.biting_words()[:40], E.to_i64([2**63 - 512, 2**63 - 1, -2**63 + 512])])
    assert len(set(mu.tolist())) == len(mu) >= 32 and E.binades_told_apart(mu) >= set(E.BINADES)
    assert np.all(E.t64tot32(mu[-3:]) == -2**31) and np.all(E.t64tot32(E.neg64(mu)) != E.trunc_shift(E.neg64(mu)))
    return mu


@pytest.mark.parametrize("kid", ["coop", "pair"])
def test_fused_extraction_of_the_bootstrap_on_edge_constants(env, kid):
    # extract16_64 inside the N = 1024 kernels: the accumulator is (0, X^{-barb} (mu, .., mu)), its coefficient 0 is mu for barb in [0, N) and
    # -mu mod 2^64 for barb in [N, 2N); a zero mask key-switches to itself, so the output record is (0, .., 0, t64tot32(+-mu))
    p, ck = env(kid)
    N = p.N
    rng = np.random.default_rng(77)
    assert ck.rotation_kernel_name(2) == KERNELS[kid][2]
    for mu in bootstrap_mus():
        amounts = np.array([rng.integers(0, N), rng.integers(N, 2 * N)])          # one job in each half
        out = ck.bootstrap(zero_mask(p, E.to_i32(amounts * E.mod_step(N, 1))), int(mu))
        ref = zero_mask(p, E.t64tot32(np.array([mu, E.neg64([mu])[0]])))
        assert np.array_equal(out, ref), (int(mu), amounts.tolist(), out[:, -1].tolist(), ref[:, -1].tolist())


E8, E4 = 1 << 29, 1 << 30
# (constant, x, y, z) of the gate's linear part, 3-gen-mk-tfhe/src/3gen_mk_gates.jl:8-14 (NAND), 24-30 (OR), 40-46 (AND), 68-74 (XOR), 55-64 (AND3);
# MUX (133-150) is AND(x, y) and AND(-x, z), then (0, 1/8) + t1 + t2 on the key-switched records
GATE_LIN = {"NAND": (E8, -1, -1, 0), "OR": (E8, 1, 1, 0), "AND": (-E8, 1, 1, 0), "XOR": (E4, 2, 2, 0), "AND3": (-E4, 1, 1, 1)}
MUX_LIN = ((-E8, 1, 1, 0), (-E8, -1, 0, 1))


def gate_sign(O, lin, ops, N):
    """(+-2^29 per gate: t64tot32(+-2^61) by the half the mod-switched body falls in, the body words themselves)"""
    v = E.to_i32(lin[0] + sum(c * o.astype(np.int64) for c, o in zip(lin[1:], ops)))
    bar = np.array([O.lib().oracle_modswitch(int(w), N) for w in v]) % (2 * N)
    return np.where(bar < N, E8, -E8), v


@pytest.mark.parametrize("kid", BY_DEGREE)
def test_gate_prologues_on_the_interval_ends(O, env, kid):
    import thfhe
    p, ck = env(kid)
    N = p.N
    rng = np.random.default_rng(N + 5)
    ends = E.interval_ends(N, 1)[:14]                               # around 0 and around 1/2: where the output's sign changes
    assert ck.rotation_kernel_name(2 * len(ends)) == KERNELS[kid][2]
    rand = lambda: E.to_i32(rng.integers(0, 1 << 32, len(ends)))
    for name, lin in GATE_LIN.items():
        y, z = rand(), rand()
        if name == "XOR":                                           # 2 (x + y) reaches the even words: each end's even neighbours
            want = E.to_i32(ends.astype(np.int64) & ~np.int64(1))
            x = E.to_i32((((want.astype(np.int64) - lin[0]) & 0xFFFFFFFF) >> 1) - y + (rng.integers(0, 2, len(ends)) << 31))
        else:
            want = ends
            x = E.to_i32(lin[1] * (want.astype(np.int64) - lin[0] - lin[2] * y.astype(np.int64) - lin[3] * z.astype(np.int64)))
        sign, v = gate_sign(O, lin, (x, y, z), N)
        assert np.array_equal(v, want) and {E8, -E8} == set(sign.tolist())
        args = [zero_mask(p, o) for o in ((x, y, z) if lin[3] else (x, y))]
        out = ck.gates(getattr(thfhe, name), *args)
        assert np.array_equal(out, zero_mask(p, sign)), (name, np.flatnonzero(out[:, -1] != sign).tolist(), v.tolist())
    # MUX: both rotations on the ends, the second one's in another order
    w1, w2 = ends, ends[rng.permutation(len(ends))]
    x = rand()
    y, z = E.to_i32(w1.astype(np.int64) + E8 - x), E.to_i32(w2.astype(np.int64) + E8 + x)
    (s1, v1), (s2, v2) = gate_sign(O, MUX_LIN[0], (x, y, z), N), gate_sign(O, MUX_LIN[1], (x, y, z), N)
    assert np.array_equal(v1, w1) and np.array_equal(v2, w2)
    out = ck.gates(thfhe.MUX, zero_mask(p, x), zero_mask(p, y), zero_mask(p, z))
    assert np.array_equal(out, zero_mask(p, E8 + s1 + s2)), ("MUX", v1.tolist(), v2.tolist())


# ---- (g) the KMS engine's gate table -------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def kms2(O):
    import thfhe
    from thfhe import keygen, kms
    p = thfhe.make_kms_params("KMS2", n=12)
    K = keygen.KMSSecretKeySet(p, seed=7)
    ck = kms.KMSCloudKey(p, K.gsw, K.uni, K.pk, K.crs, K.ksk, device=0)
    yield K, O.KMSOracle(p, K.gsw, K.uni, K.pk, K.crs, K.ksk), ck
    ck.close()


@pytest.mark.parametrize("fast_boot", [False, True])
def test_kms_gate_table_row_by_row(O, kms2, fast_boot):
    # kKmsLin (thfhe_kms.hip) is a table of its own, apart from gate_lin / mk_gate_lin: all ten rows on the four input pairs, word for word against
    # the oracle and -- independent of the oracle -- decrypted against the truth table
    K, orc, ck = kms2
    a, b = np.array([0, 0, 1, 1]), np.array([0, 1, 0, 1])
    ca, cb = K.encrypt(a, 61), K.encrypt(b, 62)
    for op in range(O.NAND, O.ORYN + 1):
        out = ck.gates(op, ca, cb, fast_boot=fast_boot)
        assert np.array_equal(K.decrypt(out), [bool(O.TRUTH[op](bool(u), bool(v))) for u, v in zip(a, b)]), op
        assert np.array_equal(out, orc.gates(op, ca, cb, fast_boot=fast_boot)), op
