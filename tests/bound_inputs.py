"""Inputs that drive the split-limb FP64 products to the exactness bound of DESIGN.md section 3 -- TEST INFRASTRUCTURE ONLY.

Every limb product sum of a CMux is an integer with |S| <= rows * N * 2^(digit bits - 1) * 2^15.  Random keys and accumulators stay 6 - 8 bits
below that; the recipe here reaches it through the public bootstrap calls:

* body = 0, every mask word 0 except a_i = 2^31 at the crafted step: bara_i = N, so X^bara acc - acc = -2 acc;
* mu = -x / 2 with x = digit_word(...): the body row of every level decomposes to the extreme digit at all N coefficients;
* every key coefficient of the crafted step = extreme_key_word(...): all 16-bit limbs at magnitude 2^15, so the sum at coefficient N - 1
  is coherent (l N 2^(Bgbit-1) 2^15 per limb from the body rows alone: half the bound);
* full bound: one step earlier, a key whose only non-zero coefficient is w X^0 in the body row of level 1, mask column, makes the mask
  equal to the body; the crafted step then has the extreme digit in all 2l rows;
* the leveled calls (thfhe_lhe_cmux, thfhe_lhe_lookup) and the encrypted-table bootstrap take mask and body from the caller: all 2l rows are
  loaded directly (lhe_cmux_case, lhe_rot_table, lut_enc_case), which reaches the full bound at l Bgbit = 32 too.

These are not valid ciphertexts: the contract under test is word equality with the oracle.  reached(...) recomputes, with Python integers,
the per-limb sum the crafted step really produces at its peak coefficient from the oracle's own decomposition."""
import numpy as np

import oracle_lib as O


def wrap(v, bits):
    """v as a signed `bits`-bit integer."""
    v &= (1 << bits) - 1
    return v - (1 << bits) if v >> (bits - 1) else v


# ---- the balanced 16-bit limb split of thfhe_lane.h (split_limbs32 / split_limbs64) --------------------------------------------
def split_limbs32(v):
    v = wrap(int(v), 32)
    lo = wrap(v, 16)
    return lo, (v - lo) >> 16


def split_limbs64(v):
    v = wrap(int(v), 64)
    out = []
    for _ in range(3):
        lo = wrap(v, 16)
        out.append(lo)
        v = wrap(v - lo, 64) >> 16      # int64 arithmetic: 2^63 - 1 splits to (-1, 0, 0, -2^15)
    return out + [v]


def split_limbs(v, bits):
    return split_limbs32(v) if bits == 32 else split_limbs64(v)


def extreme_key_word(bits):
    """A key word whose limbs all have magnitude 2^15: Torus32 0x7FFF8000 = (-2^15, +2^15); Torus64 (-2^15, -2^15, -2^15, +2^15)."""
    limbs = [-(1 << 15)] * (bits // 16 - 1) + [1 << 15]
    return wrap(sum(x << (16 * h) for h, x in enumerate(limbs)), bits)


# ---- gadget decomposition (oracle_decompose32/64) and the digit-part cut of the wide-base N = 2048 / 4096 kernels ------------------
def decomp_offset(bits, l, Bgbit):
    return sum((1 << (Bgbit - 1)) << (bits - p * Bgbit) for p in range(1, l + 1)) & ((1 << bits) - 1)


def digit_parts(Bgbit):
    """(parts, part width) of thfhe_mk_ctx_create: digits above 10 bits are cut into balanced parts of at most 9 bits."""
    parts = (Bgbit + 8) // 9 if Bgbit > 10 else 1
    return parts, ((Bgbit + parts - 1) // parts if parts > 1 else 0)


def cut_parts(v, parts, pw):
    """Balanced parts of a digit, least significant first (p2k_pack / r4k_group_digits)."""
    if parts == 1:
        return [v]
    hp, mp = 1 << (pw - 1), (1 << pw) - 1
    out = []
    for _ in range(parts - 1):
        lo = ((v + hp) & mp) - hp
        out.append(lo)
        v = (v - lo) >> pw
    return out + [v]


def extreme_digit(Bgbit):
    """The digit whose (balanced) parts all sit at their most negative value inside the digit range [-2^(Bgbit-1), 2^(Bgbit-1))."""
    parts, pw = digit_parts(Bgbit)
    half = 1 << (Bgbit - 1)
    if parts == 1:
        return -half
    low = sum(-(1 << (pw - 1)) << (pw * w) for w in range(parts - 1))
    top = -((half + low) >> (pw * (parts - 1)))        # most negative top part with low + top 2^(pw (parts-1)) >= -half
    return low + top * (1 << (pw * (parts - 1)))


def digit_word(bits, l, Bgbit):
    """The word whose decomposition puts extreme_digit(Bgbit) at every level."""
    d = extreme_digit(Bgbit) + (1 << (Bgbit - 1))
    t = sum(d << (bits - p * Bgbit) for p in range(1, l + 1))
    return wrap(t - decomp_offset(bits, l, Bgbit), bits)


def decompose(poly, bits, l, Bgbit):
    """The oracle's decomposition of one polynomial: int64[l][N]."""
    poly = np.asarray(poly)
    N = poly.shape[-1]
    if bits == 32:
        out = np.zeros(l * N, np.int32)
        O.lib().oracle_decompose32(O.p32(np.ascontiguousarray(poly, np.int32)), N, l, Bgbit, O.p32(out))
    else:
        out = np.zeros(l * N, np.int64)
        O.lib().oracle_decompose64(O.p64(np.ascontiguousarray(poly, np.int64)), N, l, Bgbit, O.p64(out))
    return out.reshape(l, N).astype(np.int64)


def bound(rows, N, Bgbit):
    """The largest limb sum the parameter checks allow: rows * N * 2^(part bits - 1) * 2^15, rows counting every digit part."""
    parts, pw = digit_parts(Bgbit)
    return rows * parts * N * (1 << ((pw if parts > 1 else Bgbit) - 1)) * (1 << 15)


def solve_mul(d, c, bits):
    """An integer w with d * w == c (mod 2^bits)."""
    M = 1 << bits
    d, c = d % M, c % M
    tz = (d & -d).bit_length() - 1
    assert c % (1 << tz) == 0, (d, c)
    m = M >> tz
    return wrap(((c >> tz) * pow(d >> tz, -1, m)) % m, bits)


def crafted_mu(bits, l, Bgbit):
    """mu with -2 mu == digit_word: the accumulator value whose step difference decomposes to extreme digits."""
    x = digit_word(bits, l, Bgbit)
    assert x % 2 == 0
    return wrap(((-x) % (1 << bits)) >> 1, bits)


# ---- reached limb sums ---------------------------------------------------------------------------------------------------------
def peak_limb_sum(pairs, bits):
    """max over limbs h of |sum over (digits, key) pairs of sum_j digits[j] * limb_h(key[N-1-j])|: the limb sums at coefficient N - 1
    (no negacyclic wrap there).  pairs: (digit polynomial, key polynomial) of one output polynomial."""
    H = bits // 16
    S = [0] * H
    for d, k in pairs:
        d = [int(v) for v in np.asarray(d)]
        N = len(d)
        limbs = {}
        for j in range(N):
            if d[j] == 0:
                continue
            kw = int(k[N - 1 - j])
            if kw not in limbs:
                limbs[kw] = split_limbs(kw, bits)
            for h in range(H):
                S[h] += d[j] * limbs[kw][h]
    return max(abs(s) for s in S)


def step_digit_rows(acc, bara, bits, l, Bgbit):
    """Digit rows (j * l + level, each cut into its parts) of the CMux difference X^bara acc - acc: list of (row, part, digits)."""
    N = acc.shape[-1]
    diff = np.zeros_like(acc)
    fn = O.lib().oracle_mul_by_monomial32 if bits == 32 else O.lib().oracle_mul_by_monomial64
    ptr = O.p32 if bits == 32 else O.p64
    parts, pw = digit_parts(Bgbit)
    rows = []
    for j in range(2):
        src = np.ascontiguousarray(acc[j])
        fn(ptr(src), int(bara), N, ptr(diff[j]))
        dj = decompose(diff[j] - src, bits, l, Bgbit)
        for lev in range(l):
            cut = np.array([cut_parts(int(v), parts, pw) for v in dj[lev]], np.int64)
            for w in range(parts):
                rows.append((j * l + lev, w, cut[:, w]))
    return rows


def shifted(key, pw, w, bits):
    """The key row multiplied by 2^(pw w) mod 2^bits (the copy a digit part multiplies, mk_expand_parts_kernel)."""
    return [wrap(int(v) << (pw * w), bits) for v in key]


# ---- single key --------------------------------------------------------------------------------------------------------------
def sk_case(p, bk, full):
    """Crafted single-key bootstrap: returns (bk', x, mu, step) -- step is the index of the CMux at the bound.  full: all 2l rows (needs
    l Bgbit <= 31); otherwise the l body rows of step 0."""
    N, l, Bgbit = p.N, p.l, p.Bgbit
    bk = np.array(bk, np.int32, copy=True)
    mu = crafted_mu(32, l, Bgbit)
    x = np.zeros(p.n + 1, np.int32)
    x[0] = -2**31
    step = 0
    if full:
        assert l * Bgbit <= 31
        step = 1
        x[1] = -2**31
        bk[0] = 0
        bk[0, l, 0, 0] = solve_mul(extreme_digit(Bgbit), mu, 32)   # body row, level 1, mask column: mask after step 0 = mu
    bk[step] = extreme_key_word(32)
    return bk, x, mu, step


def sk_acc_before(orc, p, x, mu, step):
    """The accumulator entering CMux `step` (the oracle's own steps before it; barb = 0)."""
    acc = np.zeros((2, p.N), np.int32)
    acc[1] = mu
    for i in range(step):
        b = O.lib().oracle_modswitch(int(x[i]), p.N)
        if b:
            acc = orc.mux_rotate(i, b, acc, schoolbook=True)
    return acc


def sk_reached(orc, p, bk, x, mu, step):
    """Exact peak limb sum of CMux `step` of the crafted single-key bootstrap, largest over the two output columns."""
    acc = sk_acc_before(orc, p, x, mu, step)
    bara = O.lib().oracle_modswitch(int(x[step]), p.N)
    rows = step_digit_rows(acc, bara, 32, p.l, p.Bgbit)
    return max(peak_limb_sum([(d, bk[step, r, c]) for r, _, d in rows], 32) for c in range(2))


# ---- 3-gen multi-key ---------------------------------------------------------------------------------------------------------
def mk_key_word(Bgbit):
    """Torus64 key word for the 3-gen kernels: extreme_key_word(64) for whole digits; for digit parts, a word whose shifted copies
    (2^(pw w) K) share one limb near 2^15 with the same sign (hill climb over single bit flips from the extreme word, deterministic)."""
    parts, pw = digit_parts(Bgbit)
    K = extreme_key_word(64)
    if parts == 1:
        return K
    signs = [1 if v < 0 else -1 for v in cut_parts(extreme_digit(Bgbit), parts, pw)]

    def score(k):
        best = 0
        for h in range(4):
            best = max(best, abs(sum(s * split_limbs64(wrap(k << (pw * w), 64))[h] for w, s in enumerate(signs))))
        return best
    cur = score(K)
    improved = True
    while improved:
        improved = False
        for b in range(64):
            k2 = wrap(K ^ (1 << b), 64)
            s2 = score(k2)
            if s2 > cur:
                K, cur, improved = k2, s2, True
    return K


def mk_case(p, bk, parties, full):
    """Crafted 3-gen bootstrap: every party q in `parties` gets the crafted key steps, and record x[k] runs the crafted CMux of parties[k]
    alone (its step 0 -- or, full, step 1 after a step-0 key that copies the body into the mask).  Returns (bk', x, mu)."""
    l, Bgbit = p.l, p.Bgbit
    bk = np.array(bk, np.int64, copy=True)
    mu = crafted_mu(64, l, Bgbit)
    x = np.zeros((len(parties), p.parties * p.n + 1), np.int32)
    K = mk_key_word(Bgbit)
    for k, q in enumerate(parties):
        i = 1 if full else 0
        x[k, q * p.n + i] = -2**31
        bk[q, i] = K
        if full:
            x[k, q * p.n] = -2**31
            bk[q, 0] = 0
            bk[q, 0, 3, 0, 0] = solve_mul(extreme_digit(Bgbit), mu, 64)   # P4 (g(c0) -> mask), level 1: mask after this step = mu
    return bk, x, mu


def mk_rotate(orc, p, bk, x, mu):
    """The oracle's 3-gen blind rotation of one crafted record (barb = 0), and the exact peak limb sum of every CMux whose key is one
    constant word: (acc int64[2][N], [(party, i, reached)])."""
    N, l, Bgbit = p.N, p.l, p.Bgbit
    parts, pw = digit_parts(Bgbit)
    acc = np.zeros((2, N), np.int64)
    acc[1] = mu
    out = []
    for q in range(p.parties):
        for i in range(p.n):
            b = O.lib().oracle_modswitch(int(x[q * p.n + i]), N)
            if not b:
                continue
            if np.all(bk[q, i] == bk[q, i, 0, 0, 0]):
                rows = step_digit_rows(acc, b, 64, l, Bgbit)
                key = {w: shifted(bk[q, i, 0, 0], pw, w, 64) for w in range(parts)}
                out.append((q, i, peak_limb_sum([(d, key[w]) for _, w, d in rows], 64)))
            acc = orc.mux_rotate(q, i, b, acc, schoolbook=True)
    return acc, out


def gsw_reached(acc, bara, key, l, Bgbit):
    """Exact peak limb sum of one Torus64 RLWE x TGSW CMux (digit rows j * l + level, key int64[2l][2][N]), largest over the two outputs."""
    parts, pw = digit_parts(Bgbit)
    rows = step_digit_rows(acc, bara, 64, l, Bgbit)
    return max(peak_limb_sum([(d, shifted(key[r, c], pw, w, 64)) for r, w, d in rows], 64) for c in range(2))


# ---- CCS (UniProduct_old, oracle_ccs_uniproduct) -----------------------------------------------------------------------------
# stage 1: u_i = g(a_i) . d, v_i = g(a_i) . pk_i (i < P), v_P = -g(b) . crs; stage 2: b += sum_i g(v_i) . f0, a_party += sum_i g(v_i) . f1 --
# the stage-2 sums run over (P + 1) l digit rows, the widest of any engine
def ccs_case(p, bk, pk, crs):
    """Crafted CCS bootstrap (n >= 3): pk and crs are w X^0 at level 1, so every non-zero accumulator polynomial of a step yields
    v_i = digit_word; step 0 of party q (key d = f0 = 0, f1 = w_q X^0 at level 1) sets a_q = mu; step 1 of the last party then has all
    P + 1 polynomials at mu and key words 0x7FFF8000: both stages carry the extreme digit in every row.  Step 2 of the last party (the
    oracle's own key) reads the low bits the crafted step wrote.  Returns (bk', pk', crs', x, mu, (party, step))."""
    P, n, l, Bgbit = p.parties, p.n, p.l, p.Bgbit
    assert n >= 3
    bk, pk, crs = (np.array(a, np.int32, copy=True) for a in (bk, pk, crs))
    e, T, mu = extreme_digit(Bgbit), digit_word(32, l, Bgbit), crafted_mu(32, l, Bgbit)
    pk[...] = 0
    pk[:, 0, 0] = solve_mul(e, T, 32)
    crs[...] = 0
    crs[0, 0] = solve_mul(-e, T, 32)
    x = np.zeros(P * n + 1, np.int32)
    for q in range(P):           # a_0 .. a_(q-1) and b are at mu when party q's step 0 runs: q + 1 polynomials feed f1
        bk[q, 0] = 0
        bk[q, 0, 2, 0, 0] = solve_mul((q + 1) * e, mu, 32)
        x[q * n] = -2**31
    bk[P - 1, 1] = extreme_key_word(32)
    x[(P - 1) * n + 1] = -2**31
    x[(P - 1) * n + 2] = 0x2468ACE0
    return bk, pk, crs, x, mu, (P - 1, 1)


def ccs_reached(orc, p, bk, pk, crs, x, mu, step):
    """Exact peak limb sums (stage 1, stage 2) of CCS CMux `step` = (party, j) of the crafted bootstrap: stage 1 over the l rows of one
    polynomial, stage 2 over all (P + 1) l rows into the body."""
    P, n, N, l, Bgbit = p.parties, p.n, p.N, p.l, p.Bgbit
    acc = np.zeros((P + 1, N), np.int32)
    acc[P] = mu
    for q in range(P):
        for j in range(n):
            b = O.lib().oracle_modswitch(int(x[q * n + j]), N)
            if not b:
                continue
            if (q, j) == step:
                diff = np.zeros_like(acc)
                for i in range(P + 1):
                    O.lib().oracle_mul_by_monomial32(O.p32(np.ascontiguousarray(acc[i])), b, N, O.p32(diff[i]))
                diff = diff - acc
                dig = [decompose(diff[i], 32, l, Bgbit) for i in range(P + 1)]
                s1 = max(peak_limb_sum([(dig[i][lev], bk[q, j, 0, lev]) for lev in range(l)], 32) for i in range(P + 1))
                v = np.zeros((P + 1, N), np.int64)
                prod = np.zeros(N, np.int32)
                for i in range(P + 1):
                    key = pk[i] if i < P else crs
                    for lev in range(l):
                        O.lib().oracle_polymul_schoolbook32(O.p32(np.ascontiguousarray(dig[i][lev], np.int32)), O.p32(np.ascontiguousarray(key[lev])), N, O.p32(prod))
                        v[i] += prod
                v[P] = -v[P]
                dv = [decompose(v[i].astype(np.int32), 32, l, Bgbit) for i in range(P + 1)]
                s2 = peak_limb_sum([(dv[i][lev], bk[q, j, 1, lev]) for i in range(P + 1) for lev in range(l)], 32)
                return s1, s2
            acc = orc.mux_rotate(q, j, b, acc, schoolbook=True)
    raise ValueError("step not in the record")


# ---- KMS (mk_single_blind_rotate / mk_ith_blind_rotate, oracle_kms_rlwe_rotate) ---------------------------------------------------
def kms_rlwe_case(p, gsw, party):
    """Crafted RLWE rotation: the accumulator (mu, mu) and the key of step 0 = mk_key_word(bg_gsw): all 2 l_gsw rows extreme.
    Returns (gsw', bara int32[n], acc int64[2][N])."""
    gsw = np.array(gsw, np.int64, copy=True)
    gsw[party, 0] = mk_key_word(p.bg_gsw)
    bara = np.zeros(p.n, np.int32)
    bara[0] = p.N
    return gsw, bara, np.full((2, p.N), crafted_mu(64, p.l_gsw, p.bg_gsw), np.int64)


def kms_tlev_case(p, gsw, party):
    """Crafted TLev rotation (n >= 2): TLev sample 0 starts at (0, 2^(64 - bg_lev) X^0); the step-0 key (one body row, both columns the
    constant w) turns it into (mu, mu + that gadget word at X^0), and step 1 (mk_key_word) has every row extreme except at coefficient 0.
    The other samples run through the same keys.  Returns (gsw', bara int32[n])."""
    N, lg, bg = p.N, p.l_gsw, p.bg_gsw
    gsw = np.array(gsw, np.int64, copy=True)
    mu = crafted_mu(64, lg, bg)
    body = np.zeros(N, np.int64)
    body[0] = wrap(-2 * (1 << (64 - p.bg_lev)), 64)
    d0 = decompose(body, 64, lg, bg)[:, 0]
    lev = next(q for q in range(lg) if d0[q] != 0)
    gsw[party, 0] = 0
    gsw[party, 0, lg + lev] = solve_mul(int(d0[lev]), mu, 64)
    gsw[party, 1] = mk_key_word(bg)
    bara = np.zeros(p.n, np.int32)
    bara[:2] = N
    return gsw, bara


# ---- leveled table lookup (thfhe_lhe_cmux / thfhe_lhe_lookup) ----------------------------------------------
# The leveled calls take the TGSW words and both TLWE inputs from the caller, so all 2l rows are loaded directly -- no key step that copies the
# body into the mask -- and l Bgbit = 32 reaches the full bound too.  A TLWE sample is int32[2N] = (mask, body) as in lhe_reference.py.
def _i32(v):
    return (np.asarray(v, np.int64) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)


def lhe_cmux_case(p):
    """Crafted leveled CMux: (C int32[2l][2][N] with every word extreme_key_word, d1 int32[2N] with every word digit_word, d0 = 0): the
    difference d1 - d0 decomposes to the extreme digit in all 2l rows at every coefficient."""
    C = np.full((2 * p.l, 2, p.N), extreme_key_word(32), np.int32)
    d1 = _i32(np.full(2 * p.N, digit_word(32, p.l, p.Bgbit), np.int64))
    return C, d1, np.zeros(2 * p.N, np.int32)


def lhe_rot_table(p, s):
    """The table polynomial int32[N] whose rotation step by s = N / m has the difference digit_word everywhere: segment r (coefficients
    r s .. (r + 1) s - 1) holds q_r = (r - m / 2) T.  X^(2N - s) ACC - ACC is q_(r+1) - q_r = T inside, and -q_0 - q_(m-1) = T in the last
    segment (the wrap negates).  s = 512: (-T, 0); s = 256: (-2T, -T, 0, T)."""
    m = p.N // s
    assert m >= 2 and m * s == p.N
    T = digit_word(32, p.l, p.Bgbit)
    return _i32(np.repeat([(r - m // 2) * T for r in range(m)], s))


def lhe_reached(p, C, diff):
    """Exact peak limb sum of the external product C (.) diff (C int32[2l][2][N], diff int32[2N] = (mask, body)) over all 2l rows, the larger
    of the two output columns."""
    N, l = p.N, p.l
    diff = np.asarray(diff, np.int32)
    digits = np.concatenate([decompose(diff[:N], 32, l, p.Bgbit), decompose(diff[N:], 32, l, p.Bgbit)])
    return max(peak_limb_sum([(digits[r], C[r][c]) for r in range(2 * l)], 32) for c in range(2))


def lhe_rot_diff(tab_a, tab_b, shift):
    """X^shift ACC - ACC of the accumulator (tab_a, tab_b) (tab_a None: zero mask) -> int32[2N], the difference a rotation step decomposes."""
    N = len(tab_b)
    out = np.zeros(2 * N, np.int32)
    rot = np.zeros(N, np.int32)
    for j, t in enumerate((tab_a, tab_b)):
        if t is None:
            continue
        t = np.ascontiguousarray(t, np.int32)
        O.lib().oracle_mul_by_monomial32(O.p32(t), int(shift), N, O.p32(rot))
        out[j * N:(j + 1) * N] = _i32(rot.astype(np.int64) - t)
    return out


# ---- encrypted-table bootstrap (thfhe_lut_bootstrap_enc) ---------------------------------------------------
def lut_enc_case(p, bk):
    """Crafted encrypted-table bootstrap: tables tv_a = tv_b = mu everywhere, a_0 = 2^31 (bara_0 = N at every theta), body 0, step-0 key all
    extreme_key_word: the accumulator starts as (mu, mu), so step 0 itself has -2 mu = digit_word in mask and body -- all 2l rows, with no
    key step before it.  Returns (bk', x, mu)."""
    bk = np.array(bk, np.int32, copy=True)
    bk[0] = extreme_key_word(32)
    x = np.zeros(p.n + 1, np.int32)
    x[0] = -2**31
    return bk, x, crafted_mu(32, p.l, p.Bgbit)


def lut_enc_reached(p, bk, mu):
    """Exact peak limb sum of step 0 of lut_enc_case, largest over the two output columns."""
    rows = step_digit_rows(np.full((2, p.N), mu, np.int32), p.N, 32, p.l, p.Bgbit)
    return max(peak_limb_sum([(d, bk[0, r, c]) for r, _, d in rows], 32) for c in range(2))


# ---- multi-value bootstrap (the kLutMv instantiations of the blind rotations) -------------------------------------------
# kLutMv starts like kLut, with the accumulator (0, X^{-barb} tv0): tv0 = mu everywhere, one input of weight 1 and bias 0 make the rotation of
# sk_case(p, bk, full) the gate's, so sk_reached(...) is the limb sum of its crafted step too.  What differs is the epilogue: output j is the
# integer combination of the extractions at the p tap coefficients N - box/2 - k box.
def sk_acc_after(orc, p, x, mu):
    """The accumulator after the last CMux of the crafted single-key bootstrap (the oracle's schoolbook steps), int32[2N] = (mask, body)."""
    return sk_acc_before(orc, p, x, mu, p.n).reshape(-1)


def mv_factors(rng, n_tables, q, pt):
    """Factor tables int32[n_tables][q][pt] for the bound cases: output 0 of table t is the single unit tap at k = (pt - 1 - t) mod pt, so its
    record is minus one plain extraction and shows every bit of the accumulator's mask (an even tap would hide bit 0 behind the product); the
    other outputs are random int32 taps."""
    w = rng.integers(-2**31, 2**31, size=(n_tables, q, pt), dtype=np.int64).astype(np.int32)
    for t in range(n_tables):
        w[t, 0] = 0
        w[t, 0, (pt - 1 - t) % pt] = 1
    return w


def mv_tap_positions(N, pt):
    """the body coefficients an output record of a pt-tap factor table reads"""
    box = N // pt
    return [N - box // 2 - k * box for k in range(pt)]


# ---- layered automata (sk_lhe_wfa_step_kernel<L, PUB>) ------------------------------------------------------------------
def wfa_case(p, n_states, rng=None):
    """One step of an automaton whose every non-copy state is the CMux of lhe_cmux_case: returns (C int32[2l][2][N], fin int32[n_states][2N],
    trans int32[n_states][2]).  The finals hold d0 in the even states and d1 = d0 + digit_word in the odd ones; trans[q] = (2 floor(q/2),
    2 floor(q/2) + 1) except for the last state, a copy of itself.  rng None: d0 = 0; else every pair (and the copy state) gets random words w of
    its own, (d1, d0) = (w + T, w): the same digits out of non-zero operands, and states that differ from each other.  fin[:, :N] are the masks
    (fin_a), fin[:, N:] the bodies; the public variant passes the bodies alone and reaches the l-row sum."""
    C, d1, _ = lhe_cmux_case(p)
    fin = np.zeros((n_states, 2 * p.N), np.int32)
    for q in range(0, n_states, 2):
        if rng is not None:
            fin[q] = rng.integers(-2**31, 2**31, size=2 * p.N, dtype=np.int64).astype(np.int32)
        if q + 1 < n_states:
            fin[q + 1] = _i32(fin[q].astype(np.int64) + d1)
    trans = np.array([[q & ~1, q | 1] for q in range(n_states)], np.int32)
    trans[n_states - 1] = n_states - 1
    return C, fin, trans


def wfa_copies(n_states):
    """a step whose every state is a copy of itself: the layer it writes holds the layer (or the finals) it read"""
    return np.repeat(np.arange(n_states, dtype=np.int32)[:, None], 2, axis=1)


# the automata of tests/test_gpu_wfa_bound.py (and of the CPU checks of the same cases in tests/test_bound_inputs.py): 5 states, the step bits name
# bit 0 (every word extreme_key_word) and bit 1 (random words) of one set
WFA_STATES = 5
WFA_FOLLOW = np.array([[0, 1], [1, 2], [2, 3], [3, 4], [4, 0]], np.int32)   # every state of the layer below is the d0 of one CMux, so its low bits reach an output


def wfa_bound_automata(p):
    """name -> (trans int32[n_steps][5][2], step_bit): the crafted step alone on the finals; the crafted step as the non-final layer above a step
    of copies (it reads the layer buffer); the crafted step on the finals, then a step on the random bit that reads what it wrote."""
    tr = wfa_case(p, WFA_STATES)[2]
    return {
        "one-step": (tr[None], [0]),
        "reads-a-layer": (np.stack([tr, wfa_copies(WFA_STATES)]), [0, 0]),
        "then-random": (np.stack([WFA_FOLLOW, tr]), [1, 0]),
    }


def wfa_bound_finals(p, kind, variant, seed):
    """(fin_a or None, fin_b) int32[5][N] of a variant: kind "enc" / "pub" (bodies alone), variant "zero d0" / "random d0"."""
    fin = wfa_case(p, WFA_STATES, None if variant == "zero d0" else np.random.default_rng(seed))[1]
    return (fin[:, :p.N] if kind == "enc" else None), fin[:, p.N:]


def wfa_bound_bits(p):
    """the TGSW samples int32[2][2l][2][N] of the two bits those automata read"""
    rnd = np.random.default_rng(0xE0 + 16 * p.l + p.Bgbit).integers(-2**31, 2**31, size=(2 * p.l, 2, p.N), dtype=np.int64).astype(np.int32)
    return np.stack([lhe_cmux_case(p)[0], rnd])
