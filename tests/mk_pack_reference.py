"""Reference of the multi-key packing key switch, encrypted tables and the two-digit tree of the 3-gen engine (include/thfhe_hip.h,
thfhe_mk_pack_boxes / thfhe_mk_lut_bootstrap_enc / thfhe_mk_tree_lut_bootstrap) -- TEST INFRASTRUCTURE ONLY.  An independent
numpy model on wrapping 64-bit words: the per-record sum over the key rows its digits name, the box packing by explicit negacyclic monomial
products (not the kernel's prefix sums), the accumulator start on both polynomials, and the tree composed with tests/mk_lut_reference.py."""
import numpy as np

import mk_lut_reference as R


def round_words(a, t, basebit):
    """Mask words with the LWE key switch's rounding offset, mod 2^32, as Python-exact uint64 values below 2^32."""
    bt = t * basebit
    off = 0 if bt >= 32 else 1 << (31 - bt)
    return (np.asarray(a, np.int64) + off) & 0xFFFFFFFF


def digits(a, t, basebit):
    """d[..., p] = digit p (0 = most significant) of the rounded words: 0 .. 2^basebit - 1."""
    abar = round_words(a, t, basebit)
    sh = 32 - (np.arange(t) + 1) * basebit
    return (abar[..., None] >> sh) & ((1 << basebit) - 1)


def pack_rows(recs, pk, t, basebit):
    """T_i = (0, b_i 2^32 on X^0) - sum over the non-zero digits d_jp of pk[j][p][d - 1], mod 2^64: int64[count][2][N].
    recs int32[count][D + 1], pk int64[D][t][R][2][N]."""
    recs = np.asarray(recs, np.int32)
    pk = np.asarray(pk, np.int64).view(np.uint64)
    D, N = pk.shape[0], pk.shape[-1]
    assert recs.shape[1] == D + 1 and pk.shape[1] == t and pk.shape[2] == (1 << basebit) - 1
    out = np.zeros((recs.shape[0], 2, N), np.uint64)
    for i, r in enumerate(recs):
        d = digits(r[:D], t, basebit)
        j, p = np.nonzero(d)
        out[i] = np.uint64(0) - pk[j, p, d[j, p] - 1].sum(axis=0, dtype=np.uint64)
        out[i, 1, :1] += np.array([(int(r[D]) << 32) % (1 << 64)], np.uint64)   # array addition wraps silently
    return out.view(np.int64)


def monomial_mul(poly, k):
    """X^k * poly mod X^N + 1 on wrapping 64-bit words, any integer k: coefficient by coefficient."""
    poly = np.asarray(poly, np.int64).view(np.uint64)
    N = poly.shape[-1]
    k %= 2 * N
    src = np.arange(N) - k            # coefficient c comes from c - k, read in the negacyclic extension
    sign = (src // N) % 2             # an odd number of periods away: negated
    v = poly[..., src % N]
    return np.where(sign == 1, np.uint64(0) - v, v).view(np.int64)


def pack_boxes(T, p):
    """out[g] = U(X) * sum_{i < p} X^(i B) T[g p + i], B = N / p, U = X^(-B/2) (1 + X + ... + X^(B-1)), on both polynomials: the B monomial
    products of U one by one.  T int64[count][2][N] -> (tv_a, tv_b) int64[count / p][N]."""
    T = np.asarray(T, np.int64)
    count, _, N = T.shape
    assert count % p == 0 and N % p == 0
    B = N // p
    out = np.zeros((count // p, 2, N), np.uint64)
    for g in range(count // p):
        S = np.zeros((2, N), np.uint64)
        for i in range(p):
            S += monomial_mul(T[g * p + i], i * B).view(np.uint64)
        for u in range(B):
            out[g] += monomial_mul(S.view(np.int64), u - B // 2).view(np.uint64)
    out = out.view(np.int64)
    return out[:, 0].copy(), out[:, 1].copy()


def pack(recs, pk, t, basebit, p):
    """thfhe_mk_pack_boxes."""
    return pack_boxes(pack_rows(recs, pk, t, basebit), p)


def acc_start_enc(tv_a, tv_b, barb):
    """The accumulator of a rotation on an encrypted table: (X^{-barb} tv_a, X^{-barb} tv_b) as int64[2 N]."""
    return np.concatenate([monomial_mul(tv_a, -barb), monomial_mul(tv_b, -barb)])


def lut_enc_wo_keyswitch(orc, x, tv_a, tv_b, theta):
    """mk_lut_reference.lut_wo_keyswitch with the accumulator started on both polynomials: int32[theta][N + 1]."""
    p = orc.params
    n, N, P = p.n, p.N, p.parties
    bar = R.bars(x, N, theta)
    acc = acc_start_enc(tv_a, tv_b, bar[P * n])
    for q in range(P):
        for i in range(n):
            if bar[q * n + i] != 0:
                acc = orc.mux_rotate(q, i, bar[q * n + i], acc)
    return np.stack([R.extract_at(acc, j, N) for j in range(theta)])


def lut_bootstrap_enc(orc, recs, weights, bias, tv_a, tv_b, theta, keyswitch=True):
    """Reference of thfhe_mk_lut_bootstrap_enc(_wo_keyswitch) for one sample."""
    u = lut_enc_wo_keyswitch(orc, R.prologue(recs, weights, bias), tv_a, tv_b, theta)
    return np.stack([orc.keyswitch(r) for r in u]) if keyswitch else u


def tree(orc, pk, t, basebit, tv1, lo, hi, p_hi, weights_lo=(1,), bias_lo=0, theta=1, weights_hi=(1,), bias_hi=0, parts=False):
    """Reference of thfhe_mk_tree_lut_bootstrap for one sample: tv1 int64[p_hi / theta][N] the rows of its table, lo / hi the lists of its operand
    records, pk the D = N packing key.  parts: also return the candidates and the packed table."""
    cand = np.concatenate([R.lut_bootstrap(orc, lo, weights_lo, bias_lo, row, theta, keyswitch=False) for row in tv1])
    assert cand.shape[0] == p_hi
    ta, tb = pack(cand, pk, t, basebit, p_hi)
    out = lut_bootstrap_enc(orc, hi, weights_hi, bias_hi, ta[0], tb[0], 1)[0]
    return (out, cand, ta[0], tb[0]) if parts else out
