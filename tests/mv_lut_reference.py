"""Reference of multi-value bootstrapping with factored test vectors (include/thfhe_hip.h: thfhe_mv_lut_bootstrap,
thfhe_tree_lut_bootstrap_mv) -- TEST INFRASTRUCTURE ONLY, composed from the CPU oracle's pieces (lut_reference.py,
tree_lut_reference.py): prologue -> mod-switch -> X^{-barb} tv0 -> the oracle's CMux chain -> for every output the integer combination of p
ordinary extractions -> the oracle's key switch.  Nothing here imports the product's code."""
import numpy as np

import lut_reference as R
import oracle_lib as O
import tree_lut_reference as TR


def _u64(v):
    """two's-complement words as uint64: sums and products then wrap mod 2^64, and 2^32 divides 2^64, so the low 32 bits are exact"""
    return np.asarray(v, np.int64).view(np.uint64)


def _low32(v):
    return (v & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32)


def negacyclic_mul(a, b, N):
    """a * b mod (X^N + 1, 2^32), exact, term by term of b."""
    a = _u64(a)
    out = np.zeros(N, np.uint64)
    for k in np.flatnonzero(np.asarray(b)):
        r = np.roll(a, k)                     # coefficient i <- a[i - k]
        r[:k] = np.uint64(0) - r[:k]          # below k: -a[i - k + N]
        out += r * _u64(b)[k]
    return _low32(out)


def factor_poly(c, N):
    """F(X) = sum_k c[k] X^(box/2 + k box), box = N / p, as N integers."""
    p = len(c)
    box = N // p
    F = np.zeros(N, np.int64)
    F[box // 2 + box * np.arange(p)] = np.asarray(c, np.int64)
    return F


def combine(acc, factors, N):
    """Every output of one accumulator (mask, body) int32[2N]: out[j] = - sum_k factors[j][k] * extract_at(acc, N - box/2 - k box), word-wise mod
    2^32 -> int32[q][N+1]."""
    factors = np.asarray(factors)
    q, p = factors.shape
    box = N // p
    taps = np.stack([R.extract_at(acc, N - box // 2 - k * box, N) for k in range(p)])
    return _low32(np.uint64(0) - _u64(factors) @ _u64(taps))


def rotate(orc, x, tv0):
    """The accumulator of one prologue output x (int32[n+1]) at theta = 1: (0, X^{-barb} tv0) through the oracle's CMux chain, int32[2N]."""
    p = orc.params
    n, N = p.n, p.N
    bar = [O.lib().oracle_modswitch(int(w), N) for w in x]
    acc = np.zeros(2 * N, np.int32)
    acc[N:] = R.monomial(tv0, -bar[n], N)
    for i in range(n):
        if bar[i] != 0:
            acc = orc.mux_rotate(i, bar[i], acc)
    return acc


def mv_lut(orc, recs, weights, bias, tv0, factors, keyswitch=True):
    """Reference of thfhe_mv_lut_bootstrap(_wo_keyswitch) for one sample: recs = its input records, factors int[q][p] = its table."""
    u = combine(rotate(orc, R.prologue(recs, weights, bias), tv0), factors, orc.params.N)
    return np.stack([orc.keyswitch(r) for r in u]) if keyswitch else u


def tree_mv(orc, pk, t, basebit, lo_recs, w_lo, bias_lo, hi_recs, w_hi, bias_hi, tv0, factors):
    """Reference of thfhe_tree_lut_bootstrap_mv for one sample: factors int[p_hi][p_lo] = its table.  Returns (out int32[n+1], candidates
    int32[p_hi][n+1])."""
    cands = mv_lut(orc, lo_recs, w_lo, bias_lo, tv0, factors)
    a, b = TR.pack_boxes(cands, pk, t, basebit, cands.shape[0])
    return TR.lut_enc(orc, hi_recs, w_hi, bias_hi, a[0], b[0], 1)[0], cands
