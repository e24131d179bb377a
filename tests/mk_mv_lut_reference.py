"""Reference of multi-value bootstrapping on the 3-gen multi-key engine (include/thfhe_hip.h: thfhe_mk_mv_lut_bootstrap) --
TEST INFRASTRUCTURE ONLY, composed from the CPU oracle's pieces (mk_lut_reference.py): prologue -> mod-switch at theta = 1 -> X^{-barb} tv0 over
Torus64 -> the oracle's 3-gen CMux chain, party-major with the zero skip -> for every output the integer combination of p UNCONVERTED extractions
mod 2^64, out_bias on the body word, ONE t64tot32 per word -> the oracle's multi-key key switch.  Nothing here imports the product's code."""
import numpy as np

import mk_lut_reference as R
import oracle_lib as O
from conv_edges import t64tot32   # the vectorised conversion lives with its edge words; MV.t64tot32 stays this module's name for it


def _u64(v):
    return np.ascontiguousarray(v, np.int64).view(np.uint64)


def extract_raw(acc, J, N):
    """E(ACC, J): the unconverted extraction at coefficient J of acc = (mask, body) int64[2N], as uint64[N+1]: e_i = a_{J-i} for i <= J,
    -a_{N+J-i} for i > J (mod 2^64), e_N = body_J."""
    a = _u64(acc[:N])
    i = np.arange(N)
    v = a[(J - i) % N]
    v = np.where(i <= J, v, np.uint64(0) - v)
    return np.concatenate([v, _u64(acc[N + J:N + J + 1])])


def tap_positions(p, N):
    """J_k = N - box/2 - k box, k < p."""
    box = N // p
    return [N - box // 2 - k * box for k in range(p)]


def combine64(acc, taps, p, N, out_bias=0, convert=t64tot32):
    """Every output of one accumulator int64[2N]: record j = t64tot32, word by word, of - sum_k taps[j][k] * E(acc, J_k) (+ out_bias on the body
    word), all mod 2^64, taps sign-extended -> int32[q][N+1].  convert: what is applied to the int64 sums instead of t64tot32 (the edge tests pass
    the identity and a wrong conversion)."""
    taps = np.asarray(taps, np.int64).reshape(-1, p)
    E = np.stack([extract_raw(acc, J, N) for J in tap_positions(p, N)])
    s = np.zeros((taps.shape[0], N + 1), np.uint64)
    for k in range(p):   # uint64 products and sums wrap mod 2^64
        s -= _u64(taps[:, k])[:, None] * E[k][None, :]
    s[:, N] += _u64(R.to_i64([out_bias]))[0]
    return convert(s.view(np.int64))


def convert_then_combine(acc, taps, p, N, out_bias=0):
    """The WRONG order, for the test that tells the two apart: t64tot32 of every extraction first, the combination mod 2^32 after it."""
    taps = np.asarray(taps, np.int64).reshape(-1, p)
    E = np.stack([t64tot32(extract_raw(acc, J, N).view(np.int64)) for J in tap_positions(p, N)]).astype(np.int64)
    s = -(taps @ E)
    s[:, N] += int(t64tot32(R.to_i64([out_bias]))[0])
    return (s & 0xFFFFFFFF).astype(np.uint32).view(np.int32)


def rotate(orc, x, tv0):
    """The accumulator of one prologue output x (int32[P n + 1]) at theta = 1: (0, X^{-barb} tv0) through the oracle's party-major CMux chain,
    int64[2N]."""
    p = orc.params
    n, N, P = p.n, p.N, p.parties
    bar = R.bars(x, N, 1)
    acc = np.zeros(2 * N, np.int64)
    acc[N:] = R.monomial64(tv0, -bar[P * n], N)
    for q in range(P):
        for i in range(n):
            if bar[q * n + i] != 0:
                acc = orc.mux_rotate(q, i, bar[q * n + i], acc)
    return acc


def mv_lut(orc, recs, weights, bias, tv0, factors, out_bias=0, keyswitch=True):
    """Reference of thfhe_mk_mv_lut_bootstrap(_wo_keyswitch) for one sample: recs = its input records, factors int[q][p] = its table."""
    factors = np.asarray(factors)
    u = combine64(rotate(orc, R.prologue(recs, weights, bias), tv0), factors, factors.shape[-1], orc.params.N, out_bias)
    return np.stack([orc.keyswitch(r) for r in u]) if keyswitch else u
