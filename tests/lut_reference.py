"""Reference of programmable bootstrapping (include/thfhe_hip.h, thfhe_lut_bootstrap) composed from the CPU oracle's pieces -- TEST
INFRASTRUCTURE ONLY: prologue -> mod-switch to multiples of theta -> X^{-barb} tv -> the oracle's CMux chain -> extraction at coefficients
0 .. theta-1 -> the oracle's key switch.  tests/test_lut_host.py checks it against Oracle.bootstrap_wo_keyswitch / keyswitch with a
constant test vector."""
import numpy as np

import oracle_lib as O


def to_i32(v):
    return (np.asarray(v, np.int64) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)


def monomial(poly, shift, N):
    """X^shift * poly mod X^N + 1 (oracle_mul_by_monomial32)."""
    poly = np.ascontiguousarray(poly, np.int32)
    out = np.zeros(N, np.int32)
    O.lib().oracle_mul_by_monomial32(O.p32(poly), int(shift), N, O.p32(out))
    return out


def encrypt_words(K, words, sigma, seed):
    """Fresh LWE records of arbitrary Torus32 messages under K's LWE key."""
    p = K.params
    out = np.zeros((len(words), p.n + 1), np.int32)
    for i, w in enumerate(words):
        O.lib().oracle_lwe_encrypt(O.p32(K.lwe_key), p.n, int(w), sigma, seed, i, O.p32(out[i]))
    return out


def prologue(recs, weights, bias):
    """x = sum_q weights[q] * recs[q] + (0, ..., 0, bias), word-wise mod 2^32 (one record per input)."""
    x = np.zeros(recs[0].shape[-1], np.int64)
    for r, w in zip(recs, weights):
        x += int(w) * np.asarray(r, np.int64)
    x[-1] += int(bias)
    return to_i32(x)


def extract_at(acc, j, N):
    """LWE(N) record of coefficient j of acc = (mask, body): a'_i = a_{j-i} (i <= j), -a_{N+j-i} (i > j), b = body_j."""
    a = np.asarray(acc[:N], np.int64)
    i = np.arange(N)
    v = a[(j - i) % N]
    out = np.empty(N + 1, np.int64)
    out[:N] = np.where(i <= j, v, -v)
    out[N] = acc[N + j]
    return to_i32(out)


def lut_wo_keyswitch(orc, x, tv, theta):
    """One prologue output x (int32[n+1]) through the rotation: int32[theta][N+1]."""
    p = orc.params
    n, N = p.n, p.N
    bar = [O.lib().oracle_modswitch(int(w), N // theta) * theta for w in x]
    acc = np.zeros(2 * N, np.int32)
    acc[N:] = monomial(tv, -bar[n], N)
    for i in range(n):
        if bar[i] != 0:
            acc = orc.mux_rotate(i, bar[i], acc)
    return np.stack([extract_at(acc, j, N) for j in range(theta)])


def lut_bootstrap(orc, recs, weights, bias, tv, theta, keyswitch=True):
    """Reference of thfhe_lut_bootstrap(_wo_keyswitch) for one sample: recs = its input records, tv = its test vector."""
    u = lut_wo_keyswitch(orc, prologue(recs, weights, bias), tv, theta)
    return np.stack([orc.keyswitch(r) for r in u]) if keyswitch else u
