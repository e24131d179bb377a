"""Reference of multi-key programmable bootstrapping (include/thfhe_hip.h, thfhe_mk_lut_bootstrap) composed from the CPU oracle's pieces --
TEST INFRASTRUCTURE ONLY: prologue -> mod-switch to multiples of theta -> X^{-barb} tv over Torus64 -> the oracle's 3-gen CMux chain, party-major
with the zero skip -> extraction at coefficients 0 .. theta-1 with t64tot32 -> the oracle's multi-key key switch.  tests/test_mk_lut_host.py
checks it against MKOracle.bootstrap_wo_keyswitch / keyswitch with a constant test vector."""
import numpy as np

import lut_reference as R
import oracle_lib as O

prologue = R.prologue   # x = sum_q weights[q] * recs[q] + (0, ..., 0, bias), word-wise mod 2^32: the same on P n + 1 words


def to_i64(v):
    """Python integers taken mod 2^64 as int64 words."""
    return np.array([((int(x) + (1 << 63)) % (1 << 64)) - (1 << 63) for x in np.ravel(v)], np.int64).reshape(np.shape(v))


def monomial64(poly, shift, N):
    """X^shift * poly mod X^N + 1 over Torus64 (oracle_mul_by_monomial64)."""
    poly = np.ascontiguousarray(poly, np.int64)
    out = np.zeros(N, np.int64)
    O.lib().oracle_mul_by_monomial64(O.p64(poly), int(shift), N, O.p64(out))
    return out


def encrypt_words(K, words, sigma, seed):
    """Fresh records of arbitrary Torus32 messages under the concatenated P n key of MKKeys K (as MKKeys.encrypt_bits)."""
    p = K.params
    n = p.n * p.parties
    out = np.zeros((len(words), n + 1), np.int32)
    for i, w in enumerate(words):
        O.lib().oracle_lwe_encrypt(O.p32(K.lwe_keys), n, int(w), sigma, seed, i, O.p32(out[i]))
    return out


def bars(x, N, theta):
    """The theta-rounded mod-switch of every word: oracle_modswitch(word, N / theta) * theta."""
    return [O.lib().oracle_modswitch(int(w), N // theta) * theta for w in x]


def extract_at(acc, j, N):
    """LWE(N) record of coefficient j of acc = (mask, body) over Torus64: t64tot32(a_{j-i}) for i <= j, t64tot32(-a_{N+j-i}) for i > j (the
    negation mod 2^64 first), t64tot32(body_j)."""
    a = np.asarray(acc[:N], np.int64)
    i = np.arange(N)
    v = a[(j - i) % N]
    v = np.where(i <= j, v, -v)   # int64 negation wraps: -(-2^63) = -2^63, the negation mod 2^64
    t = O.lib().oracle_t64tot32
    return np.array([t(int(w)) for w in v] + [t(int(acc[N + j]))], np.int32)


def lut_wo_keyswitch(orc, x, tv, theta):
    """One prologue output x (int32[P n + 1]) through the rotation: int32[theta][N+1]."""
    p = orc.params
    n, N, P = p.n, p.N, p.parties
    bar = bars(x, N, theta)
    acc = np.zeros(2 * N, np.int64)
    acc[N:] = monomial64(tv, -bar[P * n], N)
    for q in range(P):          # party-major, key index inner (mk_blind_rotate_3gen)
        for i in range(n):
            if bar[q * n + i] != 0:
                acc = orc.mux_rotate(q, i, bar[q * n + i], acc)
    return np.stack([extract_at(acc, j, N) for j in range(theta)])


def lut_bootstrap(orc, recs, weights, bias, tv, theta, keyswitch=True):
    """Reference of thfhe_mk_lut_bootstrap(_wo_keyswitch) for one sample: recs = its input records, tv = its Torus64 test vector."""
    u = lut_wo_keyswitch(orc, prologue(recs, weights, bias), tv, theta)
    return np.stack([orc.keyswitch(r) for r in u]) if keyswitch else u
