"""Independent numpy model of the LWE -> TLWE packing key switch: int64 arithmetic wrapped to uint32,
written from the operation's definition -- nothing here imports the product's packing code.

  digits     abar = a + 2^(32 - (1 + basebit t)),  d_jp = (abar_j >> (32 - (p+1) basebit)) & (2^basebit - 1)     (J/keyswitch.jl:45-80)
  per sample T_i = (0, b_i X^0) - sum_{j, p: d_ijp != 0} PK[j][p][d_ijp - 1]                                     (2N words: alpha, beta)
  output     P_g = sum_{i < m} X^i T_{g m + i} mod X^N + 1, both polynomials
"""
import numpy as np

M32 = (1 << 32) - 1


def wrap32(x):
    return (np.asarray(x, np.int64) & M32).astype(np.uint32).view(np.int32)


def prec_offset(t, basebit):
    bt = t * basebit
    return 0 if bt >= 32 else 1 << (31 - bt)


def digits(a, t, basebit):
    """a int[..., n] -> digits int64[..., n, t]."""
    abar = (np.asarray(a, np.int64) + prec_offset(t, basebit)) & M32
    sh = 32 - (np.arange(t, dtype=np.int64) + 1) * basebit
    return (abar[..., None] >> sh) & ((1 << basebit) - 1)


def rounded(a, t, basebit):
    """the value the digits represent: sum_p d_p 2^(32 - (p+1) basebit), mod 2^32."""
    d = digits(a, t, basebit)
    sh = 32 - (np.arange(t, dtype=np.int64) + 1) * basebit
    return (d << sh).sum(axis=-1) & M32


def per_sample(lwe, pk, t, basebit, chunk=256):
    """T int32[count][2N] for LWE records int32[count][n+1] and the key int32[n][t][R][2][N]: a one-hot GEMM on 16-bit limbs in float64
    (at most n t ones per row, so every partial sum stays below 2^53)."""
    lwe = np.asarray(lwe, np.int64)
    n, R, N2 = pk.shape[0], (1 << basebit) - 1, 2 * pk.shape[-1]
    K = np.asarray(pk, np.int64).reshape(n * t * R, N2) & M32
    lo, hi = (K & 0xFFFF).astype(np.float64), (K >> 16).astype(np.float64)
    out = np.empty((lwe.shape[0], N2), np.int32)
    for c0 in range(0, lwe.shape[0], chunk):
        x = lwe[c0:c0 + chunk]
        d = digits(x[:, :n], t, basebit).reshape(x.shape[0], n * t)
        onehot = np.zeros((x.shape[0], n * t * R), np.float64)
        rows, cols = np.nonzero(d)
        onehot[rows, cols * R + d[rows, cols] - 1] = 1.0
        s = (onehot @ lo).astype(np.int64) + ((onehot @ hi).astype(np.int64) << 16)
        s = -s
        s[:, N2 // 2] += x[:, n]
        out[c0:c0 + chunk] = wrap32(s)
    return out


def rotate_sum(T, slots, N):
    """P_g = sum_i X^i T_{g slots + i} mod X^N + 1 -> (a, b) int32[ceil(count / slots)][N]."""
    T = np.asarray(T, np.int64)
    count = T.shape[0]
    G = -(-count // slots)
    acc = np.zeros((G, 2, N), np.int64)
    for i in range(min(slots, count)):
        rows = T[i::slots].reshape(-1, 2, N)           # samples g slots + i, g = 0 .. (their count) - 1
        rolled = np.roll(rows, i, axis=-1)             # coefficient c <- f[c - i]
        rolled[..., :i] *= -1                          # c < i: -f[c - i + N]
        acc[:rows.shape[0]] += rolled
    return wrap32(acc[:, 0]), wrap32(acc[:, 1])


def pack(lwe, pk, t, basebit, slots):
    return rotate_sum(per_sample(lwe, pk, t, basebit), slots, pk.shape[-1])


def negacyclic_mul(a, z):
    """rows of a (torus polynomials) times the small integer polynomial z, exact mod 2^32: schoolbook over the shifts of z's nonzero
    coefficients (z is a key or a key share: few distinct small values)."""
    a = np.asarray(a, np.int64).reshape(-1, np.shape(z)[0])
    z = np.asarray(z, np.int64)
    N = z.shape[0]
    out = np.zeros(a.shape, np.int64)
    for k in np.nonzero(z)[0]:
        r = np.roll(a, k, axis=-1)                     # X^k a
        r[:, :k] *= -1
        out = (out + z[k] * r) & M32
    return wrap32(out)


def tlwe_phase(a, b, z):
    """b - a (*) z, int32[..., N]."""
    return wrap32(np.asarray(b, np.int64) - negacyclic_mul(a, z).astype(np.int64)).reshape(np.shape(b))


def lwe_phase(lwe, s):
    lwe = np.asarray(lwe, np.int64)
    return wrap32(lwe[:, -1] - (lwe[:, :-1] * np.asarray(s, np.int64)).sum(axis=1))


def torus(x):
    """int32 torus words -> reals in [-1/2, 1/2)."""
    return np.asarray(x, np.int32).astype(np.float64) / 2.0**32


def predicted_sigma(m, n, t, basebit, key_weight, sigma_pk):
    """Standard deviation of phase(P)[i] - phase(LWE_i) for uniform masks: the rounding of sample i (key_weight coordinates, each
    uniform in [-2^-(bt+1), 2^-(bt+1))) plus the key noise of the m n t (1 - 2^-basebit) nonzero digits of the m samples."""
    bt = t * basebit
    h = 2.0**-(bt + 1) if bt < 32 else 0.0
    return np.sqrt(key_weight * h * h / 3 + m * n * t * (1 - 2.0**-basebit) * sigma_pk**2)
