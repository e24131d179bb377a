"""The LWE key switch written from its definition, in NumPy: independent of the GPU code (csrc/thfhe_keyswitch.h) and of the C oracle.

For every party p and coordinate i of the extracted sample (mask a, last word b), all arithmetic mod 2^32:

  abar = a + 2^(31 - t basebit)                              (0 when t basebit >= 32: the digits cover the whole word)
  d_j  = (abar >> (32 - (j + 1) basebit)) & (2^basebit - 1)  j = 0 .. t - 1
  out[p n + c] -= KS[p][i][j][d_j - 1][c]                    for d_j != 0, c < n; column n of every party's rows goes to the last word
  out[last]    += b

The layouts are those of KsArgs: one mask shared by all parties (u_pstride = 0: single key, 3-gen) or one mask per party (u_pstride = N:
KMS, CCS; records of P N + 1 words); rot_per_gate = 2 sums two records and adds 2^29 to b (the MUX combine); the packing layout has key rows
of 2 N_ring words and b at column N_ring (pack_reference).  One gather per sample: the key indexed by (i, j, d - 1) where d != 0, summed with
dtype=uint32 (NumPy's wrap-around sum)."""
import numpy as np


def prec_offset(t, basebit):
    bt = t * basebit
    return 0 if bt >= 32 else 1 << (31 - bt)


def digits(a, t, basebit):
    """mask words uint32[N] -> digits int64[N][t]"""
    abar = (np.asarray(a).astype(np.int64) + prec_offset(t, basebit)) & 0xFFFFFFFF
    sh = 32 - (np.arange(t, dtype=np.int64) + 1) * basebit
    return (abar[:, None] >> sh) & ((1 << basebit) - 1)


def _gather(K, a, t, basebit):
    """sum of the rows KS[i][j][d - 1] the digits of the mask `a` name: K uint32[N][t][R][row], a uint32[N] -> uint32[row]"""
    d = digits(a, t, basebit)
    i, j = np.nonzero(d)
    return K[i, j, d[i, j] - 1].sum(axis=0, dtype=np.uint32)


def combine(u, rot_per_gate):
    """records int32[count * rot_per_gate][rec] -> the key switch's input uint32[count][rec]: the record itself, or u1 + u2 + (0, 2^29)"""
    u = np.ascontiguousarray(u, np.int32).view(np.uint32)
    u = u.reshape(-1, rot_per_gate, u.shape[-1])
    if rot_per_gate == 1:
        return u[:, 0]
    assert rot_per_gate == 2
    s = u[:, 0] + u[:, 1]
    s[:, -1] += np.uint32(1 << 29)
    return s


def keyswitch(u, ksk, t, basebit, u_pstride=0, rot_per_gate=1, rows=None):
    """u int32[count * rot_per_gate][rec], ksk int32[P][N][t][2^basebit - 1][n + 1] -> int32[len(rows)][P n + 1], the key switch of the
    samples `rows` (default: all).  rec = N + 1 with a shared mask (u_pstride = 0), P N + 1 with one mask per party (u_pstride = N)."""
    K = np.asarray(ksk, np.int32).view(np.uint32)
    P, N, n = K.shape[0], K.shape[1], K.shape[-1] - 1
    assert K.shape[2:4] == (t, (1 << basebit) - 1) and u_pstride in (0, N)
    x = combine(u, rot_per_gate)
    assert x.shape[1] == (P * N + 1 if u_pstride else N + 1)
    rows = range(x.shape[0]) if rows is None else rows
    out = np.zeros((len(rows), P * n + 1), np.uint32)
    for k, g in enumerate(rows):
        out[k, -1] = x[g, -1]
        for p in range(P):
            s = _gather(K[p], x[g, p * u_pstride:p * u_pstride + N], t, basebit)
            out[k, p * n:(p + 1) * n] -= s[:n]
            out[k, -1:] -= s[n:]   # (slices, not scalars: array arithmetic wraps silently)
    return out.view(np.int32)


def pack_keyswitch(lwe, pk, t, basebit, rows=None):
    """the packing layout: lwe int32[count][n_lwe + 1], pk int32[n_lwe][t][2^basebit - 1][2][N_ring] -> int32[len(rows)][2 N_ring],
    T = (0, b X^0) - sum of the named key rows: b lands at column N_ring, inside the row."""
    K = np.asarray(pk, np.int32).view(np.uint32)
    n_lwe, N_ring = K.shape[0], K.shape[-1]
    K = K.reshape(n_lwe, t, (1 << basebit) - 1, 2 * N_ring)
    x = combine(lwe, 1)
    assert x.shape[1] == n_lwe + 1
    rows = range(x.shape[0]) if rows is None else rows
    out = np.zeros((len(rows), 2 * N_ring), np.uint32)
    for k, g in enumerate(rows):
        out[k] -= _gather(K, x[g, :n_lwe], t, basebit)
        out[k, N_ring:N_ring + 1] += x[g, -1:]
    return out.view(np.int32)
