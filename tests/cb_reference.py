"""Reference of circuit bootstrapping (include/thfhe_hip.h: thfhe_cb_private_keyswitch, thfhe_circuit_bootstrap) -- TEST
INFRASTRUCTURE ONLY, in numpy: the digit rule, the private key switch (exact float64 GEMMs on 16-bit limbs of the key, as
thfhe.keygen.gen_keyswitch_key multiplies) and the composition with stage A, which is the CPU oracle's 3-gen bootstrap (MKOracle, the path of
mk_lut_reference.py).  Nothing here imports the product's kernels.

Layouts: key int32[2][D][t][2][N]; lwe2 int32[count][l][D+1]; rows int32[count][2l][2][N], T_0 of level j at row j, T_1 at row l + j."""
import numpy as np


def rounded(words, t, basebit):
    """The mask words rounded to t basebit bits, as wrapping uint32: (w + 2^(31 - t basebit)) with the low 32 - t basebit bits cleared."""
    bt = t * basebit
    w = np.asarray(words, np.int64) & 0xFFFFFFFF
    if bt >= 32:
        return w
    return ((w + (1 << (31 - bt))) & 0xFFFFFFFF) >> (32 - bt) << (32 - bt)


def digits(words, t, basebit):
    """THE digit rule: round the word to t basebit bits, split the kept bits into t digits of basebit bits (digit 0 the most significant), then
    from the least significant digit upward: u = raw digit + carry; u >= B/2 gives the digit u - B and carry 1, else the digit u and carry 0.
    The carry out of digit 0 is a whole turn and is dropped.  -> int64[..., t] with every digit in [-B/2, B/2) and
    sum_p d_p 2^(32 - (p+1) basebit) = the rounded word mod 2^32."""
    B, bt = 1 << basebit, t * basebit
    top = rounded(words, t, basebit) >> (32 - bt)
    out = np.empty(top.shape + (t,), np.int64)
    carry = np.zeros_like(top)
    for p in range(t - 1, -1, -1):
        u = ((top >> ((t - 1 - p) * basebit)) & (B - 1)) + carry
        carry = (u >= B // 2).astype(np.int64)
        out[..., p] = u - B * carry
    return out


def balanced_bytes(words):
    """The four balanced signed bytes of each 32-bit word, w = sum_p beta_p 2^(8p) mod 2^32, beta_p in [-128, 127] (the key planes of the
    matrix-core kernel) -> int64[..., 4]"""
    w = np.asarray(words, np.int64) & 0xFFFFFFFF
    out = np.empty(w.shape + (4,), np.int64)
    for p in range(4):
        b = ((w & 0xFF) ^ 0x80) - 0x80
        out[..., p] = b
        w = ((w - b) >> 8) & 0xFFFFFF
    return out


def private_keyswitch(key, lwe2, l, t, basebit, chunk=2048):
    """rows int32[count][2l][2][N]: T_1 = (0, b X^0) - sum d_ip K[1][i][p], T_0 = (b X^0, 0) - sum d_ip K[0][i][p].  |digit| <= 128 and limbs
    below 2^16 keep every partial sum below D t 2^23 < 2^53: the float64 products are exact."""
    key = np.asarray(key, np.int32)
    _, D, t_, _, N = key.shape
    assert t_ == t
    lwe2 = np.asarray(lwe2, np.int32).reshape(-1, l, D + 1)
    count = lwe2.shape[0]
    dig = digits(lwe2[:, :, :D], t, basebit).reshape(count * l, D * t).astype(np.float64)
    K = key.reshape(2, D * t, 2 * N)
    acc = np.zeros((2, count * l, 2 * N), np.int64)
    for f in range(2):
        for k0 in range(0, D * t, chunk):
            rows = K[f, k0:k0 + chunk].astype(np.int64)
            lo, hi = (rows & 0xFFFF).astype(np.float64), (rows >> 16).astype(np.float64)
            d = dig[:, k0:k0 + chunk]
            acc[f] += (d @ lo).astype(np.int64) + ((d @ hi).astype(np.int64) << 16)
    out = np.zeros((count, 2 * l, 2 * N), np.int64)
    b = lwe2[:, :, D].astype(np.int64)
    out[:, :l] = -acc[0].reshape(count, l, 2 * N)
    out[:, l:] = -acc[1].reshape(count, l, 2 * N)
    out[:, :l, 0] += b       # T_0: b on coefficient 0 of the mask
    out[:, l:, N] += b       # T_1: b on coefficient 0 of the body
    return out.astype(np.uint32).view(np.int32).reshape(count, 2 * l, 2, N)


def plane_sums(key, lwe2, l, t, basebit, cols):
    """max |C_plane| over the inputs, the words `cols` of the key rows and the four byte planes: the int32 partial sums of the matrix-core kernel,
    C_plane = A B_plane"""
    key = np.asarray(key, np.int32)
    _, D, _, _, N = key.shape
    lwe2 = np.asarray(lwe2, np.int32).reshape(-1, l, D + 1)
    dig = digits(lwe2[:, :, :D], t, basebit).reshape(-1, D * t).astype(np.float64)
    planes = balanced_bytes(key.reshape(2, D * t, 2 * N)[:, :, cols])
    return max(float(np.abs(dig @ planes[f, :, :, p].astype(np.float64)).max()) for f in range(2) for p in range(4))


def stage_a(orc2, recs, l, Bgbit):
    """lwe2 int32[len(recs)][l][D+1] from gate-encoded records: per gadget level the oracle's 3-gen bootstrap with mu_j = 2^(63 - (j+1) Bgbit) up to the
    extracted, converted record (MKOracle.bootstrap_wo_keyswitch), + 2^(31 - (j+1) Bgbit) on the body: an LWE sample of m 2^(32 - (j+1) Bgbit)."""
    from support import pmap
    recs = np.asarray(recs, np.int32)
    jobs = [(r, j) for r in range(recs.shape[0]) for j in range(l)]

    def one(job):
        r, j = job
        u = orc2.bootstrap_wo_keyswitch(recs[r], 1 << (63 - (j + 1) * Bgbit)).astype(np.int64)
        u[-1] += 1 << (31 - (j + 1) * Bgbit)
        return u.astype(np.uint32).view(np.int32)
    return np.stack(pmap(one, jobs)).reshape(recs.shape[0], l, -1)


def circuit_bootstrap(orc2, key, recs, l, Bgbit, t, basebit):
    """rows int32[len(recs)][2l][2][N] of the bits behind the gate-encoded records `recs` (level-1 decomposition (l, Bgbit))"""
    return private_keyswitch(key, stage_a(orc2, recs, l, Bgbit), l, t, basebit)


def centred(x):
    """int words as signed residues mod 2^32 (int64)"""
    return (np.asarray(x, np.int64) + 2**31) % 2**32 - 2**31


def row_errors(K, rows, bits, l, Bgbit):
    """phase - message of every coefficient of every row, int64[len(bits)][2l][N]: row l + j carries bit g_j on coefficient 0, row j carries
    -z bit g_j, g_j = 2^(32 - (j+1) Bgbit); K: thfhe.keygen.SecretKeySet"""
    rows = np.asarray(rows, np.int32)
    ph = K.tlwe_phase(rows[:, :, 0], rows[:, :, 1]).astype(np.int64)
    bits = np.asarray(bits, np.int64).reshape(-1)
    z = K.rlwe_key.astype(np.int64)
    for j in range(l):
        g = bits << (32 - (j + 1) * Bgbit)
        ph[:, l + j, 0] -= g
        ph[:, j] += g[:, None] * z[None, :]
    return centred(ph)


def sigma_row(D, t, basebit, sigma_pks, z2_norm2, sigma_a):
    """sigma_row^2 = D t (B^2 / 12) sigma_pks^2 + (|z2|^2 / 3) 2^(-2 (t basebit + 1)) + sigma_A^2 (torus units)"""
    B = float(1 << basebit)
    return float(np.sqrt(D * t * B * B / 12 * sigma_pks ** 2 + z2_norm2 / 3 * 2.0 ** (-2 * (t * basebit + 1)) + sigma_a ** 2))


def sigma_a(n, l2, Bgbit2, N2, z2_norm2, sigma_bk2):
    """Stage A's rotation noise and the Torus64 -> Torus32 conversion: n CMuxes, each with the decomposition's rounding (uniform below 2^-(l2 Bgbit2 + 1)
    on the 1 + |z2|^2 terms of a phase) and 2 l2 N2 digits of variance Bg^2 / 12 on the key noise; then |z2| 2^-33 / sqrt(3)."""
    eps = 2.0 ** -(l2 * Bgbit2 + 1)
    rot = n * ((1 + z2_norm2) * eps * eps / 3 + 2 * l2 * N2 * 4.0 ** Bgbit2 / 12 * sigma_bk2 ** 2)
    return float(np.sqrt(rot + z2_norm2 * 2.0 ** -66 / 3))
