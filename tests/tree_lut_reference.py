"""Reference of encrypted lookup tables and the two-digit tree PBS (include/thfhe_hip.h: thfhe_lut_bootstrap_enc, thfhe_pack_boxes,
thfhe_tree_lut_bootstrap) -- TEST INFRASTRUCTURE ONLY, composed from the CPU oracle's pieces (lut_reference.py) and
the numpy model of the packing key switch (pack_reference.py); nothing here imports the product's code."""
import numpy as np

import lut_reference as R
import oracle_lib as O
import pack_reference as PR


def lut_enc_wo_keyswitch(orc, x, tv_a, tv_b, theta):
    """lut_reference.lut_wo_keyswitch with the mask initialised too: accumulator (X^{-barb} tv_a, X^{-barb} tv_b) -> int32[theta][N+1]."""
    p = orc.params
    n, N = p.n, p.N
    bar = [O.lib().oracle_modswitch(int(w), N // theta) * theta for w in x]
    acc = np.zeros(2 * N, np.int32)
    acc[:N] = R.monomial(tv_a, -bar[n], N)
    acc[N:] = R.monomial(tv_b, -bar[n], N)
    for i in range(n):
        if bar[i] != 0:
            acc = orc.mux_rotate(i, bar[i], acc)
    return np.stack([R.extract_at(acc, j, N) for j in range(theta)])


def lut_enc(orc, recs, weights, bias, tv_a, tv_b, theta, keyswitch=True):
    """Reference of thfhe_lut_bootstrap_enc(_wo_keyswitch) for one sample: recs = its input records, (tv_a, tv_b) = its encrypted table."""
    u = lut_enc_wo_keyswitch(orc, R.prologue(recs, weights, bias), tv_a, tv_b, theta)
    return np.stack([orc.keyswitch(r) for r in u]) if keyswitch else u


def window(p, N):
    """U(X) = X^(-N/(2p)) (1 + X + ... + X^(N/p - 1)) mod X^N + 1 as N small integers: +1 on X^0 .. X^(B/2 - 1), -1 on X^(N - B/2) .. X^(N - 1)."""
    B = N // p
    u = np.zeros(N, np.int64)
    u[:B // 2] = 1
    u[N - B // 2:] = -1
    return u


def strided_rotate_sum(T, p, N):
    """S_g = sum_{i < p} X^(i N/p) T_{g p + i} mod X^N + 1 on the 2N-word records T -> int32[count / p][2][N]."""
    T = np.asarray(T, np.int64).reshape(-1, p, 2, N)
    B = N // p
    acc = np.zeros((T.shape[0], 2, N), np.int64)
    for i in range(p):
        r = np.roll(T[:, i], i * B, axis=-1)   # coefficient c <- f[c - i B]
        r[..., :i * B] *= -1                   # below i B: -f[c - i B + N]
        acc += r
    return PR.wrap32(acc)


def pack_boxes(lwe, pk, t, basebit, p, T=None):
    """Model of thfhe_pack_boxes: (a, b) int32[count / p][N] = U(X) * strided_rotate_sum(per-sample T_i), an explicit negacyclic product."""
    N = pk.shape[-1]
    T = PR.per_sample(lwe, pk, t, basebit) if T is None else T
    assert T.shape[0] % p == 0
    S = strided_rotate_sum(T, p, N)
    u = window(p, N)
    return PR.negacyclic_mul(S[:, 0], u), PR.negacyclic_mul(S[:, 1], u)


def tree(orc, pk, t, basebit, lo_recs, w_lo, bias_lo, theta1, hi_recs, w_hi, bias_hi, tv1, p_hi):
    """Reference of thfhe_tree_lut_bootstrap for one sample: tv1 = its table's rows int32[p_hi / theta1][N].  Returns (out int32[n+1],
    candidates int32[p_hi][n+1], packed (a, b))."""
    cands = np.concatenate([R.lut_bootstrap(orc, lo_recs, w_lo, bias_lo, row, theta1) for row in tv1])
    assert cands.shape[0] == p_hi
    a, b = pack_boxes(cands, pk, t, basebit, p_hi)
    return lut_enc(orc, hi_recs, w_hi, bias_hi, a[0], b[0], 1)[0], cands, (a[0], b[0])
