"""Reference of the leveled table lookup (include/thfhe_hip.h: thfhe_lhe_cmux, thfhe_lhe_lookup) -- TEST INFRASTRUCTURE
ONLY, composed from the CPU oracle's exact pieces: oracle_decompose32, the exact NTT product, oracle_mul_by_monomial32, the extraction of
lut_reference.py and the oracle's key switch.  Nothing here imports the product's code.

A TGSW sample C is int32[2l][2][N] in the bootstrapping key's layout (row j l + level, column 0 mask / 1 body); a TLWE sample is int32[2N] =
(mask, body), phase body - mask (*) z."""
import numpy as np

import lut_reference as R
import oracle_lib as O


def _add(x, y):
    return (np.asarray(x, np.int64) + np.asarray(y, np.int64)).astype(np.uint32).view(np.int32)


def _sub(x, y):
    return (np.asarray(x, np.int64) - np.asarray(y, np.int64)).astype(np.uint32).view(np.int32)


def polymul(small, torus, N):
    """small (*) torus mod (X^N + 1, 2^32), exact (oracle_polymul_ntt32)."""
    small = np.ascontiguousarray(small, np.int32)
    torus = np.ascontiguousarray(torus, np.int32)
    out = np.zeros(N, np.int32)
    O.lib().oracle_polymul_ntt32(O.p32(small), O.p32(torus), N, O.p32(out))
    return out


def decompose(poly, p):
    """the l balanced digit polynomials of a Torus32 polynomial: int32[l][N] (oracle_decompose32, J/tgsw.jl:112-138)"""
    poly = np.ascontiguousarray(poly, np.int32)
    out = np.zeros((p.l, p.N), np.int32)
    O.lib().oracle_decompose32(O.p32(poly), p.N, p.l, p.Bgbit, O.p32(out))
    return out


def extern_mul(p, C, d):
    """C (.) d: sum over the 2l digit polynomials of d = (mask, body) of digit (*) row (tgsw_extern_mul, J/tgsw.jl:146-150) -> int32[2N]"""
    N = p.N
    digits = np.concatenate([decompose(d[:N], p), decompose(d[N:], p)])
    out = np.zeros(2 * N, np.int64)
    for r in range(2 * p.l):
        for c in range(2):
            out[c * N:(c + 1) * N] += polymul(digits[r], C[r][c], N)
    return out.astype(np.uint32).view(np.int32)


def cmux(p, C, d1, d0):
    """d0 + C (.) (d1 - d0)"""
    return _add(d0, extern_mul(p, C, _sub(d1, d0)))


def tree(p, Cs, leaves, bit0):
    """CMux tree over 2^t leaves (int32[2^t][2N]): level t pairs neighbours on the TGSW sample Cs[bit0 + t] -> int32[2N]"""
    nodes = [np.asarray(v, np.int32) for v in leaves]
    t = 0
    while len(nodes) > 1:
        nodes = [cmux(p, Cs[bit0 + t], nodes[2 * q + 1], nodes[2 * q]) for q in range(len(nodes) // 2)]
        t += 1
    return nodes[0]


def rotate_chain(p, Cs, acc, d_rot):
    """for i < d_rot: ACC += Cs[i] (.) (X^(2N - box 2^i) ACC - ACC), box = N >> d_rot"""
    N = p.N
    box = N >> d_rot
    for i in range(d_rot):
        a = 2 * N - box * (1 << i)
        rot = np.concatenate([R.monomial(acc[:N], a, N), R.monomial(acc[N:], a, N)])
        acc = _add(acc, extern_mul(p, Cs[i], _sub(rot, acc)))
    return acc


def lookup_wo_keyswitch(p, Cs, tab_a, tab_b, d_tree, d_rot, theta):
    """One sample: Cs int32[d][2l][2][N] its address bits, (tab_a, tab_b) int32[2^d_tree][N] its table (tab_a None: public) -> int32[theta][N+1]"""
    N = p.N
    tab_b = np.asarray(tab_b, np.int32).reshape(1 << d_tree, N)
    tab_a = np.zeros_like(tab_b) if tab_a is None else np.asarray(tab_a, np.int32).reshape(1 << d_tree, N)
    acc = tree(p, Cs, [np.concatenate([a, b]) for a, b in zip(tab_a, tab_b)], d_rot)
    acc = rotate_chain(p, Cs, acc, d_rot)
    return np.stack([R.extract_at(acc, j, N) for j in range(theta)])


def lookup(orc, Cs, tab_a, tab_b, d_tree, d_rot, theta, keyswitch=True):
    u = lookup_wo_keyswitch(orc.params, Cs, tab_a, tab_b, d_tree, d_rot, theta)
    return np.stack([orc.keyswitch(r) for r in u]) if keyswitch else u


def trivial_tgsw(p, bits):
    """noiseless TGSW samples with a zero mask: int32[len(bits)][2l][2][N], bit * 2^(32 - (level+1) Bgbit) on coefficient 0 of polynomial j of row (j, level)"""
    bits = np.asarray(bits, np.int64).reshape(-1)
    C = np.zeros((bits.shape[0], 2 * p.l, 2, p.N), np.int32)
    for j in range(2):
        for lv in range(p.l):
            C[:, j * p.l + lv, j, 0] = R.to_i32(bits << (32 - (lv + 1) * p.Bgbit))
    return C


def tlwe_phase(p, rlwe_key, d):
    """body - mask (*) z of a TLWE sample int32[2N]"""
    return _sub(d[p.N:], polymul(rlwe_key, d[:p.N], p.N))


def ring_phase(rlwe_key, recs):
    """phase of LWE(N) records under the extracted ring key"""
    recs = np.asarray(recs, np.int32).reshape(-1, len(rlwe_key) + 1).astype(np.int64)
    return (recs[:, -1] - (recs[:, :-1] * np.asarray(rlwe_key, np.int64)).sum(axis=1)).astype(np.uint32).view(np.int32)


def address_bits(addresses, d):
    a = np.asarray(addresses, np.int64).reshape(-1)
    return ((a[:, None] >> np.arange(d)[None, :]) & 1).astype(np.int32)


def table_polys(functions, d_tree, d_rot, N=1024):
    """the layout of thfhe_lhe_lookup, written out independently of thfhe.lut.lhe_table: functions int[theta][2^d] of Torus32 words"""
    F = np.asarray(functions, np.int64)
    box = N >> d_rot
    tab = np.zeros((1 << d_tree, N), np.int64)
    for j in range(F.shape[0]):
        for e in range(F.shape[1]):
            tab[e >> d_rot, (e % (1 << d_rot)) * box + j] = F[j, e]
    return R.to_i32(tab)
