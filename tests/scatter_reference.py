"""Reference of the leveled scatter (include/thfhe_hip.h: thfhe_lhe_demux, thfhe_lhe_scatter) -- TEST INFRASTRUCTURE ONLY,
built on lhe_reference.py's exact pieces (cmux, extern_mul: oracle_decompose32 and the exact NTT product) and the oracle's monomial product.
Nothing here imports the product's code.

A TGSW sample C is int32[2l][2][N]; a TLWE sample is int32[2N] = (mask, body); a table is int32[n_tables][2^d_tree][2N]."""
import numpy as np

import lhe_reference as LR
import lut_reference as R


def demux(p, C, x):
    """(child 0, child 1): child 1 = C (.) x as the CMux 0 + C (.) (x - 0), child 0 = x - child 1"""
    x = np.asarray(x, np.int32)
    one = LR.cmux(p, C, x, np.zeros_like(x))
    return LR._sub(x, one), one


def rotate_chain_up(p, Cs, acc, d_rot):
    """for i < d_rot: ACC += Cs[i] (.) (X^(box 2^i) ACC - ACC), box = N >> d_rot -- the mirror of lhe_reference.rotate_chain"""
    N = p.N
    box = N >> d_rot
    for i in range(d_rot):
        a = box << i
        rot = np.concatenate([R.monomial(acc[:N], a, N), R.monomial(acc[N:], a, N)])
        acc = LR._add(acc, LR.extern_mul(p, Cs[i], LR._sub(rot, acc)))
    return acc


def scatter_wo_reduce(p, Cs, v, d_tree, d_rot):
    """One sample: Cs int32[d][2l][2][N] its address bits, v int32[2N] its value -> the 2^d_tree leaves int32[2^d_tree][2N]; the node at depth k
    splits on bit d-1-k, so leaf P = sum_t bit_(d_rot+t) 2^t carries the rotated value"""
    d = d_tree + d_rot
    nodes = [rotate_chain_up(p, Cs, np.asarray(v, np.int32), d_rot)]   # index = the prefix, highest bit first
    for k in range(d_tree):
        nxt = []
        for x in nodes:
            nxt.extend(demux(p, Cs[d - 1 - k], x))
        nodes = nxt
    # a prefix lists the bits from d-1 down, so as a number it IS sum_t bit_(d_rot+t) 2^t
    return np.stack(nodes)


def scatter(p, Cs, vals, d_tree, d_rot, val_index=None, n_tables=1, table_index=None):
    """Cs int32[count][d][2l][2][N], vals int32[n_vals][2N] -> int32[n_tables][2^d_tree][2N]"""
    count = len(Cs)
    vals = np.asarray(vals, np.int32).reshape(-1, 2 * p.N)
    if val_index is None:
        assert vals.shape[0] in (1, count)
        val_index = np.arange(count) if vals.shape[0] > 1 else np.zeros(count, np.int64)
    table_index = np.zeros(count, np.int64) if table_index is None else table_index
    tab = np.zeros((n_tables, 1 << d_tree, 2 * p.N), np.int64)
    for s in range(count):
        tab[table_index[s]] += scatter_wo_reduce(p, Cs[s], vals[val_index[s]], d_tree, d_rot)
    return tab.astype(np.uint32).view(np.int32)


def trivial(v_b):
    """the trivial sample(s) (0, v_b): int32[..., N] -> int32[..., 2N]"""
    v_b = np.asarray(v_b, np.int32)
    return np.concatenate([np.zeros_like(v_b), v_b], axis=-1)
