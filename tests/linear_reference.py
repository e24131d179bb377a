"""Reference of the encrypted dense layer (include/thfhe_hip.h, thfhe_lwe_linear / thfhe_linear_lut_bootstrap and their thfhe_mk_ forms) --
TEST INFRASTRUCTURE ONLY.  x from its definition in numpy (int64 products of int32 values cannot overflow singly; the running sum is wrapped after
every term), and the fused model: x, then lut_reference.lut_bootstrap / mk_lut_reference.lut_bootstrap with weights (1,), bias 0 on table
lut_index[m].  tests/test_linear_host.py checks `linear` against Python's big integers on the edge values."""
import numpy as np

EDGE_WEIGHTS = [0, 1, -1, 2**31 - 1, -2**31]
EDGE_WORDS = [0, -1, 2**31 - 1, -2**31]


def to_i32(v):
    return (np.asarray(v, np.int64) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)


def linear(W, x, bias=None):
    """x int32[count][K][rec], W int32[M][K], bias int32[M] or None -> int32[count][M][rec]:
    out[s][m][i] = sum_k W[m][k] x[s][k][i] + (i == rec - 1 ? bias[m] : 0) mod 2^32."""
    W = np.asarray(W, np.int64)
    x = np.asarray(x, np.int64)
    count, K, rec = x.shape
    M = W.shape[0]
    acc = np.zeros((count, M, rec), np.int64)
    for k in range(K):
        # |W| <= 2^31 and |x| <= 2^31: a product is at most 2^62 in magnitude and the wrapped sum below 2^32, so int64 never overflows
        acc = (acc + W[None, :, k, None] * x[:, None, k, :]) & 0xFFFFFFFF
    if bias is not None:
        acc[:, :, rec - 1] = (acc[:, :, rec - 1] + np.asarray(bias, np.int64)[None, :]) & 0xFFFFFFFF
    return to_i32(acc)


def linear_bigint(W, x, bias=None):
    """the same in Python integers of unbounded size, one word at a time"""
    W, x = np.asarray(W), np.asarray(x)
    count, K, rec = x.shape
    M = W.shape[0]
    out = np.empty((count, M, rec), np.int32)
    for s in range(count):
        for m in range(M):
            for i in range(rec):
                v = sum(int(W[m, k]) * int(x[s, k, i]) for k in range(K))
                if bias is not None and i == rec - 1:
                    v += int(bias[m])
                v &= 0xFFFFFFFF
                out[s, m, i] = v - (1 << 32) if v >= 1 << 31 else v
    return out


def fused(lut_bootstrap, orc, W, x, bias, tv, theta, lut_index, keyswitch, pmap=map):
    """The fused call's model: lut_bootstrap = lut_reference.lut_bootstrap or mk_lut_reference.lut_bootstrap (one sample per call).
    Returns int32[count][M][theta][words]."""
    xs = linear(W, x, bias)
    count, M, _ = xs.shape
    jobs = [(s, m) for s in range(count) for m in range(M)]
    out = list(pmap(lambda sm: lut_bootstrap(orc, [xs[sm[0], sm[1]]], (1,), 0, tv[0 if lut_index is None else lut_index[sm[1]]], theta, keyswitch=keyswitch), jobs))
    return np.stack(out).reshape(count, M, theta, -1)
