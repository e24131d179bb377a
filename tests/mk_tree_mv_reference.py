"""Reference of the multi-value two-digit tree of the 3-gen engine (include/thfhe_hip.h, thfhe_mk_tree_lut_bootstrap_mvk) --
TEST INFRASTRUCTURE ONLY.  No arithmetic of its own: the multi-value rotation of tests/mk_mv_lut_reference.py, the packing and the rotation on an
encrypted table of tests/mk_pack_reference.py, composed in the order the contract names."""
import numpy as np

import mk_mv_lut_reference as MV
import mk_pack_reference as MP


def tree_mvk(orc, pk, t, basebit, tv0, factors, lo, hi, weights_lo=(1,), bias_lo=0, weights_hi=(1,), bias_hi=0, out_bias=0, parts=False):
    """One sample: factors int[k][p_hi][p_lo] its table, lo / hi the lists of its operand records, pk the D = N packing key -> int32[k][P n + 1].
    Level-1 output j p_hi + h is candidate h of function j; packed table j holds candidates j p_hi .. j p_hi + p_hi - 1.
    parts: also return the candidates and the packed tables."""
    w = np.asarray(factors)
    k, p_hi, p_lo = w.shape
    cand = MV.mv_lut(orc, lo, weights_lo, bias_lo, tv0, w.reshape(k * p_hi, p_lo), out_bias, keyswitch=False)
    assert cand.shape[0] == k * p_hi
    ta, tb = MP.pack(cand, pk, t, basebit, p_hi)
    out = np.stack([MP.lut_bootstrap_enc(orc, hi, weights_hi, bias_hi, ta[j], tb[j], 1)[0] for j in range(k)])
    return (out, cand, ta, tb) if parts else out
