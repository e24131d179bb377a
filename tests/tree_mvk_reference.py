"""Reference of the k-output two-digit tree with a multi-value level 1 (include/thfhe_hip.h: thfhe_tree_lut_bootstrap_mvk; DESIGN.md section
4.14) -- TEST INFRASTRUCTURE ONLY, composed from the existing reference modules: mv_lut_reference.mv_lut (one rotation, k p_hi outputs),
tree_lut_reference.pack_boxes (k tables of p_hi candidates) and tree_lut_reference.lut_enc (one selection per table).  Nothing here imports the
product's code."""
import numpy as np

import mv_lut_reference as MV
import tree_lut_reference as TR


def tree_mvk(orc, pk, t, basebit, lo_recs, w_lo, bias_lo, hi_recs, w_hi, bias_hi, tv0, factors):
    """Reference of thfhe_tree_lut_bootstrap_mvk for one sample: factors int[k][p_hi][p_lo] = its table.  Returns (out int32[k][n+1], candidates
    int32[k p_hi][n+1]); candidate j p_hi + h is candidate h of function j."""
    factors = np.asarray(factors)
    k, p_hi, p_lo = factors.shape
    cands = MV.mv_lut(orc, lo_recs, w_lo, bias_lo, tv0, factors.reshape(k * p_hi, p_lo))
    a, b = TR.pack_boxes(cands, pk, t, basebit, p_hi)
    return np.stack([TR.lut_enc(orc, hi_recs, w_hi, bias_hi, a[j], b[j], 1)[0] for j in range(k)]), cands
