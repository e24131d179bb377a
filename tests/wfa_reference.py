"""Reference of the layered automata on TGSW-encrypted bits (include/thfhe_hip.h: thfhe_lhe_wfa) -- TEST INFRASTRUCTURE
ONLY, built from lhe_reference.cmux (the CPU oracle's decomposition and exact NTT product), the extraction of lut_reference.py and the oracle's key
switch.  Nothing here imports the product's code.

An automaton is trans int[n_steps][n_states][2], step_bit int[n_steps] (step j reads bit step_bit[j] & 15 of set step_bit[j] >> 4), final weights
(fin_a, fin_b) int32[n_states][N] (fin_a None: trivial samples) and start int[n_out].  The TGSW samples of one sample are a list over the sets of
int32[d][2l][2][N]."""
import numpy as np

import lhe_reference as LR
import lut_reference as R


def layer0(p, Cs, trans, step_bit, fin_a, fin_b):
    """V_0 of one sample, int32[n_states][2N]: V_j[q] = cmux(C_j, d1 = V_(j+1)[trans[j][q][1]], d0 = V_(j+1)[trans[j][q][0]]), a copy where both agree"""
    fin_b = np.asarray(fin_b, np.int32)
    fin_a = np.zeros_like(fin_b) if fin_a is None else np.asarray(fin_a, np.int32)
    V = [np.concatenate([a, b]) for a, b in zip(fin_a, fin_b)]
    trans = np.asarray(trans)
    for j in range(trans.shape[0] - 1, -1, -1):
        C = Cs[int(step_bit[j]) >> 4][int(step_bit[j]) & 15]
        done = {}
        for t0, t1 in {(int(a), int(b)) for a, b in trans[j]}:
            done[t0, t1] = V[t0] if t0 == t1 else LR.cmux(p, C, V[t1], V[t0])
        V = [done[int(a), int(b)] for a, b in trans[j]]
    return V


def wfa_wo_keyswitch(p, Cs, trans, step_bit, fin_a, fin_b, theta, start):
    """one sample -> int32[n_out][theta][N+1]"""
    V = layer0(p, Cs, trans, step_bit, fin_a, fin_b)
    return np.stack([np.stack([R.extract_at(V[int(q)], j, p.N) for j in range(theta)]) for q in start])


def wfa(orc, Cs, trans, step_bit, fin_a, fin_b, theta, start, keyswitch=True):
    u = wfa_wo_keyswitch(orc.params, Cs, trans, step_bit, fin_a, fin_b, theta, start)
    return np.stack([orc.keyswitch(r) for r in u.reshape(-1, u.shape[-1])]).reshape(u.shape[0], theta, -1) if keyswitch else u


def batch(p, orc, sets, trans, step_bit, fin_a, fin_b, theta, start, table_index=None):
    """Every sample of the sets (a list of int32[count][d][2l][2][N]); fin_a / fin_b int32[n_tables][n_states][N] -> (wo int32[count][n_out][theta][N+1],
    ks int32[count][n_out][theta][n+1])"""
    from support import pmap
    count = sets[0].shape[0]
    idx = np.zeros(count, np.int64) if table_index is None else np.asarray(table_index)
    fin_b = np.asarray(fin_b, np.int32).reshape(-1, np.asarray(trans).shape[1], p.N)
    fin_a = None if fin_a is None else np.asarray(fin_a, np.int32).reshape(fin_b.shape)
    wo = np.stack(pmap(lambda s: wfa_wo_keyswitch(p, [C[s] for C in sets], trans, step_bit, None if fin_a is None else fin_a[idx[s]], fin_b[idx[s]],
                                                  theta, start), range(count)))
    ks = np.stack(pmap(orc.keyswitch, wo.reshape(-1, p.N + 1))).reshape(wo.shape[:3] + (-1,))
    return wo, ks
