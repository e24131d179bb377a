"""The cases tests/test_gpu_wfa.py runs on the device and tests/test_wfa_host.py runs on the CPU model first: SK-128 real
keys, wfa_less_than(8) and wfa_equal(8) on 8 samples.  Inputs and model outputs are built once per process and shared."""
import math

import numpy as np

import wfa_reference as WR
from support import N

WIDTH, P_OUT, THETA = 8, 8, 2
# equal operands, operands that differ in the top bit only and in the bottom bit only (both orders), and three unrelated pairs
A = np.array([0x5A, 0x80, 0x00, 0x01, 0x00, 0xC3, 0x17, 0xFF])
B = np.array([0x5A, 0x00, 0x80, 0x00, 0x01, 0x3C, 0xE8, 0xFE])
SEED = 4600


class Keys:
    def __init__(self, O, name="SK-128"):
        import thfhe
        from thfhe import keygen
        self.name, self.sig = name, thfhe.SIGMAS[name]
        self.tp = thfhe.make_params(name)
        self.K = keygen.SecretKeySet(self.tp, seed=0x5EED0100 + self.tp.n, sigma_lwe=self.sig["lwe"], sigma_bk=self.sig["bk"], sigma_ks=self.sig["ks"])
        self.p = O.make_params(name)
        self.orc = O.Oracle(self.p, self.K.bk, self.K.ksk)

    def sigma_cmux(self):
        return math.sqrt(2 * self.p.l * N * 4.0 ** self.p.Bgbit / 12) * self.sig["bk"]


_made = {}


def keys(O):
    if "keys" not in _made:
        _made["keys"] = Keys(O)
    return _made["keys"]


def case(O, which):
    """which: "less_than" or "equal" -> dict of the automaton, the TGSW samples of the two sets, the finals (f at coefficient 0, 1 - f at
    coefficient 1, modulus P_OUT), the plain result, the non-copy steps of every sample's path and the model's records"""
    if which not in _made:
        from thfhe import circuits, lut
        S = keys(O)
        aut = (circuits.wfa_less_than if which == "less_than" else circuits.wfa_equal)(WIDTH)
        trans, step_bit, fin, start = aut
        bits = circuits.wfa_pair_bits(A, B, WIDTH)
        sets = [S.K.tgsw_encrypt(b.reshape(-1), seed=SEED + 10 * i + len(which)).reshape(len(A), WIDTH, 2 * S.p.l, 2, N) for i, b in enumerate(bits)]
        fin_b = lut.wfa_finals(np.concatenate([fin, 1 - fin]), THETA, encode=lambda v: lut.encode(v, P_OUT))
        f = circuits.wfa_run_plain(aut, bits)[:, :, 0]
        want = np.stack([f, 1 - f], axis=-1)                       # [count][n_out][theta]
        wo, ks = WR.batch(S.p, S.orc, sets, trans, step_bit, None, fin_b, THETA, start)
        _made[which] = dict(aut=aut, bits=bits, sets=sets, fin_b=fin_b, want=want, steps=circuits.wfa_noise_steps(aut, bits), wo=wo, ks=ks)
    return _made[which]


def noise(S, recs_wo, want):
    """std of phase - encode over ring-key records (torus units)"""
    from thfhe import lut
    ph = S.K.ring_phase(recs_wo).reshape(want.shape).astype(np.int64)
    err = (ph - lut.encode(want, P_OUT).astype(np.int64) + 2**31) % 2**32 - 2**31
    return float(err.std()) / 2.0**32


def predicted(S, cases):
    """sqrt(mean number of non-copy steps on a path) sigma_1"""
    return math.sqrt(float(np.mean(np.concatenate([c["steps"].reshape(-1) for c in cases])))) * S.sigma_cmux()
