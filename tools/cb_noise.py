#!/usr/bin/env python3
"""Noise of circuit bootstrapping, on the CPU only: the prediction of a TGSW row's noise for the tabulated key noises and
digit shapes, what a CMux and a d = 10 lookup on such a set then carry on SK-128 and SK-80, and a measurement of stage A and of a row on the CPU
model (tests/cb_reference.py with the oracle's 3-gen rotation) at FULL n, 8 rotations.

  sigma_row^2 = D t (B^2 / 12) sigma_pks^2 + (|z2|^2 / 3) 2^(-2 (t basebit + 1)) + sigma_A^2
  sigma_A^2   = n ((1 + |z2|^2) 2^(-2 (l2 Bgbit2 + 1)) / 3 + 2 l2 N2 (Bg2^2 / 12) sigma_bk2^2) + |z2|^2 2^-66 / 3
  sigma_cmux  = sqrt(2 l N) (Bg / sqrt(12)) sigma_row

Measured: sigma_A over `--coeffs` extracted coefficients of each of the 8 level-2 accumulators (rotation by a fresh gate-encoded record, mu_0, every
extraction through the oracle's Torus64 -> Torus32 conversion) against +-mu_0; sigma_row over the 8 x 2 x 1024 coefficients of the rows T_0, T_1
of those 8 records at level 0, with a key at sigma_pks = 2^-31 and (t, basebit) = (7, 4).

Input margin of stage A: the gate-encoded input sits at +-1/8, so stage A decides its bit while the input's phase error stays inside the half-box
1/8.  Two terms, as DESIGN 4.8: the mod-switch rounding sigma_ms = theta / (2 D) / sqrt(12) sqrt(n / 2 + 1) (theta = 1 in the default mode; the
smallest power of two >= l in one-rotation mode) and the gate output's key-switch noise from SIGMAS,
sigma_ks^2 = N t sigma_ks,row^2 + (N / 2) 2^(-2 t basebit) / 12 (binary ring key).  The project's threshold for "supported" is 6 sigma.

usage: python tools/cb_noise.py [--rotations 8] [--coeffs 64] [--set SK-128] [--no-measure]
"""
import argparse
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "torus-fhe_amd")]

import cb_reference as CB          # noqa: E402
import mk_lut_reference as R       # noqa: E402
import mk_mv_lut_reference as MV   # noqa: E402
import oracle_lib as O             # noqa: E402
import thfhe                       # noqa: E402
from thfhe import keygen           # noqa: E402

SIGMAS_PKS = (2.0**-25, 2.0**-28, 2.0**-31)
DIGITS = ((7, 4), (8, 4), (10, 3))
D2 = 2048
Z2_NORM2 = 2 * 0.113546097609674 * D2      # expected |z2|^2 of a ternary key (keygen.rand_ternary)
QUARTER = 2.0**-5 / 4                      # a quarter of the half-step at p_out = 8


def sigma_cmux(p, srow):
    return math.sqrt(2 * p["l"] * p["N"] * 4.0 ** p["Bgbit"] / 12) * srow


def predictions():
    p2, s2 = thfhe.CB_PARAM_SETS["CB-128"], thfhe.CB_SIGMAS["CB-128"]
    print("| sigma_pks | (t, basebit) | key MiB | sigma_row | SK-128 CMux | SK-128 d = 10 | below 7.8e-3 | SK-80 CMux | SK-80 d = 10 |")
    print("|---|---|---|---|---|---|---|---|---|")
    for spk in SIGMAS_PKS:
        for t, b in DIGITS:
            cols = []
            for sk, cb in (("SK-128", "CB-128"), ("SK-80", "CB-80")):
                n = thfhe.PARAM_SETS[sk]["n"]
                sa = CB.sigma_a(n, p2["l"], p2["Bgbit"], D2, Z2_NORM2, s2["bk"])
                srow = CB.sigma_row(D2, t, b, spk, Z2_NORM2, sa)
                c = sigma_cmux(thfhe.PARAM_SETS[sk], srow)
                cols.append((srow, c, math.sqrt(10) * c))
            print("| 2^%d | (%d, %d) | %d | %.2e | %.2e | %.2e | %s | %.2e | %.2e |" % (
                round(math.log2(spk)), t, b, 2 * D2 * t * 8192 >> 20, cols[0][0], cols[0][1], cols[0][2], "yes" if cols[0][2] < QUARTER else "no",
                cols[1][1], cols[1][2]))


def input_margins():
    """half-box 1/8 over the input's phase error at stage A's mod-switch, per set and mode"""
    print("| set | l | theta | sigma_ks (gate output) | sigma_ms, one rotation | margin, one rotation | sigma_ms, per level | margin, per level (theta = 1) |")
    print("|---|---|---|---|---|---|---|---|")
    for sk, cb in (("SK-128", "CB-128"), ("SK-80", "CB-80")):
        p, s = thfhe.PARAM_SETS[sk], thfhe.SIGMAS[sk]
        D = thfhe.CB_PARAM_SETS[cb]["N"]
        theta = 1 if p["l"] == 1 else (2 if p["l"] == 2 else 4)
        sks = math.sqrt(p["N"] * p["ks_t"] * s["ks"] ** 2 + p["N"] / 2 * 4.0 ** (-p["ks_t"] * p["ks_basebit"]) / 12)
        ms = lambda th: th / (2 * D) / math.sqrt(12) * math.sqrt(p["n"] / 2 + 1)
        margin = lambda th: 0.125 / math.hypot(sks, ms(th))
        print("| %s / %s | %d | %d | %.2e | %.2e | %.1f sigma | %.2e | %.1f sigma |" % (sk, cb, p["l"], theta, sks, ms(theta), margin(theta), ms(1), margin(1)))
    print("threshold for \"supported\": 6 sigma.  One-rotation mode assumes gate-encoded inputs (+-1/8): an input with a smaller box is the caller's risk.")


def measure(name, rotations, coeffs, seed=0x5EED0C50):
    cb = {"SK-128": "CB-128", "SK-80": "CB-80"}[name]
    tp, s1 = thfhe.make_params(name), thfhe.SIGMAS[name]
    tp2, s2 = thfhe.make_params(**thfhe.CB_PARAM_SETS[cb]), thfhe.CB_SIGMAS[cb]
    t0 = time.time()
    K = keygen.SecretKeySet(tp, seed=seed, sigma_lwe=s1["lwe"], sigma_bk=s1["bk"], sigma_ks=s1["ks"])
    K2 = keygen.MKSecretKeySet(tp2, seed=seed + 1, sigma_lwe=s2["lwe"], sigma_bk=s2["bk"], sigma_ks=s2["ks"], lwe_keys=K.lwe_key[None, :])
    z2 = K2.rlwe_keys[0]
    z2n = float((z2.astype(np.float64) ** 2).sum())
    T, B = 7, 4
    pks = keygen.gen_cb_key(np.random.default_rng(seed + 2), z2, K.rlwe_key, T, B, 2.0**-31)
    orc2 = O.MKOracle(O.make_params(**tp2.as_dict()), K2.bk, K2.ksk)
    t1 = time.time()
    bits = np.random.default_rng(seed + 3).integers(0, 2, rotations)
    x = K.encrypt(bits, seed + 4)
    mu = 1 << (63 - tp.Bgbit)
    g0 = 1 << (32 - tp.Bgbit)
    errs, lwe2 = [], np.empty((rotations, 1, D2 + 1), np.int32)
    for r in range(rotations):
        acc = MV.rotate(orc2, x[r], np.full(D2, mu, np.int64))
        for j in range(coeffs):
            u = R.extract_at(acc, j, D2).astype(np.int64)
            ph = int(u[-1] - (u[:-1] * z2).sum() + (1 << (31 - tp.Bgbit)))          # + 2^(31 - Bgbit): 0 or g_0
            errs.append(int(CB.centred(ph - int(bits[r]) * g0)))
            if j == 0:
                u[-1] += 1 << (31 - tp.Bgbit)
                lwe2[r, 0] = u.astype(np.uint32).view(np.int32)
    t2 = time.time()
    sa_meas = float(np.std(np.array(errs, np.float64))) / 2.0**32
    sa_pred = CB.sigma_a(tp.n, tp2.l, tp2.Bgbit, D2, z2n, s2["bk"])
    rows = CB.private_keyswitch(pks, lwe2, 1, T, B)
    e = CB.row_errors(K, rows, bits, 1, tp.Bgbit)
    srow_meas = float(e.std()) / 2.0**32
    srow_pred = CB.sigma_row(D2, T, B, 2.0**-31, z2n, sa_pred)
    print("%s + %s, n = %d, |z2|^2 = %d: keys %.0f s, %d rotations %.0f s" % (name, cb, tp.n, z2n, t1 - t0, rotations, t2 - t1))
    print("| quantity | predicted | measured | ratio |")
    print("|---|---|---|---|")
    print("| sigma_A (%d rotations x %d coefficients) | %.2e | %.2e | %.2f |" % (rotations, coeffs, sa_pred, sa_meas, sa_meas / sa_pred))
    print("| sigma_row at sigma_pks = 2^-31, (7, 4) (%d coefficients) | %.2e | %.2e | %.2f |" % (e.size, srow_pred, srow_meas, srow_meas / srow_pred))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rotations", type=int, default=8)
    ap.add_argument("--coeffs", type=int, default=64)
    ap.add_argument("--set", default="SK-128")
    ap.add_argument("--no-measure", action="store_true")
    a = ap.parse_args()
    predictions()
    print()
    input_margins()
    print()
    if not a.no_measure:
        O.lib()
        measure(a.set, a.rotations, a.coeffs)
