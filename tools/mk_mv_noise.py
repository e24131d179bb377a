#!/usr/bin/env python3
"""The blind rotation's own noise sigma_br on the 3-gen multi-key parameter sets, measured on the CPU oracle (no GPU), and the margins of a
multi-value output that follow from it.

Method: full-size keys from oracle_lib.SIGMAS (one key seed per set); the base vector 2^60 at every coefficient rotated by fresh encryptions of
random words through the oracle's party-major CMux chain (tests/mk_mv_lut_reference.py: rotate); the ring phase body - mask * sum_i z_i of all N
coefficients against +-2^60; sigma_br = the standard deviation of the error over rotations x N coefficients, in torus units.  sigma_ks is section
4.8's formula.  An output with taps c carries |c|_2 sigma_br (+) sigma_ks; the table gives half-step / sigma_out for outputs at modulus p_out = 2
(the gate encoding, half-step 1/8).

usage: python tools/mk_mv_noise.py [--rotations 8] [set ...]        (default sets: MK2 MK3 MK4 MK5 MK8 MK4-N2048 MK16)
"""
import argparse
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import mk_lut_reference as R       # noqa: E402
import mk_mv_lut_reference as MV   # noqa: E402
import oracle_lib as O             # noqa: E402

NORMS = (1.4, 2.6, 3.5, 7.5, 20.0)


def sigma_ks(p, s):
    """section 4.8: P key switches of the N-word mask, t rows per word, rounding to t basebit bits against ternary ring keys"""
    return math.sqrt(p.parties * p.N * p.ks_t * s["ks"] ** 2 + p.parties * p.N * (2.0 / 3.0) * 2.0 ** (-2 * p.ks_t * p.ks_basebit) / 12.0)


def ring_phase_errors(K, acc, N, mu):
    """error of every coefficient's phase against the nearer of +-mu, as floats in torus units"""
    z = np.ascontiguousarray(K.rlwe_keys.astype(np.int64).sum(axis=0))
    az = np.zeros(N, np.int64)
    O.lib().oracle_polymul_schoolbook64(O.p64(np.ascontiguousarray(acc[:N])), O.p64(z), N, O.p64(az))
    ph = (acc[N:].view(np.uint64) - az.view(np.uint64)).view(np.int64)
    e = np.where(ph >= 0, ph - mu, ph + mu)   # int64 wrap cannot occur: |ph| stays near mu = 2^60
    return e.astype(np.float64) / 2.0 ** 64


def measure(name, rotations, seed=0x5EED):
    p, s = O.make_params(name), O.SIGMAS[name]
    t0 = time.time()
    K = O.MKKeys(p, seed, s["bk"], s["ks"])
    orc = O.MKOracle(p, K.bk, K.ksk)
    rng = np.random.default_rng(seed)
    x = R.encrypt_words(K, rng.integers(-2**31, 2**31, rotations), s["lwe"], seed + 1)
    mu = 1 << 60
    tv0 = np.full(p.N, mu, np.int64)
    errs = []
    t1 = time.time()
    for g in range(rotations):
        errs.append(ring_phase_errors(K, MV.rotate(orc, x[g], tv0), p.N, mu))
    e = np.concatenate(errs)
    per = [float(np.sqrt(np.mean(v ** 2))) for v in errs]
    return dict(set=name, rotations=rotations, sigma_br=float(np.sqrt(np.mean(e ** 2))), sigma_br_min=min(per), sigma_br_max=max(per), mean=float(e.mean()),
                sigma_ks=sigma_ks(p, s), keygen_s=round(t1 - t0, 1), s_per_rotation=round((time.time() - t1) / rotations, 2))


def margins(sigma_br, sks):
    return [0.125 / math.hypot(c * sigma_br, sks) for c in NORMS]


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rotations", type=int, default=8)
    ap.add_argument("sets", nargs="*", default=["MK2", "MK3", "MK4", "MK5", "MK8", "MK4-N2048", "MK16"])
    a = ap.parse_args()
    for name in a.sets:
        r = measure(name, a.rotations)
        m = " | ".join("%.1f" % v for v in margins(r["sigma_br"], r["sigma_ks"]))
        print("| %s | %d | %.2e (%.2e .. %.2e) | %.2e | %s |   # mean %.1e, keygen %.1f s, %.2f s / rotation" % (
            r["set"], r["rotations"], r["sigma_br"], r["sigma_br_min"], r["sigma_br_max"], r["sigma_ks"], m, r["mean"], r["keygen_s"], r["s_per_rotation"]), flush=True)
