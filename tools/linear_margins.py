#!/usr/bin/env python3
"""Noise margins of an encrypted dense layer, from the CPU oracle alone (SK-128; no GPU).

Measured, on `--samples` records each:
  sigma_fresh  the phase error of fresh encryptions (the set's 2^-15);
  sigma_ms     the error the theta = 1 mod-switch to Z_2N adds to a record's phase (section 4.7's term), from the mod-switched words and the key;
  sigma_boot   the phase error of a programmable bootstrap's key-switched output (identity table at p = 4 on fresh inputs);
  two layers   the network of tests/test_gpu_linear.py (7 fresh bits -> 3 threshold neurons -> majority): the phase error of the layer-1 sums, of the
               layer-1 outputs and of the layer-2 sums, against the rule below.
Rule: Var(x_m) = sum_k W[m][k]^2 Var(in_k); the table then sees sigma = sqrt(Var(x_m) + sigma_ms^2) against a half-box of 1 / (4p).
The table printed last applies the rule to fresh and to bootstrapped inputs for several |W_m|^2 and p.  Writes one JSON document to --out.

usage: python tools/linear_margins.py [--samples 256] [--out profiles/linear_margins.json]
"""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "torus-fhe_amd")):
    sys.path.insert(0, d)
import linear_reference as LR      # noqa: E402
import lut_reference as R          # noqa: E402
import oracle_lib as O             # noqa: E402
from support import pmap           # noqa: E402
from thfhe import circuits, lut    # noqa: E402


def centred(words):
    w = np.asarray(words, np.int64) & 0xFFFFFFFF
    return ((w + (1 << 31)) % (1 << 32) - (1 << 31)) / 2.0**32


def phase_error(K, recs, msgs, p):
    """phase minus the encoded message, as a real in [-1/2, 1/2)"""
    return centred(K.phases(recs).astype(np.int64) - lut.encode(np.asarray(msgs), p).astype(np.int64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "linear_margins.json"))
    args = ap.parse_args()
    p = O.make_params("SK-128")
    s = O.SIGMAS["SK-128"]
    K = O.SKKeys(p, 0x5EED0001, s["bk"], s["ks"], lwe_key=O.fixture_key())
    orc = O.Oracle(p, K.bk, K.ksk)
    n, N, B = p.n, p.N, args.samples
    rng = np.random.default_rng(7)

    m = rng.integers(0, 4, B)
    x = R.encrypt_words(K, lut.encode(m, 4), s["lwe"], 11)
    sigma_fresh = float(np.std(phase_error(K, x, m, 4)))
    # the mod-switch: phase of the rounded record (words bar * 2^32 / 2N) against the phase of the record itself
    bar = np.array([[O.lib().oracle_modswitch(int(w), N) for w in r] for r in x], np.int64)
    sigma_ms = float(np.std(centred(K.phases(R.to_i32(bar * ((1 << 32) // (2 * N)))).astype(np.int64) - K.phases(x).astype(np.int64))))
    ident = lut.test_vector(lut.int_outputs(lambda v: v, 4), 4)
    y = np.stack(pmap(lambda g: R.lut_bootstrap(orc, [x[g]], (1,), 0, ident, 1)[0], range(B)))
    sigma_boot = float(np.std(phase_error(K, y, m, 4)))

    # the two-layer network of the GPU test, on B samples
    W1 = np.array([[1, 1, 1, 1, 1, 1, 1], [1, 1, 1, 1, 0, 0, 0], [1, 0, 1, 0, 1, 0, 1]], np.int32)
    thr = np.array([4, 2, 2])
    W2 = np.array([[1, 1, 1]], np.int32)
    tv1 = np.stack([lut.test_vector(lut.int_outputs(lambda v, t=t: int(v >= t), 4, 8), 8) for t in thr])
    tv2 = lut.test_vector(lut.int_outputs(lambda v: int(v >= 2), 4, 4), 4)[None]
    S = max(8, B // 8)
    bits = rng.integers(0, 2, (S, 7))
    xb = R.encrypt_words(K, lut.encode(bits.reshape(-1), 8), s["lwe"], 12).reshape(S, 7, n + 1)
    sums1 = circuits.dense_plain(W1, None, bits, 8)
    want1 = (sums1 >= thr).astype(np.int64)
    sums2 = circuits.dense_plain(W2, None, want1, 4)
    want2 = (sums2 >= 2).astype(np.int64)
    e_x1 = phase_error(K, LR.linear(W1, xb).reshape(-1, n + 1), sums1.reshape(-1), 8).reshape(S, 3)
    h = LR.fused(R.lut_bootstrap, orc, W1, xb, None, tv1, 1, np.arange(3), True, pmap).reshape(S, 3, n + 1)
    e_h = phase_error(K, h.reshape(-1, n + 1), want1.reshape(-1), 4)
    e_x2 = phase_error(K, LR.linear(W2, h).reshape(-1, n + 1), sums2.reshape(-1), 4)
    out2 = LR.fused(R.lut_bootstrap, orc, W2, h, None, tv2, 1, None, True, pmap).reshape(S, n + 1)
    e_out = phase_error(K, out2, want2.reshape(-1), 4)
    wrong = int((lut.decode(K.phases(h.reshape(-1, n + 1)), 4) != want1.reshape(-1)).sum() + (lut.decode(K.phases(out2), 4) != want2.reshape(-1)).sum())

    def margin(norm2, sigma_in, pp):
        sig = math.sqrt(norm2 * sigma_in**2 + sigma_ms**2)
        return sig, (1.0 / (4 * pp)) / sig

    table = []
    for kind, sig_in in (("fresh", sigma_fresh), ("bootstrapped", sigma_boot)):
        for norm2 in (1, 3, 7, 16, 64, 256, 784):
            row = dict(inputs=kind, norm2=norm2)
            for pp in (4, 8, 16, 32):
                sig, mg = margin(norm2, sig_in, pp)
                row["sigma"] = round(sig, 6)
                row[f"p{pp}"] = round(mg, 1)
            table.append(row)
    res = dict(tool="linear_margins", params="SK-128", samples=B, network_samples=S,
               sigma_fresh=sigma_fresh, sigma_modswitch=sigma_ms, sigma_modswitch_derived=math.sqrt((n / 2 + 1) / 12.0) / (2 * N), sigma_bootstrapped=sigma_boot,
               network=dict(layer1_sum_sigma=[float(v) for v in e_x1.std(axis=0)], layer1_sum_rule=[float(math.sqrt(r) * sigma_fresh) for r in (W1.astype(np.int64)**2).sum(axis=1)],
                            layer1_margin=margin(7, sigma_fresh, 8)[1], layer1_out_sigma=float(e_h.std()), layer2_sum_sigma=float(e_x2.std()),
                            layer2_sum_rule=math.sqrt(3) * float(e_h.std()), layer2_margin=margin(3, float(e_h.std()), 4)[1], out_sigma=float(e_out.std()),
                            wrong_decryptions=wrong),
               margins=table)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in res.items() if k != "margins"}, indent=1))
    print("| inputs | sum of squared weights | sigma at the table | margin p=4 | p=8 | p=16 | p=32 |\n|---|---|---|---|---|---|---|")
    for r in table:
        print(f"| {r['inputs']} | {r['norm2']} | {r['sigma']:.2e} | {r['p4']} | {r['p8']} | {r['p16']} | {r['p32']} |")


if __name__ == "__main__":
    main()
