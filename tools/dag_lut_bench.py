#!/usr/bin/env python3
"""LUT nodes in the gate-DAG executor: cost of the DAG path and what LUT arithmetic saves, in one process on one device.

(a) SK-128: one level of 4 096 theta = 1 LUT nodes (thfhe_dag_run_lut_batch, operands read from the wire table by the fused prologue)
    against thfhe_lut_bootstrap on the same 4 096 samples.
(b) SK-128 and MK2: Q = 256 and Q = 2 048 instances of a 32-bit add -- circuits.full_adder (gate DAG, thfhe_dag_run_batch) against
    circuits.lut_ripple_add (LUT DAG, one theta = 2 node per bit).  Levels, rotations, wall time and additions per second.
Every call is a host-buffer call that synchronises the device before it returns (uploads, the run, the download of the selected wires);
wall time around it.  Each workload is warmed up once, then the workloads alternate for --reps rounds; the median is kept.
Prints one JSON line and writes it to --out.

usage: python tools/dag_lut_bench.py [--reps 5] [--device 0] [--out profiles/r07_dag_lut_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "torus-fhe_amd"))
import thfhe  # noqa: E402
from thfhe import circuits as Cc, keygen, lut  # noqa: E402


def _timed(run):
    t = time.perf_counter()
    run()
    return (time.perf_counter() - t) * 1e3


def _adders(ck, words, Q, rng, N, torus_bits):
    """The two 32-bit adders as (circuit, inputs, output wires); random input words (timing only)."""
    g = Cc.Circuit()
    a, b, z = g.inputs(32), g.inputs(32), g.inputs(1)[0]
    s, carry = Cc.full_adder(g, a, b, z)
    g_out = s + [carry[0]]
    L = Cc.Circuit()
    a, b = L.inputs(32), L.inputs(32)
    s, cy = Cc.lut_ripple_add(L, a, b, N=N, torus_bits=torus_bits)
    l_out = s + [cy]
    xg = rng.integers(-2**31, 2**31, (Q, g.n_inputs, words)).astype(np.int32)
    xl = rng.integers(-2**31, 2**31, (Q, L.n_inputs, words)).astype(np.int32)
    return (g, xg, g_out), (L, xl, l_out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07_dag_lut_bench.json"))
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    res = dict(tool="dag_lut_bench", device=args.device, reps=args.reps, timing="wall, host-buffer calls (device synchronised), median")

    # (a) one level of 4 096 theta = 1 nodes against thfhe_lut_bootstrap
    p = thfhe.make_params("SK-128")
    K = keygen.SecretKeySet(p, seed=0x5EED0001)
    ck = thfhe.CloudKey(p, K.bk, K.ksk, device=args.device)
    B = 4096
    tv = lut.test_vector(lut.int_outputs(lambda m: (m + 1) % 4, 4), 4)
    c = Cc.Circuit()
    x = c.inputs(1)
    t = c.table(tv)
    c.lut(t, x)
    xs = K.encrypt(rng.integers(0, 2, B), 1).reshape(B, 1, -1)
    work = {"lut_bootstrap_4096": lambda: ck.lut_bootstrap(tv, xs[:, 0]),
            "dag_level_4096": lambda: Cc.evaluate_batch(ck, c, xs, [1])}
    for run in work.values():
        run()
    ms = {k: [] for k in work}
    for _ in range(args.reps):
        for k, run in work.items():
            ms[k].append(_timed(run))
    med = {k: statistics.median(v) for k, v in ms.items()}
    res["a"] = dict(params="SK-128", samples=B, ms={k: round(v, 3) for k, v in med.items()},
                    ms_min={k: round(min(v), 3) for k, v in ms.items()}, ms_max={k: round(max(v), 3) for k, v in ms.items()},
                    dag_vs_lut_bootstrap_rate=round(med["lut_bootstrap_4096"] / med["dag_level_4096"], 4))

    # (b) 32-bit adders, SK-128 and MK2
    res["b"] = {}
    keys = [("SK-128", ck, 1024, 32)]
    mp = thfhe.make_params("MK2")
    MK = keygen.MKSecretKeySet(mp, seed=0x5EED0002, device=args.device)
    keys.append(("MK2", thfhe.MKCloudKey(mp, MK.bk, MK.ksk, device=args.device), mp.N, 64))
    for name, key, N, tb in keys:
        for Q in (256, 2048):
            (g, xg, g_out), (L, xl, l_out) = _adders(key, key.words, Q, rng, N, tb)
            st = {"full_adder": {}, "lut_ripple_add": {}}
            work = {"full_adder": lambda: Cc.evaluate_batch(key, g, xg, g_out, st["full_adder"]),
                    "lut_ripple_add": lambda: Cc.evaluate_batch(key, L, xl, l_out, st["lut_ripple_add"])}
            for run in work.values():
                run()
            ms = {k: [] for k in work}
            for _ in range(args.reps):
                for k, run in work.items():
                    ms[k].append(_timed(run))
            med = {k: statistics.median(v) for k, v in ms.items()}
            res["b"][f"{name}_Q{Q}"] = {k: dict(levels=st[k]["levels"], rotations_per_add=st[k]["rotations"] // Q, launches=st[k]["launches"],
                                                ms=round(med[k], 3), ms_min=round(min(ms[k]), 3), ms_max=round(max(ms[k]), 3),
                                                adds_per_s=round(Q / med[k] * 1e3, 1)) for k in work}
            res["b"][f"{name}_Q{Q}"]["lut_vs_gate_speedup"] = round(med["full_adder"] / med["lut_ripple_add"], 3)
        key.close()
    line = json.dumps(res)
    print(line, flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
