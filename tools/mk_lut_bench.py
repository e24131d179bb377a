#!/usr/bin/env python3
"""Multi-key programmable bootstrapping throughput against the NAND gate, in one process on one device (3-gen sets).

Times thfhe_mk_lut_bootstrap on 1024 samples at theta = 1, 2 and 4 (MK2, MK4) and theta = 1 (MK4-N2048), and thfhe_mk_gates(NAND) on the
same batch.  Every call is timed by the context's device events (prologue start .. key-switch end, thfhe_mk_last_timings); the host-buffer
call synchronises its stream before the events are read.  Each shape is warmed up first, then the workloads of a set alternate for --reps
rounds; the median is kept.  Prints one JSON line.

usage: python tools/mk_lut_bench.py [--reps 7] [--device 0] [--batch 1024]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "torus-fhe_amd"))
import thfhe  # noqa: E402
from thfhe import keygen, lut  # noqa: E402

SETS = {"MK2": (1, 2, 4), "MK4": (1, 2, 4), "MK4-N2048": (1,)}


def bench_set(name, thetas, B, reps, device):
    p = thfhe.make_params(name)
    K = keygen.MKSecretKeySet(p, seed=1, sigma_lwe=2.0**-13.26, device=device)
    ck = thfhe.MKCloudKey(p, K.bk, K.ksk, device=device)
    rng = np.random.default_rng(0)
    xa, xb = K.encrypt(rng.integers(0, 2, B), 1), K.encrypt(rng.integers(0, 2, B), 2)
    work = {f"nand_{B}": lambda: ck.gates(thfhe.NAND, xa, xb)}
    for t in thetas:
        tv = lut.test_vector([lut.int_outputs(lambda m, j=j: (m + j) % 4, 4, torus_bits=64) for j in range(t)], 4, t, p.N, torus_bits=64)
        work[f"lut_{B}_theta{t}"] = lambda tv=tv, t=t: ck.lut_bootstrap(tv, xa, theta=t)
    ck.set_profiling(True)
    for run in work.values():   # warm-up: code objects loaded, workspace and staging grown for every shape
        run()
    ms = {k: [] for k in work}
    for _ in range(reps):       # alternate the workloads: drift of the machine hits all of them alike
        for k, run in work.items():
            run()
            ms[k].append(ck.last_timings()["total_ms"])
    ck.set_profiling(False)
    ck.close()
    med = {k: statistics.median(v) for k, v in ms.items()}
    rate = {k: B / med[k] * 1e3 for k in work}   # samples (gates) per second
    return dict(ms={k: round(v, 3) for k, v in med.items()}, ms_min={k: round(min(v), 3) for k, v in ms.items()},
                ms_max={k: round(max(v), 3) for k, v in ms.items()}, samples_per_s={k: round(v) for k, v in rate.items()},
                lut_theta1_vs_nand=round(rate[f"lut_{B}_theta1"] / rate[f"nand_{B}"], 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--batch", type=int, default=1024)
    args = ap.parse_args()
    res = dict(tool="mk_lut_bench", device=args.device, reps=args.reps, batch=args.batch, timing="device events, prologue .. key switch, median",
               sets={name: bench_set(name, thetas, args.batch, args.reps, args.device) for name, thetas in SETS.items()})
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
