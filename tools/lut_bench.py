#!/usr/bin/env python3
"""Programmable bootstrapping throughput against the NAND gate, in one process on one device (SK-128).

Times thfhe_lut_bootstrap on 4096 and 1024 samples at theta = 1, 2 and 4 and thfhe_gates(NAND) on the same batch sizes.  Every call is
timed by the context's device events (prologue start .. key-switch end, thfhe_last_timings); the host-buffer call synchronises its
stream before the events are read.  Each shape is warmed up first, then the workloads alternate for --reps rounds; the median is kept.
Prints one JSON line.

usage: python tools/lut_bench.py [--reps 7] [--device 0]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    p = thfhe.make_params("SK-128")
    K = keygen.SecretKeySet(p, seed=0x5EED0001)
    ck = thfhe.CloudKey(p, K.bk, K.ksk, device=args.device)
    rng = np.random.default_rng(0)
    xa, xb = K.encrypt(rng.integers(0, 2, 4096), 1), K.encrypt(rng.integers(0, 2, 4096), 2)
    tables = {t: lut.test_vector([lut.int_outputs(lambda m, j=j: (m + j) % 4, 4) for j in range(t)], 4, theta=t) for t in (1, 2, 4)}

    work = {}
    for B in (4096, 1024):
        work[f"nand_{B}"] = (B, lambda B=B: ck.gates(thfhe.NAND, xa[:B], xb[:B]))
        for t in (1, 2, 4):
            work[f"lut_{B}_theta{t}"] = (B, lambda B=B, t=t: ck.lut_bootstrap(tables[t], xa[:B], theta=t))
    ck.set_profiling(True)
    for _, (_, run) in work.items():   # warm-up: code objects loaded, workspace and staging grown for every shape
        run()
    ms = {k: [] for k in work}
    for _ in range(args.reps):         # alternate the workloads: drift of the machine hits all of them alike
        for k, (_, run) in work.items():
            run()
            ms[k].append(ck.last_timings()["total_ms"])
    ck.set_profiling(False)
    med = {k: statistics.median(v) for k, v in ms.items()}
    rate = {k: work[k][0] / med[k] * 1e3 for k in work}   # samples (gates) per second
    res = dict(tool="lut_bench", params="SK-128", device=args.device, reps=args.reps, timing="device events, prologue .. key switch, median",
               ms={k: round(v, 3) for k, v in med.items()}, ms_min={k: round(min(v), 3) for k, v in ms.items()},
               ms_max={k: round(max(v), 3) for k, v in ms.items()}, samples_per_s={k: round(v) for k, v in rate.items()},
               lut_theta1_vs_nand_4096=round(rate["lut_4096_theta1"] / rate["nand_4096"], 4),
               lut_theta1_vs_nand_1024=round(rate["lut_1024_theta1"] / rate["nand_1024"], 4))
    print(json.dumps(res), flush=True)
    ck.close()


if __name__ == "__main__":
    main()
