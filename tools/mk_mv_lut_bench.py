#!/usr/bin/env python3
"""Multi-key multi-value bootstrapping against the many-LUT programmable bootstrap, in one process on one device (3-gen sets).

Times thfhe_mk_mv_lut_bootstrap at q = 4, 16 and 64 (p = 8 taps, bit tables through thfhe.lut.mv_bool_factors) and thfhe_mk_lut_bootstrap at
theta = 1 and 4 on the same samples: MK2 and MK4 at 1024 samples, MK16 at 256.  Every call is one slice (thfhe_mk_set_mv_slice = samples x q) and
is timed by the context's device events (thfhe_mk_last_timings: prologue + accumulator start | rotation + extraction | key switch); the host-buffer
call synchronises its stream before the events are read.  Each shape is warmed up first, then the workloads of a set alternate for --reps rounds;
the median is kept.  The expectation to hold a multi-value call against is one rotation, plus q key switches, plus the epilogue: the report gives
the key switch's slot, and the epilogue as the rotation slot minus that of the theta = 1 call (whose slot holds the rotation and ONE extraction).
Prints one JSON line and writes it to profiles/mk_mv_lut_bench.json.

usage: python tools/mk_mv_lut_bench.py [--reps 5] [--device 0] [--sets MK2 MK4 MK16]
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

SETS = {"MK2": 1024, "MK4": 1024, "MK16": 256}
QS = (4, 16, 64)
P = 8


def bench_set(name, B, reps, device):
    p = thfhe.make_params(name)
    K = keygen.MKSecretKeySet(p, seed=1, sigma_lwe=2.0**-13.26, device=device)
    ck = thfhe.MKCloudKey(p, K.bk, K.ksk, device=device)
    rng = np.random.default_rng(0)
    x = K.encrypt(rng.integers(0, 2, B), 1)
    work = {}
    for t in (1, 4):
        tv = lut.test_vector([lut.int_outputs(lambda m, j=j: (m + j) % 4, 4, torus_bits=64) for j in range(t)], 4, t, p.N, torus_bits=64)
        work[f"lut_theta{t}"] = lambda tv=tv, t=t: ck.lut_bootstrap(tv, x, theta=t)
    for q in QS:
        tv0, c, ob = lut.mv_bool_factors(rng.integers(0, 2, (q, P)), P, 64, p.N)
        work[f"mv_q{q}"] = lambda tv0=tv0, c=c, ob=ob: ck.mv_lut_bootstrap(c, x, tv0=tv0, out_bias=ob)
    ck.set_mv_slice(B * max(QS))
    ck.set_profiling(True)
    for run in work.values():   # warm-up: code objects loaded, workspace and staging grown for every shape
        run()
    slots = {k: [] for k in work}
    for _ in range(reps):       # alternate the workloads: drift of the machine hits all of them alike
        for k, run in work.items():
            run()
            slots[k].append(ck.last_timings())
    ck.set_profiling(False)
    ck.close()
    med = {k: {s: statistics.median(t[s] for t in v) for s in v[0]} for k, v in slots.items()}
    out = {}
    for k, m in med.items():
        outs = int(k.split("q")[1]) if k.startswith("mv_") else int(k[-1])
        out[k] = dict(total_ms=round(m["total_ms"], 3), rotation_slot_ms=round(m["blind_rotate_ms"], 3), keyswitch_ms=round(m["keyswitch_ms"], 3),
                      total_ms_min=round(min(t["total_ms"] for t in slots[k]), 3), total_ms_max=round(max(t["total_ms"] for t in slots[k]), 3),
                      outputs_per_s=round(B * outs / m["total_ms"] * 1e3))
        if k.startswith("mv_"):
            out[k].update(epilogue_ms=round(m["blind_rotate_ms"] - med["lut_theta1"]["blind_rotate_ms"], 3),
                          keyswitch_share=round(m["keyswitch_ms"] / m["total_ms"], 3), vs_lut_theta1=round(m["total_ms"] / med["lut_theta1"]["total_ms"], 3))
    return dict(samples=B, p=P, calls=out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--sets", nargs="*", default=list(SETS))
    args = ap.parse_args()
    res = dict(tool="mk_mv_lut_bench", device=args.device, reps=args.reps, timing="device events, prologue .. key switch, median of alternating rounds",
               sets={name: bench_set(name, SETS[name], args.reps, args.device) for name in args.sets})
    line = json.dumps(res)
    print(line, flush=True)
    with open(os.path.join(ROOT, "profiles", "mk_mv_lut_bench.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
