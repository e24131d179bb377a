#!/usr/bin/env python3
"""Multi-value bootstrap timing in one process on one device (SK-128).

For 1024 and 4096 samples it times
  tree_mv   thfhe_tree_lut_bootstrap_mv at p = 4, 8, 16: 1 + 1 rotations per sample
  tree      thfhe_tree_lut_bootstrap on the same inputs at (p = 4, theta1 = 2), (p = 8, theta1 = 2), (p = 16, theta1 = 1): R + 1 rotations
  mv_qQ     thfhe_mv_lut_bootstrap at p = 16 and q = 4, 16, 64 outputs
  lut       thfhe_lut_bootstrap at theta = 1 on the same count: one rotation and one key switch per sample, so mv_qQ - lut is the epilogue
            plus the q - 1 further key switches
Device events (prologue .. last key switch; the tree entries: the whole call) and wall time of the host-buffer call.  Each workload is warmed up,
then the workloads alternate for --reps rounds; medians are kept.  Prints one JSON line.  --tree-only keeps the `tree` and `lut` legs: with
THFHE_HIP_LIB pointing at a library that lacks the multi-value entries (the parent commit's) it gives that build's figures.

usage: python tools/mv_lut_bench.py [--reps 5] [--device 0] [--counts 1024,4096] [--tree-only]
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
from thfhe import keygen, lut  # noqa: E402
from thfhe import threshold as T  # noqa: E402

SHAPES = [(4, 2), (8, 2), (16, 1)]   # (p, theta1 of the tree it is compared with)
MV_NAMES = ("thfhe_mv_lut_bootstrap", "thfhe_mv_lut_bootstrap_wo_keyswitch", "thfhe_tree_lut_bootstrap_mv")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--counts", default="1024,4096")
    ap.add_argument("--tree-only", action="store_true", help="only the thfhe_tree_lut_bootstrap and thfhe_lut_bootstrap legs (a library without the multi-value entries)")
    args = ap.parse_args()
    if args.tree_only:
        for name in MV_NAMES:
            thfhe.SIGNATURES.pop(name, None)   # not bound: the library may lack them
    counts = [int(c) for c in args.counts.split(",")]
    p = thfhe.make_params("SK-128")
    K = keygen.SecretKeySet(p, seed=0x5EED0001)
    ck = thfhe.CloudKey(p, K.bk, K.ksk, device=args.device)
    rng = np.random.default_rng(0)
    pc = T.PolyContext(args.device)
    pc.set_pack_key(keygen.gen_pack_key(rng, K.lwe_key, K.rlwe_key, p.ks_t, p.ks_basebit, thfhe.SIGMAS["SK-128"]["bk"]), p.ks_t, p.ks_basebit)
    xl, xh = K.encrypt(rng.integers(0, 2, max(counts)), 1), K.encrypt(rng.integers(0, 2, max(counts)), 2)   # timing only: any records do
    f = lambda h, l: (h * l + 1) % 2
    work = {}
    for B in counts:
        a, b = xl[:B], xh[:B]
        work[f"lut_{B}"] = lambda a=a: ck.lut_bootstrap(lut.test_vector(lut.int_outputs(lambda m: m & 1, 2, 16), 16), a)
        for pp, th in SHAPES:
            tv1 = lut.tree_test_vectors(f, pp, pp, 2, theta=th)
            work[f"tree_p{pp}_{B}"] = lambda a=a, b=b, pp=pp, th=th, tv1=tv1: ck.tree_lut_bootstrap(pc, tv1, a, b, p_hi=pp, theta=th)
            if not args.tree_only:
                tv0, w = lut.tree_mv_factors(f, pp, pp, 2)
                work[f"tree_mv_p{pp}_{B}"] = lambda a=a, b=b, tv0=tv0, w=w: ck.tree_lut_bootstrap_mv(pc, w, a, b, tv0=tv0)
        if not args.tree_only:
            for q in (4, 16, 64):
                w = lut.mv_factors(rng.integers(0, 2, (q, 16)), 16)
                work[f"mv_q{q}_{B}"] = lambda a=a, w=w: ck.mv_lut_bootstrap(w, a, tv0=lut.mv_base(1 << 30))
    ck.set_tree_slice(1 << 20)   # no call below is cut into slices (4096 samples x 64 outputs = 262 144 records): the events cover the whole call
    ck.set_profiling(True)
    for run in work.values():
        run()
    wall, ev = {k: [] for k in work}, {k: [] for k in work}
    for _ in range(args.reps):
        for k, run in work.items():
            t0 = time.perf_counter()
            run()
            wall[k].append((time.perf_counter() - t0) * 1e3)
            ev[k].append(ck.last_timings()["total_ms"])
    ck.set_profiling(False)
    med = lambda d: {k: round(statistics.median(v), 3) for k, v in d.items()}
    spread = lambda d: {k: [round(min(v), 3), round(max(v), 3)] for k, v in d.items()}
    res = dict(tool="mv_lut_bench", params="SK-128", device=args.device, reps=args.reps, lib=os.path.abspath(thfhe.LIB_PATH), tree_only=args.tree_only,
               timing="median of alternating rounds; wall = host-buffer call, events = first prologue .. last key switch on the device",
               wall_ms=med(wall), wall_ms_min_max=spread(wall), event_ms=med(ev), event_ms_min_max=spread(ev))
    if not args.tree_only:
        e = res["event_ms"]
        res["tree_over_tree_mv"] = {f"p{pp}_{B}": round(e[f"tree_p{pp}_{B}"] / e[f"tree_mv_p{pp}_{B}"], 4) for pp, _ in SHAPES for B in counts}
        res["rotation_count_ratio"] = {f"p{pp}": (pp // th + 1) / 2 for pp, th in SHAPES}
        res["mv_over_lut"] = {f"q{q}_{B}": round(e[f"mv_q{q}_{B}"] / e[f"lut_{B}"], 4) for q in (4, 16, 64) for B in counts}
    print(json.dumps(res), flush=True)
    ck.close()
    pc.close()


if __name__ == "__main__":
    main()
