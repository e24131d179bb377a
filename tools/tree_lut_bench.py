#!/usr/bin/env python3
"""Two-digit tree PBS timing in one process on one device (SK-128).

For 1024 and 4096 samples at (p = 4, theta1 = 2) and (p = 8, theta1 = 2) it times
  tree      thfhe_tree_lut_bootstrap, the fused call (wall time of the host-buffer call, and the device events ms[3] of thfhe_last_timings)
  compose   the same result as three host-buffer calls: thfhe_lut_bootstrap on replicated inputs -> thfhe_pack_boxes -> thfhe_lut_bootstrap_enc
  lut       thfhe_lut_bootstrap at theta1 on count * (R + 1) samples: the same number of rotations without the second key switch, the packing
            and the box kernel (device events).  Run the tool with THFHE_HIP_LIB pointing at another build for that build's number.
Each workload is warmed up, then the workloads alternate for --reps rounds; medians are kept.  Prints one JSON line.

usage: python tools/tree_lut_bench.py [--reps 5] [--device 0] [--lut-only]
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

N = 1024


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--lut-only", action="store_true", help="only the thfhe_lut_bootstrap legs (a library without the tree entry points)")
    args = ap.parse_args()
    p = thfhe.make_params("SK-128")
    K = keygen.SecretKeySet(p, seed=0x5EED0001)
    ck = thfhe.CloudKey(p, K.bk, K.ksk, device=args.device)
    rng = np.random.default_rng(0)
    shapes = [(4, 2), (8, 2)]
    counts = [1024, 4096]
    enc = {pp: (K.encrypt(rng.integers(0, 2, 4096), 1), K.encrypt(rng.integers(0, 2, 4096), 2)) for pp, _ in shapes}   # timing only: any records do
    tv1 = {pp: lut.tree_test_vectors(lambda h, l: (h * l + 1) % pp, pp, pp, pp, theta=th) for pp, th in shapes}
    work = {}
    for pp, th in shapes:
        R = pp // th
        for B in counts:
            xl, xh = enc[pp][0][:B], enc[pp][1][:B]
            big = np.tile(xl, (R + 1, 1))
            work[f"lut_p{pp}_{B}"] = ("ev", lambda big=big, pp=pp, th=th: ck.lut_bootstrap(tv1[pp][0], big, theta=th))
    if not args.lut_only:
        from thfhe import threshold as T
        pc = T.PolyContext(args.device)
        pc.set_pack_key(keygen.gen_pack_key(rng, K.lwe_key, K.rlwe_key, p.ks_t, p.ks_basebit, thfhe.SIGMAS["SK-128"]["bk"]), p.ks_t, p.ks_basebit)

        def compose(pp, th, xl, xh):
            R, B = pp // th, xl.shape[0]
            c1 = ck.lut_bootstrap(tv1[pp], np.repeat(xl, R, axis=0), theta=th, lut_index=np.tile(np.arange(R), B))
            a, b = T.PackBoxes(pc, c1.reshape(B * pp, -1), pp)
            return ck.lut_bootstrap_enc(a, b, xh, lut_index=np.arange(B))

        for pp, th in shapes:
            for B in counts:
                xl, xh = enc[pp][0][:B], enc[pp][1][:B]
                work[f"tree_p{pp}_{B}"] = ("both", lambda pp=pp, th=th, xl=xl, xh=xh: ck.tree_lut_bootstrap(pc, tv1[pp], xl, xh, p_hi=pp, theta=th))
                work[f"compose_p{pp}_{B}"] = ("wall", lambda pp=pp, th=th, xl=xl, xh=xh: compose(pp, th, xl, xh))
    ck.set_profiling(True)
    for _, run in work.values():
        run()
    wall, ev = {k: [] for k in work}, {k: [] for k in work}
    for _ in range(args.reps):
        for k, (kind, run) in work.items():
            t0 = time.perf_counter()
            run()
            wall[k].append((time.perf_counter() - t0) * 1e3)
            if kind != "wall":
                ev[k].append(ck.last_timings()["total_ms"])
    ck.set_profiling(False)
    med = lambda d: {k: round(statistics.median(v), 3) for k, v in d.items() if v}
    spread = lambda d: {k: [round(min(v), 3), round(max(v), 3)] for k, v in d.items() if v}
    res = dict(tool="tree_lut_bench", params="SK-128", device=args.device, reps=args.reps, lib=os.path.basename(thfhe.LIB_PATH),
               timing="median of alternating rounds; wall = host-buffer call, events = prologue .. last key switch on the device",
               wall_ms=med(wall), wall_ms_min_max=spread(wall), event_ms=med(ev), event_ms_min_max=spread(ev))
    if not args.lut_only:
        e, w = res["event_ms"], res["wall_ms"]
        res["tree_vs_lut_same_rotations"] = {f"p{pp}_{B}": round(e[f"tree_p{pp}_{B}"] / e[f"lut_p{pp}_{B}"], 4) for pp, _ in shapes for B in counts}
        res["compose_vs_tree_wall"] = {f"p{pp}_{B}": round(w[f"compose_p{pp}_{B}"] / w[f"tree_p{pp}_{B}"], 4) for pp, _ in shapes for B in counts}
    print(json.dumps(res), flush=True)
    ck.close()


if __name__ == "__main__":
    main()
