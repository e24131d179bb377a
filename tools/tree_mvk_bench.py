#!/usr/bin/env python3
"""k-output multi-value tree timing in one process on one device (SK-128).

For 1024 and 4096 samples at (p_hi, p_lo, k) = (8, 8, 4) and (4, 4, 2) it times three ways to the same k outputs per sample
  mvk      thfhe_tree_lut_bootstrap_mvk: 1 + k rotations per sample, one call
  k_mv     k calls of thfhe_tree_lut_bootstrap_mv, one per table: k (1 + 1) rotations
  calls3   thfhe_mv_lut_bootstrap (q = k p_hi) -> thfhe_pack_boxes -> thfhe_lut_bootstrap_enc: 1 + k rotations, every candidate and packed table
           crossing the host twice
Wall time of the host-buffer calls (each ends in a stream synchronise) and, for the single-call leg, the device events of the whole call.  Each
workload is warmed up, then the workloads alternate for --reps rounds; medians are kept.  Prints one JSON line.  --parent keeps the k_mv and calls3
legs: with THFHE_HIP_LIB pointing at a library that lacks the fused entry (the parent commit's) it gives that build's figures.

usage: python tools/tree_mvk_bench.py [--reps 5] [--device 0] [--counts 1024,4096] [--parent]
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

SHAPES = [(8, 8, 4), (4, 4, 2)]   # (p_hi, p_lo, k)
NEW_NAMES = ("thfhe_tree_lut_bootstrap_mvk", "thfhe_dag_run_mv_batch")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--counts", default="1024,4096")
    ap.add_argument("--parent", action="store_true", help="only the k_mv and calls3 legs (a library without thfhe_tree_lut_bootstrap_mvk)")
    args = ap.parse_args()
    if args.parent:
        for name in NEW_NAMES:
            thfhe.SIGNATURES.pop(name, None)   # not bound: the library may lack them
    counts = [int(c) for c in args.counts.split(",")]
    p = thfhe.make_params("SK-128")
    K = keygen.SecretKeySet(p, seed=0x5EED0001)
    ck = thfhe.CloudKey(p, K.bk, K.ksk, device=args.device)
    rng = np.random.default_rng(0)
    pc = T.PolyContext(args.device)
    pc.set_pack_key(keygen.gen_pack_key(rng, K.lwe_key, K.rlwe_key, p.ks_t, p.ks_basebit, thfhe.SIGMAS["SK-128"]["bk"]), p.ks_t, p.ks_basebit)
    xl, xh = K.encrypt(rng.integers(0, 2, max(counts)), 1), K.encrypt(rng.integers(0, 2, max(counts)), 2)   # timing only: any records do
    work, single = {}, set()
    for B in counts:
        a, b = xl[:B], xh[:B]
        for p_hi, p_lo, k in SHAPES:
            fs = [lambda h, l, j=j: ((h * l + j) >> (j & 1)) & 1 for j in range(k)]
            tv0, w = lut.tree_mv_factors(fs[0], p_hi, p_lo, 2)[0], np.stack([lut.tree_mv_factors(f, p_hi, p_lo, 2)[1] for f in fs])
            tag = f"p{p_hi}x{p_lo}_k{k}_{B}"

            def k_mv(a=a, b=b, tv0=tv0, w=w):
                return [ck.tree_lut_bootstrap_mv(pc, w[j], a, b, tv0=tv0) for j in range(w.shape[0])]

            def calls3(a=a, b=b, tv0=tv0, w=w):
                k, p_hi, p_lo = w.shape
                cands = ck.mv_lut_bootstrap(w.reshape(k * p_hi, p_lo), a, tv0=tv0)
                ta, tb = T.PackBoxes(pc, cands.reshape(-1, cands.shape[-1]), p_hi)
                return ck.lut_bootstrap_enc(ta, tb, np.repeat(b, k, axis=0), lut_index=np.arange(len(ta)))

            work[f"k_mv_{tag}"], work[f"calls3_{tag}"] = k_mv, calls3
            if not args.parent:
                work[f"mvk_{tag}"] = lambda a=a, b=b, tv0=tv0, w=w: ck.tree_lut_bootstrap_mvk(pc, w, a, b, tv0=tv0)
                single.add(f"mvk_{tag}")
    ck.set_tree_slice(1 << 20)   # no call below is cut into slices (4096 samples x 32 candidates = 131 072): the events cover the whole call
    ck.set_profiling(True)
    for run in work.values():
        run()
    wall, ev = {k: [] for k in work}, {k: [] for k in single}
    for _ in range(args.reps):
        for k, run in work.items():
            t0 = time.perf_counter()
            run()
            wall[k].append((time.perf_counter() - t0) * 1e3)
            if k in single:
                ev[k].append(ck.last_timings()["total_ms"])
    ck.set_profiling(False)
    med = lambda d: {k: round(statistics.median(v), 3) for k, v in d.items()}
    spread = lambda d: {k: [round(min(v), 3), round(max(v), 3)] for k, v in d.items()}
    res = dict(tool="tree_mvk_bench", params="SK-128", device=args.device, reps=args.reps, lib=os.path.abspath(thfhe.LIB_PATH), parent=args.parent,
               timing="median of alternating rounds; wall = the leg's host-buffer calls, each ending in a stream synchronise; events = the fused call on the device",
               wall_ms=med(wall), wall_ms_min_max=spread(wall), event_ms=med(ev), event_ms_min_max=spread(ev))
    if not args.parent:
        wl = res["wall_ms"]
        tags = [f"p{p_hi}x{p_lo}_k{k}_{B}" for B in counts for p_hi, p_lo, k in SHAPES]
        res["k_mv_over_mvk"] = {t: round(wl[f"k_mv_{t}"] / wl[f"mvk_{t}"], 4) for t in tags}
        res["calls3_over_mvk"] = {t: round(wl[f"calls3_{t}"] / wl[f"mvk_{t}"], 4) for t in tags}
        res["rotation_count_ratio"] = {f"k{k}": dict(k_mv=2 * k / (1 + k), calls3=1.0) for _, _, k in SHAPES}
    print(json.dumps(res), flush=True)
    ck.close()
    pc.close()


if __name__ == "__main__":
    main()
