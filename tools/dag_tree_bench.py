#!/usr/bin/env python3
"""Tree nodes in the gate-DAG executor, timing in one process on one device (SK-128).

  (a) level   one level of 4 096 TREE nodes (p = 4, theta1 = 2; 4 096 instances of a one-node circuit) through thfhe_dag_run_tree_batch against
              thfhe_tree_lut_bootstrap on the same samples (wall time of the host-buffer calls).  --flat-only times the flat call alone: run it
              with THFHE_HIP_LIB pointing at the parent commit's library for that build's number (it lacks the DAG entry).
  (b) embed   tree_mul_digits between two gate levels (NAND, NAND -> two TREE nodes -> NAND), Q = 256 and 2 048 instances: one
              thfhe_dag_run_tree_batch call against the same three levels as host-buffer calls (thfhe_gates, thfhe_tree_lut_bootstrap, thfhe_gates)
              with the download and upload between them.  Timing only: any records do; the two forms are checked to give the same words.
Each workload is warmed up, then the workloads alternate for --reps rounds; medians are kept.  Prints one JSON line.

usage: python tools/dag_tree_bench.py [--reps 5] [--device 0] [--flat-only]
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
from thfhe import threshold as T  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--flat-only", action="store_true", help="only thfhe_tree_lut_bootstrap of (a) (a library without thfhe_dag_run_tree_batch)")
    args = ap.parse_args()
    if args.flat_only:
        thfhe.SIGNATURES.pop("thfhe_dag_run_tree_batch", None)
    p = thfhe.make_params("SK-128")
    K = keygen.SecretKeySet(p, seed=0x5EED0001)
    ck = thfhe.CloudKey(p, K.bk, K.ksk, device=args.device)
    rng = np.random.default_rng(0)
    pc = T.PolyContext(args.device)
    pc.set_pack_key(keygen.gen_pack_key(rng, K.lwe_key, K.rlwe_key, p.ks_t, p.ks_basebit, thfhe.SIGMAS["SK-128"]["bk"]), p.ks_t, p.ks_basebit)
    B = 4096
    xl, xh = K.encrypt(rng.integers(0, 2, B), 1), K.encrypt(rng.integers(0, 2, B), 2)   # timing only: any records do
    rows = lut.tree_test_vectors(lambda h, l: (h * l + 1) % 4, 4, 4, 4, theta=2)
    work = {"flat_4096": lambda: ck.tree_lut_bootstrap(pc, rows, xl, xh, p_hi=4, theta=2)}
    check = {}
    if not args.flat_only:
        one = Cc.Circuit()
        a, b = one.inputs(2)
        t = one.tree(one.tree_rows(rows), [a], [b], 4, theta1=2)
        x1 = np.ascontiguousarray(np.stack([xl, xh], axis=1))
        work["dag_level_4096"] = lambda: Cc.evaluate_batch(ck, one, x1, [t], pack=pc)
        check["level"] = lambda: np.array_equal(work["dag_level_4096"]()[:, 0], work["flat_4096"]())
        cir = Cc.Circuit()
        g = cir.inputs(4)
        ga, gb = cir.gate(thfhe.NAND, g[0], g[1]), cir.gate(thfhe.NAND, g[2], g[3])
        lo, hi = Cc.tree_mul_digits(cir, ga, gb)
        out = cir.gate(thfhe.NAND, lo, hi)
        tv1 = np.stack(cir.tv1).reshape(2, 4, 1024)
        for Q in (256, 2048):
            x = np.ascontiguousarray(np.stack([K.encrypt(rng.integers(0, 2, Q), 10 + i) for i in range(4)], axis=1))

            def levels(x=x, Q=Q):
                l1 = ck.gates(thfhe.NAND, np.concatenate([x[:, 0], x[:, 2]]), np.concatenate([x[:, 1], x[:, 3]]))
                l2 = ck.tree_lut_bootstrap(pc, tv1, np.tile(l1[:Q], (2, 1)), np.tile(l1[Q:], (2, 1)), p_hi=8, theta=2, table_index=np.repeat([0, 1], Q))
                return ck.gates(thfhe.NAND, l2[:Q], l2[Q:])
            work[f"embed_dag_{Q}"] = lambda x=x: Cc.evaluate_batch(ck, cir, x, [out], pack=pc)
            work[f"embed_levels_{Q}"] = levels
            check[f"embed_{Q}"] = lambda Q=Q: np.array_equal(work[f"embed_dag_{Q}"]()[:, 0], work[f"embed_levels_{Q}"]())
    same = {k: bool(f()) for k, f in check.items()}   # also the warm-up of the DAG forms
    for run in work.values():
        run()
    wall = {k: [] for k in work}
    for _ in range(args.reps):
        for k, run in work.items():
            t0 = time.perf_counter()
            run()
            wall[k].append((time.perf_counter() - t0) * 1e3)
    med = {k: round(statistics.median(v), 3) for k, v in wall.items()}
    res = dict(tool="dag_tree_bench", params="SK-128", device=args.device, reps=args.reps, lib=os.path.basename(thfhe.LIB_PATH), flat_only=args.flat_only,
               timing="median of alternating rounds; wall time of the host-buffer calls", wall_ms=med,
               wall_ms_min_max={k: [round(min(v), 3), round(max(v), 3)] for k, v in wall.items()}, same_words=same)
    if not args.flat_only:
        res["dag_level_rate_vs_flat"] = round(med["flat_4096"] / med["dag_level_4096"], 4)
        res["levels_vs_dag"] = {str(Q): round(med[f"embed_levels_{Q}"] / med[f"embed_dag_{Q}"], 4) for Q in (256, 2048)}
    print(json.dumps(res), flush=True)
    ck.close()
    pc.close()


if __name__ == "__main__":
    main()
