#!/usr/bin/env python3
"""An encrypted dense layer against the host-side way of doing it, in one process on one device (SK-128).

The shape is one 784 -> 128 layer on 32 samples: 4 096 programmable bootstraps, the benchmark's own batch.  Three workloads alternate for --reps
rounds after a warm-up, and the median of every figure is kept:

  fused    thfhe_linear_lut_bootstrap: inputs up, lwe_linear_kernel, PBS of the 4 096 sums, records down.  Device events give the input upload,
           the linear kernel, the PBS stages (thfhe_last_timings) and upload start .. key-switch end (thfhe_linear_last_timings); the wall clock
           gives the whole call.
  linear   thfhe_lwe_linear alone (wall clock; its kernel by device events).
  host     what a tree without these calls can do: W x in numpy on the host (int64 matmul, low 32 bits kept; wall clock), then
           thfhe_lut_bootstrap of the 4 096 records (device events for its stages, wall clock for the call).

--host-only runs the third workload alone and touches nothing this tool's tree added, so it runs on an older tree too: --root names the tree
whose thfhe package and library are loaded.  --parent-json adds such a run's document under "parent_commit".  Writes one JSON document to --out
and prints it.

usage: python tools/linear_bench.py [--reps 5] [--device 0] [--out profiles/linear_bench.json] [--host-only] [--root TREE] [--parent-json FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M, K, S = 128, 784, 32


def host_linear(W, x):
    """W x word-wise mod 2^32 on the host: int64 products and sums wrap mod 2^64, their low 32 bits are the answer"""
    W64 = W.astype(np.int64)
    return np.stack([(W64 @ x[s].astype(np.int64)).astype(np.int32) for s in range(x.shape[0])])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "linear_bench.json"))
    ap.add_argument("--host-only", action="store_true")
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--parent-json")
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(os.path.abspath(args.root), "torus-fhe_amd"))
    import thfhe
    from thfhe import keygen, lut

    p = thfhe.make_params("SK-128")
    keys = keygen.SecretKeySet(p, seed=0x5EED0001)
    ck = thfhe.CloudKey(p, keys.bk, keys.ksk, device=args.device)
    rng = np.random.default_rng(0)
    x = rng.integers(-2**31, 2**31, (S, K, p.n + 1), dtype=np.int64).astype(np.int32)   # the timing does not depend on the words
    W = rng.integers(-1, 2, (M, K)).astype(np.int32)
    tv = lut.test_vector(lut.int_outputs(lambda m: (m + 1) % 4, 4), 4)[None]
    times = {}

    def note(name, v):
        times.setdefault(name, []).append(v)

    def run_fused(keep):
        t0 = time.perf_counter()
        out = ck.linear_lut_bootstrap(tv, W, x)
        wall = (time.perf_counter() - t0) * 1e3
        if keep:
            lt, pt = ck.linear_last_timings(), ck.last_timings()
            note("fused_wall_ms", wall)
            note("fused_upload_ms", lt["upload_ms"])
            note("fused_linear_kernel_ms", lt["linear_ms"])
            note("fused_device_ms", lt["total_ms"])
            note("fused_pbs_ms", pt["total_ms"])
            note("fused_keyswitch_ms", pt["keyswitch_ms"])
        return out

    def run_linear(keep):
        t0 = time.perf_counter()
        out = ck.lwe_linear(W, x)
        wall = (time.perf_counter() - t0) * 1e3
        if keep:
            note("linear_wall_ms", wall)
            note("linear_kernel_ms", ck.linear_last_timings()["linear_ms"])
        return out

    def run_host(keep):
        t0 = time.perf_counter()
        xs = host_linear(W, x)
        t1 = time.perf_counter()
        out = ck.lut_bootstrap(tv, xs.reshape(-1, p.n + 1))
        t2 = time.perf_counter()
        if keep:
            note("host_numpy_ms", (t1 - t0) * 1e3)
            note("host_lut_bootstrap_wall_ms", (t2 - t1) * 1e3)
            note("host_wall_ms", (t2 - t0) * 1e3)
            note("host_pbs_ms", ck.last_timings()["total_ms"])
        return out

    work = [run_host] if args.host_only else [run_fused, run_linear, run_host]
    ck.set_profiling(True)
    outs = [run(False) for run in work]     # warm-up: code objects loaded, workspace and staging grown
    if not args.host_only:                  # the three ways agree before anything is timed
        assert np.array_equal(outs[0].reshape(outs[2].shape), outs[2]) and np.array_equal(outs[1], host_linear(W, x))
    for _ in range(args.reps):              # alternate the workloads: drift of the machine hits all of them alike
        for run in work:
            run(True)
    ck.set_profiling(False)
    ck.close()
    med = {k: round(statistics.median(v), 3) for k, v in times.items()}
    res = dict(tool="linear_bench", params="SK-128", layer=f"{K} -> {M}", samples=S, rotations=S * M, device=args.device, reps=args.reps,
               host_only=args.host_only, timing="device events (upload, kernels, PBS stages) and wall clock (whole calls, numpy); medians of alternating rounds",
               ms=med, ms_min={k: round(min(v), 3) for k, v in times.items()}, ms_max={k: round(max(v), 3) for k, v in times.items()})
    if not args.host_only:
        res["linear_share_of_fused_device"] = round(med["fused_linear_kernel_ms"] / med["fused_device_ms"], 4)
        res["keyswitch_share_of_fused_device"] = round(med["fused_keyswitch_ms"] / med["fused_device_ms"], 4)
        res["fused_vs_host_wall"] = round(med["host_wall_ms"] / med["fused_wall_ms"], 3)
    if args.parent_json:
        with open(args.parent_json) as f:
            res["parent_commit"] = json.load(f)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
