#!/usr/bin/env python3
"""Leveled scatter timing in one process on one device (SK-128).

For 1024 and 4096 samples and (d_tree, d_rot) = (0, 10), (6, 0), (6, 4) it times
  scatter_T_R_B   thfhe_lhe_scatter of one trivial value: d_rot + 2^d_tree - 1 external products per sample, then the sum into one table
  lookup_T_R_B    thfhe_lhe_lookup_wo_keyswitch on a public table at the same shape on the same set: the same number of products
The TGSW samples are noiseless (zero mask): timing does not depend on the words.  Device events of a call that is not cut into slices (scatter:
rotations .. sum; lookup: tree .. rotations) and wall time of the host-buffer call.  Each workload is warmed up, then the workloads alternate for
--reps rounds; medians are kept.  Every product streams its own 2l x 32 KiB of spectra once: the tool reports products/s, the ratio to the lookup's,
and the achieved bytes/s of spectra against the measured HBM copy rate of the device guide, 6.29 TB/s.  The expectation is parity with the lookup:
a demux node stores two TLWE samples where a CMux loads two.  Prints one JSON line and writes it to profiles/scatter_bench.json.

usage: python tools/scatter_bench.py [--reps 5] [--device 0] [--counts 1024,4096] [--out profiles/scatter_bench.json]
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

HBM_BYTES_PER_S = 6.29e12   # measured float4 copy rate of one MI355X (8.0 TB/s spec)
SHAPES = [(0, 10), (6, 0), (6, 4)]


def trivial_tgsw(p, bits):
    C = np.zeros((len(bits), 2 * p.l, 2, p.N), np.int32)
    for j in range(2):
        for lv in range(p.l):
            C[:, j * p.l + lv, j, 0] = (np.asarray(bits, np.int64) << (32 - (lv + 1) * p.Bgbit)).astype(np.uint32).view(np.int32)
    return C


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--counts", default="1024,4096")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scatter_bench.json"))
    args = ap.parse_args()
    counts = [int(c) for c in args.counts.split(",")]
    p = thfhe.make_params("SK-128")
    K = keygen.SecretKeySet(p, seed=0x5EED0001)
    ck = thfhe.CloudKey(p, K.bk, K.ksk, device=args.device)
    rng = np.random.default_rng(0)
    one = lut.lhe_value([1], encode=lambda v: lut.encode(v, 8))
    work, sets, products = {}, [], {}
    for d_tree, d_rot in SHAPES:
        d = d_tree + d_rot
        tab = lut.lhe_table(rng.integers(0, 8, 1 << d), d_tree, d_rot, encode=lambda v: lut.encode(v, 8))
        ts = ck.tgsw_set(trivial_tgsw(p, lut.lhe_address_bits(rng.integers(0, 1 << d, max(counts)), d)), d)
        sets.append(ts)
        for B in counts:
            tag = f"{d_tree}_{d_rot}_{B}"
            work["scatter_" + tag] = lambda ts=ts, d_tree=d_tree, d_rot=d_rot, B=B: ck.lhe_scatter(ts, one, d_tree=d_tree, d_rot=d_rot, count=B)
            work["lookup_" + tag] = lambda ts=ts, tab=tab, d_tree=d_tree, d_rot=d_rot, B=B: ck.lhe_lookup_wo_keyswitch(ts, tab, d_tree=d_tree, d_rot=d_rot, count=B)
            products[tag] = B * ((1 << d_tree) - 1 + d_rot)
    ck.set_tree_slice(1 << 20)   # no call below is cut into slices: the events cover the whole call
    ck.set_profiling(True)
    for run in work.values():
        run()
    wall, ev, sums = {k: [] for k in work}, {k: [] for k in work}, {k: [] for k in work}
    for _ in range(args.reps):
        for k, run in work.items():
            t0 = time.perf_counter()
            run()
            wall[k].append((time.perf_counter() - t0) * 1e3)
            t = ck.last_timings()
            # scatter: rotations | tree | sum.  lookup: tree | rotations | (no key switch); its last interval is empty
            ev[k].append(t["prologue_ms"] + t["blind_rotate_ms"])
            sums[k].append(t["keyswitch_ms"])
    ck.set_profiling(False)
    med = lambda d: {k: round(statistics.median(v), 3) for k, v in d.items()}
    spread = lambda d: {k: [round(min(v), 3), round(max(v), 3)] for k, v in d.items()}
    e = med(ev)
    per_product = 2 * p.l * 32768
    rate = {k: products[k.split("_", 1)[1]] / (e[k] * 1e-3) for k in work}
    res = dict(tool="scatter_bench", params="SK-128", device=args.device, reps=args.reps, lib=os.path.abspath(thfhe.LIB_PATH),
               timing="median of alternating rounds; wall = host-buffer call, product_ms = device events over the external products "
                      "(scatter: rotations + demux tree; lookup: CMux tree + rotations), sum_ms = the scatter's reduction kernel",
               wall_ms=med(wall), wall_ms_min_max=spread(wall), product_ms=e, product_ms_min_max=spread(ev),
               sum_ms={k: v for k, v in med(sums).items() if k.startswith("scatter")}, products=products,
               products_per_s={k: round(v, 0) for k, v in rate.items()},
               scatter_over_lookup_products_per_s={t: round(rate["scatter_" + t] / rate["lookup_" + t], 4) for t in products},
               spectra_bytes_per_product=per_product, spectra_bytes_per_s={k: round(v * per_product, 0) for k, v in rate.items()},
               hbm_bytes_per_s=HBM_BYTES_PER_S, fraction_of_hbm={k: round(v * per_product / HBM_BYTES_PER_S, 4) for k, v in rate.items()})
    line = json.dumps(res)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    for ts in sets:
        ts.close()
    ck.close()


if __name__ == "__main__":
    main()
