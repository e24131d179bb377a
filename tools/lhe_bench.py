#!/usr/bin/env python3
"""Leveled table lookup timing in one process on one device (SK-128).

For 1024 and 4096 samples it times
  lhe_0_10   thfhe_lhe_lookup at (d_tree, d_rot) = (0, 10): ten CMuxes per sample on one public polynomial
  lhe_6_10   thfhe_lhe_lookup at (6, 10): 63 + 10 CMuxes per sample on a public 16-bit table
  lut        thfhe_lut_bootstrap at theta = 1 on the same count: one blind rotation (n CMuxes) and one key switch per sample
The TGSW samples are noiseless (zero mask): timing does not depend on the words, and 4 096 x 16 real samples would take minutes to encrypt.
Device events (tree .. key switch of a call that is not cut into slices) and wall time of the host-buffer call.  Each workload is warmed up,
then the workloads alternate for --reps rounds; medians are kept.  Every CMux streams its own 2l x 32 KiB of spectra once: the tool reports the
achieved bytes/s of spectra (events of tree + rotations) against the measured HBM copy rate of the device guide, 6.29 TB/s.  Prints one JSON line.

usage: python tools/lhe_bench.py [--reps 5] [--device 0] [--counts 1024,4096]
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
SHAPES = [(0, 10), (6, 10)]


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
    args = ap.parse_args()
    counts = [int(c) for c in args.counts.split(",")]
    p = thfhe.make_params("SK-128")
    K = keygen.SecretKeySet(p, seed=0x5EED0001)
    ck = thfhe.CloudKey(p, K.bk, K.ksk, device=args.device)
    rng = np.random.default_rng(0)
    x = K.encrypt(rng.integers(0, 2, max(counts)), 1)   # timing only: any records do
    tv = lut.test_vector(lut.int_outputs(lambda m: m & 1, 2, 16), 16)
    work, sets, cmuxes = {}, [], {}
    for d_tree, d_rot in SHAPES:
        d = d_tree + d_rot
        tab = lut.lhe_table(rng.integers(0, 8, 1 << d), d_tree, d_rot, encode=lambda v: lut.encode(v, 8))
        ts = ck.tgsw_set(trivial_tgsw(p, lut.lhe_address_bits(rng.integers(0, 1 << d, max(counts)), d)), d)
        sets.append(ts)
        for B in counts:
            work[f"lhe_{d_tree}_{d_rot}_{B}"] = lambda ts=ts, tab=tab, d_tree=d_tree, d_rot=d_rot, B=B: ck.lhe_lookup(ts, tab, d_tree=d_tree, d_rot=d_rot, count=B)
            cmuxes[f"lhe_{d_tree}_{d_rot}_{B}"] = B * ((1 << d_tree) - 1 + d_rot)
    for B in counts:
        work[f"lut_{B}"] = lambda a=x[:B]: ck.lut_bootstrap(tv, a)
    ck.set_tree_slice(1 << 20)   # no call below is cut into slices: the events cover the whole call
    ck.set_profiling(True)
    for run in work.values():
        run()
    wall, ev, dev = {k: [] for k in work}, {k: [] for k in work}, {k: [] for k in work}
    for _ in range(args.reps):
        for k, run in work.items():
            t0 = time.perf_counter()
            run()
            wall[k].append((time.perf_counter() - t0) * 1e3)
            t = ck.last_timings()
            ev[k].append(t["total_ms"])
            dev[k].append(t["total_ms"] - t["keyswitch_ms"])   # lhe: tree + rotations
    ck.set_profiling(False)
    med = lambda d: {k: round(statistics.median(v), 3) for k, v in d.items()}
    spread = lambda d: {k: [round(min(v), 3), round(max(v), 3)] for k, v in d.items()}
    e, c = med(ev), med(dev)
    per_cmux = 2 * p.l * 32768
    rate = {k: cmuxes[k] * per_cmux / (c[k] * 1e-3) for k in cmuxes}
    res = dict(tool="lhe_bench", params="SK-128", device=args.device, reps=args.reps, lib=os.path.abspath(thfhe.LIB_PATH),
               timing="median of alternating rounds; wall = host-buffer call, events = tree .. key switch on the device",
               wall_ms=med(wall), wall_ms_min_max=spread(wall), event_ms=e, event_ms_min_max=spread(ev), cmux_ms=c, cmuxes=cmuxes,
               spectra_bytes_per_cmux=per_cmux, spectra_bytes_per_s={k: round(v, 0) for k, v in rate.items()},
               hbm_bytes_per_s=HBM_BYTES_PER_S, fraction_of_hbm={k: round(v / HBM_BYTES_PER_S, 4) for k, v in rate.items()},
               lhe_over_lut={f"{dt}_{dr}_{B}": round(e[f"lhe_{dt}_{dr}_{B}"] / e[f"lut_{B}"], 4) for dt, dr in SHAPES for B in counts})
    print(json.dumps(res), flush=True)
    for ts in sets:
        ts.close()
    ck.close()


if __name__ == "__main__":
    main()
