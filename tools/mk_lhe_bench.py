#!/usr/bin/env python3
"""Leveled lookup timing on the 64-bit ring of degree 2048, in one process on one device (CB-128's ring).

For 256 and 4096 samples it times
  lhe_0_10   thfhe_mk_lhe_lookup_wo_keyswitch at (d_tree, d_rot) = (0, 10): ten CMuxes per sample on one public polynomial
  lhe_6_10   ... at (6, 10): 63 + 10 CMuxes per sample on a public table, each CMux streaming its own 1 MiB of spectra
  rotate     thfhe_mk_rotate_partial_dev on the same context: n CMuxes per job, all jobs sharing ONE key stream -- the number to compare with
The set and key words are random or noiseless (timing does not depend on the words).  A set of 4096 x 16 bits is 64 GiB of spectra; the (0, 10) set
is closed before the (6, 10) set is made, and a set the device has no room for is reported as skipped.  Lookups: device events (tree .. extraction
of a call that is not cut into slices); rotate: wall time round the enqueue and the stream's drain (the entry records no events).  Each group of
workloads is warmed up, then its workloads alternate for --reps rounds; medians are kept.  One JSON line, also written to
profiles/mk_lhe_bench.json.

usage: python tools/mk_lhe_bench.py [--reps 5] [--device 0] [--counts 256,4096]
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
from thfhe import lut  # noqa: E402

HBM_BYTES_PER_S = 6.29e12   # measured float4 copy rate of one MI355X (8.0 TB/s spec)


def trivial_tgsw(p, bits):
    """Noiseless TGswSample_3gen of every bit: the gadget value on coefficient 0 of part_1 and part_3."""
    C = np.zeros((len(bits), 4, p.l, p.N), np.int64)
    for lv in range(p.l):
        g = np.asarray(bits, np.int64) << (64 - (lv + 1) * p.Bgbit)
        C[:, 0, lv, 0] = g
        C[:, 2, lv, 0] = g
    return C


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--counts", default="256,4096")
    args = ap.parse_args()
    counts = [int(c) for c in args.counts.split(",")]
    p = thfhe.make_params(**thfhe.CB_PARAM_SETS["CB-128"])
    rng = np.random.default_rng(0)
    bk = rng.integers(-2**63, 2**63, size=(1, p.n, 4, p.l, p.N), dtype=np.int64)
    ksk = np.zeros((1, p.N, p.ks_t, (1 << p.ks_basebit) - 1, p.n + 1), np.int32)
    ck = thfhe.MKCloudKey(p, bk, ksk, device=args.device)
    ck.set_tree_slice(1 << 18)   # 4096 samples x 32 accumulators: no call below is cut into slices, the events cover the whole call
    parts = (p.Bgbit + 8) // 9 if p.Bgbit > 10 else 1
    per_cmux = 2 * p.l * parts * 131072   # bytes of spectra one CMux streams
    med, spread, cmuxes, skipped = {}, {}, {}, {}

    # the shared-key rotation: `B` jobs of n CMuxes on random non-zero amounts
    B_max = max(counts)
    bara = rng.integers(1, 2 * p.N, size=(B_max, p.n)).astype(np.int32)
    d_bara, d_barb, d_acc = (thfhe.DeviceBuffer(ck, n) for n in (bara.nbytes, 4 * B_max, 16 * B_max * p.N))
    d_bara.upload(bara)
    d_barb.upload(np.zeros(B_max, np.int32))

    def rotate(B):
        t0 = time.perf_counter()
        thfhe._check(thfhe.lib().thfhe_mk_rotate_partial_dev(ck.h, d_bara.ptr, d_barb.ptr, 1 << 61, None, d_acc.ptr, B))
        ck.sync()
        return (time.perf_counter() - t0) * 1e3

    def group(work):
        """warm up, then alternate the workloads; work: name -> callable returning its milliseconds"""
        for run in work.values():
            run()
        t = {k: [] for k in work}
        for _ in range(args.reps):
            for k, run in work.items():
                t[k].append(run())
        for k, v in t.items():
            med[k], spread[k] = round(statistics.median(v), 3), [round(min(v), 3), round(max(v), 3)]

    for d_tree, d_rot in ((0, 10), (6, 10)):
        d = d_tree + d_rot
        name = f"lhe_{d_tree}_{d_rot}"
        tab = lut.lhe_table(rng.integers(0, 8, 1 << d) << 61, d_tree, d_rot, N=p.N, torus_bits=64)
        try:
            ts = ck.tgsw_set(trivial_tgsw(p, lut.lhe_address_bits(rng.integers(0, 1 << d, B_max), d)), d)
        except thfhe.ThfheError as e:
            skipped[name] = str(e)
            continue
        ck.set_profiling(True)

        def look(B, ts=ts, tab=tab, d_tree=d_tree, d_rot=d_rot):
            ck.lhe_lookup_wo_keyswitch(ts, tab, d_tree=d_tree, d_rot=d_rot, count=B)
            t = ck.last_timings()
            return t["total_ms"] - t["keyswitch_ms"]   # tree + rotation chain + extraction
        work = {}
        for B in counts:
            work[f"{name}_{B}"] = lambda B=B: look(B)
            cmuxes[f"{name}_{B}"] = B * ((1 << d_tree) - 1 + d_rot)
            work[f"rotate_{B}_next_to_{name}"] = lambda B=B: rotate(B)
            cmuxes[f"rotate_{B}_next_to_{name}"] = B * p.n
        group(work)
        ck.set_profiling(False)
        ts.close()

    res = dict(tool="mk_lhe_bench", params="CB-128", device=args.device, reps=args.reps, lib=os.path.basename(thfhe.LIB_PATH),
               timing="median of alternating rounds; lhe_*: device events tree .. extraction of thfhe_mk_lhe_lookup_wo_keyswitch; rotate_*: wall time "
                      "of thfhe_mk_rotate_partial_dev + stream drain",
               ms=med, ms_min_max=spread, cmuxes=cmuxes, cmuxes_per_s={k: round(n / (med[k] * 1e-3), 0) for k, n in cmuxes.items() if k in med},
               spectra_bytes_per_cmux=per_cmux,
               lhe_spectra_bytes_per_s={k: round(n * per_cmux / (med[k] * 1e-3), 0) for k, n in cmuxes.items() if k in med and k.startswith("lhe")},
               hbm_bytes_per_s=HBM_BYTES_PER_S, skipped=skipped,
               rotation_kernel={str(B): ck.rotation_kernel_name(B) for B in counts})
    line = json.dumps(res)
    print(line, flush=True)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "mk_lhe_bench.json"), "w") as f:
        f.write(line + "\n")
    for b in (d_bara, d_barb, d_acc):
        b.free()
    ck.close()


if __name__ == "__main__":
    main()
