#!/usr/bin/env python3
"""Layered-automaton timing in one process on one device (SK-128).

For 256 and 4096 samples it times
  wfa_S      thfhe_lhe_wfa of a 64-step automaton with n_states = S in {1, 8, 32}: every state of every step is a CMux (its two transitions
             differ), so a call is 64 S CMuxes per sample; the 64 steps walk the 4 bits of one set
  lhe_6_10   thfhe_lhe_lookup at (d_tree, d_rot) = (6, 10) on the same build: 63 + 10 CMuxes per sample, each streaming its own spectra
The TGSW samples are noiseless (zero mask): timing does not depend on the words.  Device events (first step .. extraction of a call that is not
cut into slices) and the wall time of the host-buffer call.  Each workload is warmed up, then the workloads alternate for --reps rounds; medians
are kept.  A workgroup of thfhe_lhe_wfa loads the 2l x 32 KiB of spectra of its sample's bit once per step and chunk of states; the tool reports
CMuxes/s and the achieved bytes/s of spectra (ceil(S / chunk) loads per sample and step) and of TLWE operands (16 KiB read + 8 KiB written per CMux).  One JSON line, also written to
profiles/wfa_bench.json.

usage: python tools/wfa_bench.py [--reps 5] [--device 0] [--counts 256,4096] [--states 1,8,32]
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
STEPS, BITS = 64, 4


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
    ap.add_argument("--counts", default="256,4096")
    ap.add_argument("--states", default="1,8,32")
    ap.add_argument("--no-lookup", action="store_true", help="skip the thfhe_lhe_lookup comparison (its set is count x 16 x 192 KiB)")
    args = ap.parse_args()
    counts = [int(c) for c in args.counts.split(",")]
    states = [int(c) for c in args.states.split(",")]
    p = thfhe.make_params("SK-128")
    K = keygen.SecretKeySet(p, seed=0x5EED0001)
    ck = thfhe.CloudKey(p, K.bk, K.ksk, device=args.device)
    rng = np.random.default_rng(0)
    ts = ck.tgsw_set(trivial_tgsw(p, rng.integers(0, 2, max(counts) * BITS)), BITS)
    sets, work, cmuxes, chunks, spec_loads = [ts], {}, {}, {}, {}
    import torch
    cus = torch.cuda.get_device_properties(args.device).multi_processor_count
    step_bit = (np.arange(STEPS) % BITS).astype(np.int32)
    for S in states:
        q = np.arange(S)
        layer = np.stack([(q + 1) % S, (q + 2) % S], axis=1) if S > 1 else np.zeros((1, 2), np.int64)   # S = 1: the one state copies itself
        trans = np.repeat(layer[None], STEPS, axis=0).astype(np.int32)
        fin = lut.wfa_finals(rng.integers(0, 8, S), encode=lambda v: lut.encode(v, 8))
        for B in counts:
            k = f"wfa_{S}_{B}"
            work[k] = lambda trans=trans, fin=fin, B=B: ck.lhe_wfa([ts], trans, step_bit, fin, [0], count=B)
            cmuxes[k] = B * STEPS * S if S > 1 else 0
            # the automatic chunk of the library (wfa_chunk_for): the largest G with ceil(S / G) B >= compute units, else 1; a workgroup loads the
            # 2l x 32 KiB of its sample's bit once per step (l <= 3), so a call loads B STEPS ceil(S / G) sets of spectra
            G = next((g for g in range(S, 1, -1) if -(-S // g) * B >= cus), 1)
            chunks[k] = G
            if S > 1:
                spec_loads[k] = B * STEPS * -(-S // G)
    if not args.no_lookup:
        tab = lut.lhe_table(rng.integers(0, 8, 1 << 16), 6, 10, encode=lambda v: lut.encode(v, 8))
        t16 = ck.tgsw_set(trivial_tgsw(p, lut.lhe_address_bits(rng.integers(0, 1 << 16, max(counts)), 16)), 16)
        sets.append(t16)
        for B in counts:
            work[f"lhe_6_10_{B}"] = lambda B=B: ck.lhe_lookup(t16, tab, d_tree=6, d_rot=10, count=B)
            cmuxes[f"lhe_6_10_{B}"] = B * 73
    ck.set_tree_slice(1 << 20)   # 4096 samples x 2 x 32 states: no call below is cut into slices, the events cover the whole call
    ck.set_profiling(True)
    for run in work.values():
        run()
    wall, dev = {k: [] for k in work}, {k: [] for k in work}
    for _ in range(args.reps):
        for k, run in work.items():
            t0 = time.perf_counter()
            run()
            wall[k].append((time.perf_counter() - t0) * 1e3)
            t = ck.last_timings()
            dev[k].append(t["total_ms"] - t["keyswitch_ms"])   # wfa: steps + extraction; lhe: tree + rotations
    ck.set_profiling(False)
    med = lambda d: {k: round(statistics.median(v), 3) for k, v in d.items()}
    spread = lambda d: {k: [round(min(v), 3), round(max(v), 3)] for k, v in d.items()}
    c = med(dev)
    per_cmux = 2 * p.l * 32768
    res = dict(tool="wfa_bench", params="SK-128", device=args.device, reps=args.reps, steps=STEPS, lib=os.path.abspath(thfhe.LIB_PATH),
               timing="median of alternating rounds; wall = host-buffer call, cmux_ms = device events first step .. extraction (lhe: tree + rotations)",
               wall_ms=med(wall), wall_ms_min_max=spread(wall), cmux_ms=c, cmux_ms_min_max=spread(dev), cmuxes=cmuxes,
               cmuxes_per_s={k: round(n / (c[k] * 1e-3), 0) for k, n in cmuxes.items() if n},
               spectra_bytes_per_cmux=per_cmux, tlwe_bytes_per_cmux=24576,
               lhe_spectra_bytes_per_s={k: round(n * per_cmux / (c[k] * 1e-3), 0) for k, n in cmuxes.items() if k.startswith("lhe")},
               wfa_chunk=chunks, wfa_spectra_bytes_per_s={k: round(spec_loads[k] * per_cmux / (c[k] * 1e-3), 0) for k in spec_loads},
               wfa_tlwe_bytes_per_s={k: round(n * 24576 / (c[k] * 1e-3), 0) for k, n in cmuxes.items() if n and k.startswith("wfa")},
               hbm_bytes_per_s=HBM_BYTES_PER_S,
               note="wfa_1_*: the one state copies itself, no CMux runs (64 copy launches); wfa_spectra_bytes_per_s counts one load of the spectra per "
                    "chunk and step, which holds for l <= 3 (SK-128: l = 3) -- the l = 4 kernel requests them per CMux")
    line = json.dumps(res)
    print(line, flush=True)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "wfa_bench.json"), "w") as f:
        f.write(line + "\n")
    for s in sets:
        s.close()
    ck.close()


if __name__ == "__main__":
    main()
