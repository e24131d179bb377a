#!/usr/bin/env python3
"""The wide packing-rows kernel against the direct one, in one process on one device (3-gen sets).

Times the packing stage of thfhe_mk_tree_lut_bootstrap_mvk (mk_pack_rows_wide_kernel or mk_pack_rows_kernel, then mk_pack_boxes_kernel; ms[1] of
thfhe_mk_last_timings, device events) at 64, 256, 1 024, 4 096 and 16 384 candidates in one slice -- (p_hi, k) = (64, 1), so candidates / 64 samples
-- on D = N keys of random words: N = 1024 with (t, basebit) = (12, 1), N = 2048 with (8, 1), and the multi-bit (8, 2) at N = 1024.  The
candidates are the level-1 rotation's own outputs, uniform words to the packing.  The bootstrapping keys are cut to n = 16 and two parties: the
rotations only feed the packing, whose time depends on N, D, t and basebit alone.  Each size is warmed up through both kernels, then the two
alternate for --reps rounds (thfhe_mk_set_pack_wide_threshold 1 / 0).

The threshold the measurement chooses for a key: the smallest measured size from which on -- at it and at every larger measured size -- the wide
kernel's median lies below the direct kernel's MINIMUM over the rounds; none if there is no such size.  The library's default is the largest of
the keys' choices (the direct kernel where any key prefers it).  Writes one JSON line to profiles/mk_pack_wide_bench.json and prints it.

usage: python tools/mk_pack_bench.py [--reps 7] [--device 0]
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
from thfhe import lut  # noqa: E402

KEYS = {"N1024_t12_b1": ("MK2", 12, 1), "N2048_t8_b1": ("MK4-N2048", 8, 1), "N1024_t8_b2": ("MK2", 8, 2)}
SIZES = (64, 256, 1024, 4096, 16384)
P_HI = 64


def bench_key(name, t, basebit, reps, device, sizes):
    p = thfhe.make_params(name, n=16, parties=2)
    rng = np.random.default_rng(1)
    bk = rng.integers(-2**63, 2**63, (p.parties, p.n, 4, p.l, p.N), dtype=np.int64)
    ksk = rng.integers(-2**31, 2**31, (p.parties, p.N, p.ks_t, (1 << p.ks_basebit) - 1, p.n + 1), dtype=np.int64).astype(np.int32)
    ck = thfhe.MKCloudKey(p, bk, ksk, device=device)
    del bk, ksk
    pk = rng.integers(-2**63, 2**63, (p.N, t, (1 << basebit) - 1, 2, p.N), dtype=np.int64)
    ck.pack_key_set(pk, t, basebit)
    key_mib = pk.nbytes / 2**20
    del pk
    tv0, w = lut.tree_mvk_factors([lambda h, l: (h + l) & 1], P_HI, 2, 2, N=p.N, torus_bits=64)
    ck.set_profiling(True)
    rows = {}
    for cand in sizes:
        B = cand // P_HI
        lo = rng.integers(-2**31, 2**31, (B, ck.words), dtype=np.int64).astype(np.int32)
        hi = rng.integers(-2**31, 2**31, (B, ck.words), dtype=np.int64).astype(np.int32)
        ms = {"wide": [], "direct": []}

        def run(kind):
            ck.set_pack_wide_threshold(1 if kind == "wide" else 0)
            assert ck.pack_kernel_name(cand) == ("mk_pack_rows_wide_kernel" if kind == "wide" else "mk_pack_rows_kernel")
            ck.tree_lut_bootstrap_mvk(w, lo, hi, tv0=tv0)
            return ck.last_timings()["blind_rotate_ms"]   # ms[1]: the packing stage of a tree call

        for kind in ms:
            run(kind)
        for _ in range(reps):
            for kind in ms:
                ms[kind].append(run(kind))
        wide, direct = statistics.median(ms["wide"]), statistics.median(ms["direct"])
        key_bytes = cand * p.N * t * (1 - 2.0**-basebit) * 2 * p.N * 8    # the direct kernel's requests: one row per non-zero digit
        rows[str(cand)] = dict(wide_ms=round(wide, 4), wide_min_ms=round(min(ms["wide"]), 4), wide_max_ms=round(max(ms["wide"]), 4),
                               direct_ms=round(direct, 4), direct_min_ms=round(min(ms["direct"]), 4), direct_max_ms=round(max(ms["direct"]), 4),
                               speedup=round(direct / wide, 3), wins=bool(wide < min(ms["direct"])),
                               direct_key_GBps=round(key_bytes / (direct * 1e-3) / 1e9, 1))
    ck.set_profiling(False)
    ck.close()
    chosen = None
    for cand in reversed(sizes):      # the smallest size from which on the wide kernel wins at every measured size
        if not rows[str(cand)]["wins"]:
            break
        chosen = cand
    return dict(N=p.N, pack_digits=[t, basebit], pack_key_mib=round(key_mib), sizes=rows, threshold=chosen)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--keys", default=",".join(KEYS))
    ap.add_argument("--sizes", default=",".join(map(str, SIZES)))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mk_pack_wide_bench.json"))
    args = ap.parse_args()
    sizes = tuple(int(s) for s in args.sizes.split(","))
    keys = {k: bench_key(*KEYS[k], args.reps, args.device, sizes) for k in args.keys.split(",")}
    th = [v["threshold"] for v in keys.values()]
    res = dict(tool="mk_pack_bench", device=args.device, reps=args.reps, timing="device events, packing stage of a tree call, alternating rounds, one process",
               keys_are="random words", rule="smallest measured size from which the wide median < the direct minimum at every larger measured size",
               keys=keys, default_threshold=None if None in th else max(th))
    line = json.dumps(res)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
