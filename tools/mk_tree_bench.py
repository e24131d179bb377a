#!/usr/bin/env python3
"""The multi-key two-digit trees against the rotations they are made of, in one process on one device (3-gen sets, DESIGN.md sections 4.20, 4.23).

Times thfhe_mk_tree_lut_bootstrap at (p_hi, p_lo, theta_lo) = (4, 4, 1) and (4, 4, 2) on MK2 and MK4 (1024 samples) and MK16 (256 samples), and
thfhe_mk_lut_bootstrap at theta = 1 on the same batch and build.  Every call is timed by the context's device events (thfhe_mk_last_timings: for
the tree level 1 | packing | selection of the one slice the batch runs in).  Each workload is warmed up first, then the workloads of a set
alternate for --reps rounds; the median is kept.  The figure to hold the tree against is (p_hi / theta_lo + 1) x the rotation time plus the
packing.  The packing kernel's key traffic is the EXPECTED number of non-zero digits (D t (1 - 2^-basebit) per candidate) x 2N x 8 B over the
packing time, which also holds the box kernel -- what the direct mk_pack_rows_kernel requests; slices of 4 096 candidates and more run
mk_pack_rows_wide_kernel, which requests a row once per 32 records, so there the figure is a rate of rows APPLIED, not fetched.

The multi-value rows: thfhe_mk_tree_lut_bootstrap_mvk at (p_hi, p_lo, k) = (4, 4, 1) and (8, 8, 2) on the same batches, next to the
many-LUT rows: level 1 with its epilogue | packing | selection | tree, the packing-rows kernel the slice ran, and the expectation the tree is held
against -- one theta = 1 rotation of the batch (which carries a key switch the level-1 stage does not have) + the packing + k selections, i.e.
(1 + k) x the rotation time plus the packing.  These rows also go, alone, to profiles/mk_tree_mv_bench.json.

Every key is random words: no time of a stage depends on the key's contents, only on the inputs' zero mask words, and the inputs are uniform.
Writes one JSON line to profiles/mk_tree_bench.json and prints it.

usage: python tools/mk_tree_bench.py [--reps 7] [--device 0]
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

SETS = {"MK2": (1024, 12, 1), "MK4": (1024, 12, 1), "MK16": (256, 8, 1)}   # samples, packing digits t, basebit
TREES = ((4, 4, 1), (4, 4, 2))
MV_TREES = ((4, 4, 1), (8, 8, 2))   # (p_hi, p_lo, k)


def bench_set(name, B, t, basebit, reps, device):
    p = thfhe.make_params(name)
    rng = np.random.default_rng(1)
    bk = rng.integers(-2**63, 2**63, (p.parties, p.n, 4, p.l, p.N), dtype=np.int64)
    ksk = rng.integers(-2**31, 2**31, (p.parties, p.N, p.ks_t, (1 << p.ks_basebit) - 1, p.n + 1), dtype=np.int64).astype(np.int32)
    ck = thfhe.MKCloudKey(p, bk, ksk, device=device)
    del bk, ksk
    R = (1 << basebit) - 1
    pk = rng.integers(-2**63, 2**63, (p.N, t, R, 2, p.N), dtype=np.int64)
    ck.pack_key_set(pk, t, basebit)
    key_mib = pk.nbytes / 2**20
    del pk
    lo = rng.integers(-2**31, 2**31, (B, ck.words), dtype=np.int64).astype(np.int32)
    hi = rng.integers(-2**31, 2**31, (B, ck.words), dtype=np.int64).astype(np.int32)
    tv = lut.test_vector(lut.int_outputs(lambda m: m ^ 1, 4, torus_bits=64), 4, 1, p.N, torus_bits=64)
    work = {"lut_theta1": lambda: ck.lut_bootstrap(tv, lo)}
    for p_hi, p_lo, th in TREES:
        tv1 = lut.tree_test_vectors(lambda h, l: (h + l) & 1, p_hi, p_lo, 2, th, p.N, torus_bits=64)
        work[f"tree_{p_hi}x{p_lo}_theta{th}"] = lambda tv1=tv1, p_hi=p_hi, th=th: ck.tree_lut_bootstrap(tv1, lo, hi, p_hi=p_hi, theta=th)
    for p_hi, p_lo, k in MV_TREES:
        tv0, w = lut.tree_mvk_factors([lambda h, l, j=j: (h + l + j) & 1 for j in range(k)], p_hi, p_lo, 2, N=p.N, torus_bits=64)
        work[f"tree_mv_{p_hi}x{p_lo}_k{k}"] = lambda tv0=tv0, w=w: ck.tree_lut_bootstrap_mvk(w, lo, hi, tv0=tv0)
    pack_kernels = {(p_hi, k): ck.pack_kernel_name(B * k * p_hi) for p_hi, _, k in MV_TREES}
    ck.set_profiling(True)
    for run in work.values():
        run()
    ms = {k: [] for k in work}
    for _ in range(reps):
        for k, run in work.items():
            run()
            ms[k].append(tuple(ck.last_timings().values()))
    ck.set_profiling(False)
    ck.close()
    med = {k: [statistics.median(col) for col in zip(*v)] for k, v in ms.items()}
    rot = med["lut_theta1"][3]
    out = dict(samples=B, pack_digits=[t, basebit], pack_key_mib=round(key_mib), lut_theta1_ms=round(rot, 3), lut_theta1_per_s=round(B / rot * 1e3))
    for p_hi, p_lo, th in TREES:
        l1, pack, sel, tot = med[f"tree_{p_hi}x{p_lo}_theta{th}"]
        key_bytes = B * p_hi * p.N * t * (1 - 2.0**-basebit) * 2 * p.N * 8
        out[f"tree_{p_hi}x{p_lo}_theta{th}"] = dict(
            level1_ms=round(l1, 3), packing_ms=round(pack, 3), selection_ms=round(sel, 3), total_ms=round(tot, 3), trees_per_s=round(B / tot * 1e3),
            rotations_plus_packing_ms=round((p_hi // th + 1) * rot + pack, 3), packing_key_GBps=round(key_bytes / (pack * 1e-3) / 1e9, 1),
            packing_over_level1=round(pack / l1, 3))
    for p_hi, p_lo, k in MV_TREES:
        l1, pack, sel, tot = med[f"tree_mv_{p_hi}x{p_lo}_k{k}"]
        out[f"tree_mv_{p_hi}x{p_lo}_k{k}"] = dict(
            level1_ms=round(l1, 3), packing_ms=round(pack, 3), selection_ms=round(sel, 3), total_ms=round(tot, 3), trees_per_s=round(B / tot * 1e3),
            functions_per_s=round(B * k / tot * 1e3), rotations_plus_packing_ms=round((1 + k) * rot + pack, 3), candidates=B * k * p_hi,
            pack_rows_kernel=pack_kernels[(p_hi, k)], packing_over_level1=round(pack / l1, 3))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--sets", default=",".join(SETS))
    args = ap.parse_args()
    res = dict(tool="mk_tree_bench", device=args.device, reps=args.reps, timing="device events, median of alternating rounds, one process",
               keys="random words", sets={name: bench_set(name, *SETS[name], args.reps, args.device) for name in args.sets.split(",")})
    line = json.dumps(res)
    with open(os.path.join(ROOT, "profiles", "mk_tree_bench.json"), "w") as f:
        f.write(line + "\n")
    keep = ("samples", "pack_digits", "pack_key_mib", "lut_theta1_ms", "lut_theta1_per_s")
    mv = dict(res, tool="mk_tree_bench (multi-value rows)",
              sets={name: {k: v for k, v in row.items() if k in keep or k.startswith("tree_mv_")} for name, row in res["sets"].items()})
    with open(os.path.join(ROOT, "profiles", "mk_tree_mv_bench.json"), "w") as f:
        f.write(json.dumps(mv) + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
