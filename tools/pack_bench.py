#!/usr/bin/env python3
"""The LWE -> TLWE packing key switch and the threshold decryption it feeds, in one process on one device.

Times: the packing key's upload (rows + matrix-core planes, SK-128); thfhe_pack_lwe on 4096 SK-128 samples at slots = 32 and 1024 and on
1, 7 / 8 and 32 samples (7 / 8: the two sides of the plain / matrix-core threshold); the full 3-party threshold decryption of 4096 bits, packed 1024 per
sample (pack + 3 partial decryptions + final decryption), for SK-128 and SK-lib; and for SK-lib the same decryption unpacked (per-bit
TLweFromLwe).  The poly context's calls copy from and to host arrays and synchronise their stream, so every figure is host wall clock
around whole calls, transfers included.  Each workload is warmed up first, then the workloads alternate for --reps rounds; the median
is kept.  Prints one JSON line.

usage: python tools/pack_bench.py [--reps 7] [--device 0]
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
from thfhe import keygen  # noqa: E402
from thfhe import threshold as T  # noqa: E402

N = 1024


def ms_of(run):
    t0 = time.perf_counter()
    run()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    ctx = T.PolyContext(args.device)
    keys, lwe = {}, {}
    t_keygen = {}
    for name in ("SK-128", "SK-lib"):
        p = thfhe.make_params(name)
        s, z = rng.integers(0, 2, p.n).astype(np.int32), rng.integers(0, 2, N).astype(np.int32)
        t0 = time.perf_counter()
        keys[name] = (keygen.gen_pack_key(rng, s, z, p.ks_t, p.ks_basebit, thfhe.SIGMAS[name]["bk"]), p.ks_t, p.ks_basebit)
        t_keygen[name] = (time.perf_counter() - t0) * 1e3
        lwe[name] = rng.integers(-2**31, 2**31, size=(4096, p.n + 1), dtype=np.int64).astype(np.int32)
    shares = [rng.integers(-1, 2, N).astype(np.int32) for _ in range(3)]
    noise = rng.integers(-2**12, 2**12, size=(4096, N)).astype(np.int32)

    def decrypt(a, b):
        parts = np.stack([T.PartialDecrypt(ctx, s, a, noise[:a.shape[0]]) for s in shares])
        return T.finalDecrypt(ctx, b, parts, want_result=True)

    def packed_flow(name):
        a, b = T.PackLwe(ctx, lwe[name], 1024)
        return decrypt(a, b)

    def unpacked_flow():
        a, b = T.TLweFromLwe(ctx, lwe["SK-lib"])
        return decrypt(a, b)

    ms = {}
    # the key upload (one per set, so it alternates with nothing): warm-up, then --reps uploads
    for name in ("SK-lib", "SK-128"):
        ctx.set_pack_key(*keys[name])
        ms[f"key_upload_{name}"] = [ms_of(lambda: ctx.set_pack_key(*keys[name])) for _ in range(args.reps)]
    work = {
        "pack_sk128_4096_slots32": lambda: T.PackLwe(ctx, lwe["SK-128"], 32),
        "pack_sk128_4096_slots1024": lambda: T.PackLwe(ctx, lwe["SK-128"], 1024),
        "pack_sk128_1_plain": lambda: T.PackLwe(ctx, lwe["SK-128"][:1], 32),
        "pack_sk128_7_plain": lambda: T.PackLwe(ctx, lwe["SK-128"][:7], 32),
        "pack_sk128_8_mfma": lambda: T.PackLwe(ctx, lwe["SK-128"][:8], 32),
        "pack_sk128_32_mfma": lambda: T.PackLwe(ctx, lwe["SK-128"][:32], 32),
        "threshold3_sk128_4096_packed": lambda: packed_flow("SK-128"),
    }
    for run in work.values():
        run()
    for k in work:
        ms[k] = []
    for _ in range(args.reps):
        for k, run in work.items():
            ms[k].append(ms_of(run))
    ctx.set_pack_key(*keys["SK-lib"])
    work2 = {"threshold3_sklib_4096_packed": lambda: packed_flow("SK-lib"), "threshold3_sklib_4096_unpacked": unpacked_flow}
    for run in work2.values():
        run()
    for k in work2:
        ms[k] = []
    for _ in range(args.reps):
        for k, run in work2.items():
            ms[k].append(ms_of(run))
    ctx.close()
    med = {k: statistics.median(v) for k, v in ms.items()}
    res = dict(tool="pack_bench", device=args.device, reps=args.reps, timing="host wall clock around whole calls (transfers included), median",
               ms={k: round(v, 3) for k, v in med.items()}, ms_min={k: round(min(v), 3) for k, v in ms.items()},
               ms_max={k: round(max(v), 3) for k, v in ms.items()}, keygen_cpu_ms={k: round(v, 1) for k, v in t_keygen.items()},
               sklib_packed_vs_unpacked=round(med["threshold3_sklib_4096_unpacked"] / med["threshold3_sklib_4096_packed"], 3))
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
