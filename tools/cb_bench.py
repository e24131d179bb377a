#!/usr/bin/env python3
"""Circuit bootstrapping timing in one process on one device (SK-128 at full size with its level-2 set CB-128).

For count x d = 256 and 4 096 bits it times thfhe_circuit_bootstrap and reports
  bits_per_s       wall time of the host-buffer call (upload of the records, the three stages, allocation of the set's spectra)
  stage_a_ms       device events: one prologue and l level-2 rotations + extractions per bit
  stage_b_ms       the private key switch, on the plain kernel and on the matrix-core kernel at the same shape (thfhe_cb_set_batch_threshold)
  transform_ms     the key transform of the rows into the set
  key_bytes_per_s  stage B: the key bytes its kernel has to read (plain: inputs x 2 D t 8 KiB; matrix cores: 256-input tiles x the byte planes)
                   over stage_b_ms
The events are those of the call's LAST slice (2 048 bits), whose size is reported.  --sweep adds stage B on both kernels at small batches: the
figures behind the threshold kCbBatchMinInputs.  Each workload is warmed up, then the kernels alternate for --reps rounds; medians are kept.
The records are fresh encryptions, not gate outputs: timing does not depend on the words.  Writes one JSON line to --out and prints it.

--mode both times the default stage A (l level-2 rotations per bit) against the one-rotation mode (THFHE_CB_ONE_ROTATION) instead: the two modes
alternate for --reps rounds in this one process, stage B on the library's own choice of kernel, and every workload reports per mode stage A / B /
transform ms (device events, last slice), bits per second (wall), and the ratios per-level / one-rotation.  --mode one-rotation runs the workloads
above in that mode.

usage: python tools/cb_bench.py [--reps 5] [--device 0] [--bits 256,4096] [--sweep 1,2,4,8,16,64] [--mode per-level|one-rotation|both]
                                [--out profiles/cb_bench.json]
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

T, BASEBIT, SIGMA_PKS, D = 7, 4, 2.0**-31, 2048
SLICE_BITS = 2048          # kCbSliceBits
PLAIN, MFMA = 1 << 40, 1   # batch thresholds that force a kernel


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--bits", default="256,4096")
    ap.add_argument("--sweep", default="1,2,4,8,16,64")
    ap.add_argument("--d", type=int, default=16)
    ap.add_argument("--mode", choices=("per-level", "one-rotation", "both"), default="per-level")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cb_bench.json"))
    args = ap.parse_args()
    bits = [int(b) for b in args.bits.split(",")]
    sweep = [int(b) for b in args.sweep.split(",")] if args.sweep else []
    p, p2 = thfhe.make_params("SK-128"), thfhe.make_params(**thfhe.CB_PARAM_SETS["CB-128"])
    s2 = thfhe.CB_SIGMAS["CB-128"]
    t0 = time.perf_counter()
    K = keygen.SecretKeySet(p, seed=0x5EED0001)
    K2 = keygen.MKSecretKeySet(p2, seed=0x5EED0002, sigma_lwe=s2["lwe"], sigma_bk=s2["bk"], sigma_ks=s2["ks"], device=args.device, lwe_keys=K.lwe_key[None, :])
    pks = keygen.gen_cb_key(np.random.default_rng(3), K2.rlwe_keys[0], K.rlwe_key, T, BASEBIT, SIGMA_PKS, device=args.device)
    keygen_s = time.perf_counter() - t0
    ck = thfhe.CloudKey(p, K.bk, K.ksk, device=args.device)
    ck2 = thfhe.MKCloudKey(p2, K2.bk, K2.ksk, device=args.device)
    ck.cb_key_set(ck2, pks, T, BASEBIT)
    ck.set_profiling(True)
    recs = K.encrypt(np.random.default_rng(4).integers(0, 2, max(bits + sweep)), 5)
    row_bytes = 2 * D * T * 8192

    def run(nbits, thr, one_rotation=args.mode == "one-rotation"):
        d = args.d if nbits % args.d == 0 else 1
        ck.cb_set_batch_threshold(thr)
        t = time.perf_counter()
        ck.circuit_bootstrap(recs[:nbits], d, one_rotation=one_rotation).close()
        wall = time.perf_counter() - t
        ms = ck.last_timings()
        return wall, ms["prologue_ms"], ms["blind_rotate_ms"], ms["keyswitch_ms"]

    def measure(nbits):
        for thr in (PLAIN, MFMA):
            run(nbits, thr)                       # warm-up of both shapes
        got = {PLAIN: [], MFMA: []}
        for _ in range(args.reps):                # alternating rounds
            for thr in (PLAIN, MFMA):
                got[thr].append(run(nbits, thr))
        med = {thr: [statistics.median(v[q] for v in got[thr]) for q in range(4)] for thr in got}
        last = nbits % SLICE_BITS or min(nbits, SLICE_BITS)           # bits of the last slice: what the events cover
        inputs = last * p.l
        key_bytes = {PLAIN: inputs * row_bytes, MFMA: -(-inputs // 256) * row_bytes}
        return dict(bits=nbits, last_slice_bits=last, stage_b_inputs=inputs,
                    bits_per_s={"plain": nbits / med[PLAIN][0], "mfma": nbits / med[MFMA][0]},
                    stage_a_ms=med[MFMA][1], transform_ms=med[MFMA][3],
                    stage_b_ms={"plain": med[PLAIN][2], "mfma": med[MFMA][2]},
                    key_bytes_per_s={"plain": key_bytes[PLAIN] / (med[PLAIN][2] * 1e-3), "mfma": key_bytes[MFMA] / (med[MFMA][2] * 1e-3)})

    def measure_modes(nbits):
        modes = {"per_level": False, "one_rotation": True}
        for one in modes.values():
            run(nbits, 0, one)                    # warm-up of both modes
        got = {m: [] for m in modes}
        for _ in range(args.reps):                # alternating rounds
            for m, one in modes.items():
                got[m].append(run(nbits, 0, one))
        med = {m: [statistics.median(v[q] for v in got[m]) for q in range(4)] for m in got}
        out = dict(bits=nbits, last_slice_bits=nbits % SLICE_BITS or min(nbits, SLICE_BITS))
        for m in modes:
            out[m] = dict(bits_per_s=nbits / med[m][0], stage_a_ms=med[m][1], stage_b_ms=med[m][2], transform_ms=med[m][3])
        out["stage_a_ratio"] = med["per_level"][1] / med["one_rotation"][1]
        out["bits_per_s_ratio"] = med["per_level"][0] / med["one_rotation"][0]
        return out

    if args.mode == "both":
        res = dict(tool="cb_bench", mode="both", set="SK-128 + CB-128", l=p.l, theta=4 if p.l > 2 else p.l, t=T, basebit=BASEBIT, D=D, reps=args.reps,
                   rotation_kernel={str(b): ck2.rotation_kernel_name(min(b, SLICE_BITS)) for b in bits}, workloads=[measure_modes(b) for b in bits])
        line = json.dumps(res)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
        print(line)
        ck.close()
        ck2.close()
        return

    res = dict(tool="cb_bench", set="SK-128 + CB-128", t=T, basebit=BASEBIT, D=D, key_MiB=row_bytes / 2**20, keygen_s=keygen_s, reps=args.reps,
               workloads=[measure(b) for b in bits],
               sweep=[dict(bits=m["bits"], inputs=m["stage_b_inputs"], stage_b_ms=m["stage_b_ms"]) for m in (measure(b) for b in sweep)])
    for w in res["workloads"]:
        w["dominant"] = "stage A" if w["stage_a_ms"] > w["stage_b_ms"]["mfma"] else "stage B"
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)
    ck.close()
    ck2.close()


if __name__ == "__main__":
    main()
