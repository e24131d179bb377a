#!/usr/bin/env python3
"""Circuit-bootstrap nodes in the gate-DAG executor, timed in one process on one device (SK-128 at full size with its level-2 set CB-128, one-rotation
mode).

  one_run    a circuit that computes a 4-bit index with XOR gates and 16 candidates with gates, reads the candidates at the index (CB node, d = 4,
             GATHER of 16 at (1, 3)) and feeds the result into a NAND: wall time of ONE dag_run_cb_batch against the three-call host sequence of the
             same circuit (dag_run_batch for the gates, circuit_bootstrap, dag_run_lhe_batch with the wires uploaded again), at --instances.
  cb_group   a CB node of d = 4 on input wires at 2 048 bits (512 instances): the group's device time (thfhe_dag_last_group_ms) against the sum of
             the three stage intervals of the flat thfhe_circuit_bootstrap_mode on the same records (thfhe_last_timings).  With --parent-lib the
             flat call is also timed on that library, in a child process of this one (the same records; rounds do not alternate across processes).

Each pair is warmed up once, then alternates for --reps rounds; medians are kept.  The records are fresh encryptions: timing does not depend on the
words.  Writes one JSON line to --out and prints it.

usage: python tools/dag_cb_bench.py [--reps 5] [--device 0] [--instances 256,2048] [--parent-lib PATH] [--out profiles/dag_cb_bench.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "torus-fhe_amd"))
import thfhe  # noqa: E402
from thfhe import circuits as CI, keygen, threshold  # noqa: E402

T, BASEBIT, SIGMA_PKS = 7, 4, 2.0**-31
NAND, OR, AND, XOR = 0, 1, 2, 3
GROUP_INSTANCES, D = 512, 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--instances", default="256,2048")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--flat-only", action="store_true", help="time the flat call alone and print its median (the child of --parent-lib)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dag_cb_bench.json"))
    args = ap.parse_args()
    if args.flat_only:   # an earlier library: without the entries it does not have
        import ctypes
        L = ctypes.CDLL(thfhe.LIB_PATH)
        for name in [n for n in thfhe.SIGNATURES if not hasattr(L, n)]:
            del thfhe.SIGNATURES[name]
    p, p2 = thfhe.make_params("SK-128"), thfhe.make_params(**thfhe.CB_PARAM_SETS["CB-128"])
    s2 = thfhe.CB_SIGMAS["CB-128"]
    K = keygen.SecretKeySet(p, seed=0x5EED0001)
    K2 = keygen.MKSecretKeySet(p2, seed=0x5EED0002, sigma_lwe=s2["lwe"], sigma_bk=s2["bk"], sigma_ks=s2["ks"], device=args.device, lwe_keys=K.lwe_key[None, :])
    pks = keygen.gen_cb_key(np.random.default_rng(3), K2.rlwe_keys[0], K.rlwe_key, T, BASEBIT, SIGMA_PKS, device=args.device)
    ck = thfhe.CloudKey(p, K.bk, K.ksk, device=args.device)
    ck2 = thfhe.MKCloudKey(p2, K2.bk, K2.ksk, device=args.device)
    ck.cb_key_set(ck2, pks, T, BASEBIT)
    med = lambda v: statistics.median(v)
    group_recs = K.encrypt(np.random.default_rng(4).integers(0, 2, GROUP_INSTANCES * D), 5)

    def flat_ms():
        ck.set_profiling(True)
        ck.circuit_bootstrap(group_recs, D, one_rotation=True).close()
        ms = ck.last_timings()["total_ms"]
        ck.set_profiling(False)
        return ms

    if args.flat_only:
        flat_ms()
        print(json.dumps(dict(flat_stage_sum_ms=med([flat_ms() for _ in range(args.reps)]))))
        return

    pc = threshold.PolyContext(args.device)
    pk = keygen.gen_pack_key(np.random.default_rng(6), K.lwe_key, K.rlwe_key, p.ks_t, p.ks_basebit, thfhe.SIGMAS["SK-128"]["bk"])
    pc.set_pack_key(pk, p.ks_t, p.ks_basebit)

    # ---- cb_group: the CB group against the flat call ---------------------------------------------------------------------------------------
    one = CI.Circuit()
    one.cb_set(one.inputs(D))
    x_group = group_recs.reshape(GROUP_INSTANCES, D, -1)

    def group_ms():
        ck.set_profiling(True)
        ck.dag_run_cb_batch(x_group, one.nodes(), one_rotation=True, out_wires=[D], **one.cb_families())
        ms = ck.dag_last_group_ms()
        ck.set_profiling(False)
        return ms

    group_ms(), flat_ms()
    pairs = [(group_ms(), flat_ms()) for _ in range(args.reps)]
    group = dict(bits=GROUP_INSTANCES * D, d=D, group_ms=med([a for a, _ in pairs]), flat_stage_sum_ms=med([b for _, b in pairs]))
    group["group_over_flat"] = group["group_ms"] / group["flat_stage_sum_ms"]
    if args.parent_lib:
        child = subprocess.run([sys.executable, os.path.abspath(__file__), "--flat-only", "--reps", str(args.reps), "--device", str(args.device)],
                               env=dict(os.environ, THFHE_HIP_LIB=os.path.abspath(args.parent_lib)), capture_output=True, text=True, timeout=600)
        if child.returncode:
            raise SystemExit("the flat call on --parent-lib failed:\n" + child.stderr[-2000:])
        group["parent_flat_stage_sum_ms"] = json.loads(child.stdout.strip().splitlines()[-1])["flat_stage_sum_ms"]
        group["group_over_parent_flat"] = group["group_ms"] / group["parent_flat_stage_sum_ms"]

    # ---- one_run: one run against the three-call host sequence ----------------------------------------------------------------------------------
    cir = CI.Circuit()
    a, b, c = cir.inputs(D), cir.inputs(D), cir.inputs(9)
    idx = [cir.gate(XOR, u, v) for u, v in zip(a, b)]
    cand = [cir.gate((NAND, XOR, AND, OR)[i % 4], c[i % 8], c[(3 * i + 1) % 8]) for i in range(16)]
    read = CI.cb_array_read(cir, cand, idx, 1, 3)
    out = cir.gate(NAND, read, c[8])
    gates_only = CI.Circuit()            # call 1 of the host sequence: the gates
    gates_only.n_inputs, gates_only.gates = cir.n_inputs, cir.gates[:D + 16]
    tail = CI.Circuit()                  # call 3: the GATHER and the NAND on the wires uploaded again
    t_in = tail.inputs(17)
    t_out = tail.gate(NAND, tail.lhe_gather(0, t_in[0], 1, 3), t_in[16])

    def one_run(x):
        t = time.perf_counter()
        CI.evaluate_batch(ck, cir, x, out_wires=[out], pack=pc, one_rotation=True)
        return time.perf_counter() - t

    def host_sequence(x):
        t = time.perf_counter()
        w = CI.evaluate_batch(ck, gates_only, x, out_wires=idx + cand)
        with ck.circuit_bootstrap(w[:, :D].reshape(-1, w.shape[-1]), D, one_rotation=True) as ts:
            CI.evaluate_batch(ck, tail, np.concatenate([w[:, D:], x[:, -1:]], axis=1), out_wires=[t_out], pack=pc, tgsw_sets=[ts])
        return time.perf_counter() - t

    runs = []
    for q in [int(v) for v in args.instances.split(",")]:
        x = K.encrypt(np.random.default_rng(7).integers(0, 2, q * cir.n_inputs), 8).reshape(q, cir.n_inputs, -1)
        one_run(x), host_sequence(x)
        pairs = [(one_run(x), host_sequence(x)) for _ in range(args.reps)]
        r = dict(instances=q, d=D, gather=16, one_run_s=med([u for u, _ in pairs]), host_sequence_s=med([v for _, v in pairs]))
        r["host_over_one_run"] = r["host_sequence_s"] / r["one_run_s"]
        runs.append(r)

    res = dict(tool="dag_cb_bench", set="SK-128 + CB-128", mode="one rotation", t=T, basebit=BASEBIT, reps=args.reps, cb_group=group, one_run=runs)
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)
    pc.close()
    ck.close()
    ck2.close()


if __name__ == "__main__":
    main()
