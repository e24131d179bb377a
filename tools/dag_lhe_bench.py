#!/usr/bin/env python3
"""Leveled gather nodes in the gate-DAG executor, timing in one process on one device (SK-128).

For every (2^d, instances) of --d x --instances, a circuit whose one node picks one of 2^d input wires:
  gather_dag    an LHE_GATHER node at (d_tree, d_rot) = (max(d - 9, 0), min(d, 9)) through thfhe_dag_run_lhe_batch;
  gather_flat   the same gather as flat calls through the host: thfhe_pack_boxes, then thfhe_lhe_lookup on the packed samples;
  select_dag    at 2^d = 16 only: a THFHE_SELECT node at p = 16 through the same entry (its index: one more input wire), the bootstrapped pick.
Timing only: the records and the TGSW samples are random words; the two gather forms are checked to give the same words.  Each workload is warmed
up, then the workloads alternate for --reps rounds; medians are kept.  device_ms: HIP events on the gate context's stream around the node's launch
group alone (thfhe_set_profiling / thfhe_dag_last_group_ms: gather kernel to scatter, no copy and no allocation inside) -- the figure that compares
a GATHER with a SELECT.  wall_ms: the whole host-buffer call, uploads of the input wires included; gather_flat has only this one, its trips through
the host being what it measures.  Writes one JSON line to profiles/dag_lhe_bench.json (rewritten after every shape, so a run cut short leaves the
shapes it finished) and prints it.

usage: python tools/dag_lhe_bench.py [--reps 5] [--device 0] [--d 4 9] [--instances 256 4096]
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
from thfhe import circuits as Cc, keygen  # noqa: E402
from thfhe import threshold as T  # noqa: E402


def words(rng, *shape):
    return rng.integers(-2**31, 2**31, size=shape, dtype=np.int32)   # drawn as int32: no wider temporary


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--d", type=int, nargs="+", default=[4, 9])
    ap.add_argument("--instances", type=int, nargs="+", default=[256, 4096])
    args = ap.parse_args()
    p = thfhe.make_params("SK-128")
    K = keygen.SecretKeySet(p, seed=0x5EED0001)
    ck = thfhe.CloudKey(p, K.bk, K.ksk, device=args.device)
    rng = np.random.default_rng(0)
    pc = T.PolyContext(args.device)
    pc.set_pack_key(keygen.gen_pack_key(rng, K.lwe_key, K.rlwe_key, p.ks_t, p.ks_basebit, thfhe.SIGMAS["SK-128"]["bk"]), p.ks_t, p.ks_basebit)
    res = dict(tool="dag_lhe_bench", params="SK-128", device=args.device, reps=args.reps, lib=os.path.basename(thfhe.LIB_PATH),
               timing="median of alternating rounds; device_ms: events around the node's launch group, wall_ms: the host-buffer call", device_ms={},
               wall_ms={}, same_words={})
    ck.set_profiling(True)
    for d in args.d:
        d_rot, d_tree = min(d, 9), max(d - 9, 0)
        P = 1 << d
        for Q in args.instances:
            x = words(rng, Q, P + 1, ck.words)
            ts = ck.tgsw_set(words(rng, Q * d, 2 * p.l, 2, p.N), d)
            cir = Cc.Circuit()
            w = cir.inputs(P + 1)
            out = cir.lhe_gather(0, w[0], d_tree, d_rot)
            work = {"gather_dag": lambda: Cc.evaluate_batch(ck, cir, x, [out], pack=pc, tgsw_sets=[ts])}

            def flat():
                a, b = T.PackBoxes(pc, x[:, :P].reshape(-1, ck.words), 1 << d_rot)
                return ck.lhe_lookup(ts, b, d_tree=d_tree, d_rot=d_rot, tab_a=a, table_index=np.arange(Q))
            work["gather_flat"] = flat
            if P == 16:
                sel = Cc.Circuit()
                v = sel.inputs(P + 1)
                s_out = sel.select([v[P]], v[0], P)
                work["select_dag"] = lambda: Cc.evaluate_batch(ck, sel, x, [s_out], pack=pc)
            tag = f"{P}x{Q}"
            res["same_words"][tag] = bool(np.array_equal(work["gather_dag"]()[:, 0], work["gather_flat"]()[:, 0]))   # also the warm-up
            for run in work.values():
                run()
            wall, dev = {k: [] for k in work}, {k: [] for k in work if k != "gather_flat"}
            for _ in range(args.reps):
                for k, run in work.items():
                    t0 = time.perf_counter()
                    run()
                    wall[k].append((time.perf_counter() - t0) * 1e3)
                    if k in dev:
                        dev[k].append(ck.dag_last_group_ms())
            res["wall_ms"][tag] = {k: round(statistics.median(v), 3) for k, v in wall.items()}
            res["device_ms"][tag] = {k: round(statistics.median(v), 3) for k, v in dev.items()}
            ts.close()
            line = json.dumps(res)
            os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
            with open(os.path.join(ROOT, "profiles", "dag_lhe_bench.json"), "w") as f:
                f.write(line + "\n")
            print(tag, "done", file=sys.stderr, flush=True)
    print(line, flush=True)
    ck.close()
    pc.close()


if __name__ == "__main__":
    main()
