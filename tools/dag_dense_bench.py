#!/usr/bin/env python3
"""Dense-layer nodes of the gate-DAG executor against the flat calls they replace, on one device (SK-128).

Two workloads, each in two forms that alternate for --reps rounds after a warm-up (medians, with min - max, of the wall clock of whole calls):

  (a) one level: ONE 784 -> 128 DENSE node on 32 instances (4 096 rotations) through thfhe_dag_run_dense_batch, against
      thfhe_linear_lut_bootstrap on the same records.  The flat call is also timed on the DAG side's own context (`a_flat_same_context`): two
      contexts hold two copies of the bootstrapping key, and the rotation kernel's time differs between them by more than the DAG path adds.
  (b) a network: 784 -> 16 -> 16 -> 10 with an argmax tail (circuits.dense_argmax: 45 LUT nodes, NOTs and ANDs) on 32 instances as ONE run,
      against the same three layers as flat calls in a row -- the M records of every sample come down and go up again as the next layer's inputs --
      and a thfhe_dag_run_lut_batch for the tail.

The flat forms touch nothing this node added, so they run on an older tree: --flat-root names the tree whose thfhe package and library time them
(default: this one).  Each side is a worker process with its own context; the parent process alternates them, one call at a time, so drift of the
machine hits both alike.

After the timed rounds come --reps profiled rounds, again alternating, which give the STAGES of both forms (medians): for a DAG run the Python
marshalling (wall clock of the whole call less that of the C entry), the host work of the C entry before its first event (checks, plan, workspace,
upload of the table families: the entry's wall clock less its events' span), and by device events the uploads into the wire table, the levels, the
DENSE group within them (thfhe_dag_last_group_ms), the dense kernel within that (thfhe_linear_last_timings), and the output gather and download
(thfhe_dag_last_stage_ms); for the flat call the same split as far as its events go (input upload, kernel, upload start .. key-switch end).

--flat-label names the flat side's tree in the output; the libraries are named by their path inside their tree.  --bench-py-parent / --bench-py-this
take the one-line JSON results of bench.py runs made next to this tool (the parent's checkout and this tree alternating in the same job) and copy
their values and the command into the document, so that one file holds every figure of DESIGN 4.25.  Writes one JSON document to --out and prints it.

usage: python tools/dag_dense_bench.py [--reps 5] [--device 0] [--flat-root TREE] [--flat-label TEXT] [--bench-py-parent F ...] [--bench-py-this F ...]
                                       [--out profiles/dag_dense_bench.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q, P = 32, 8
LAYER_A = (128, 784)
NET = ((16, 784), (16, 16), (10, 16))


def worker(side, root, device):
    """one side's context and workloads; runs the workload named on every line of stdin and answers with one JSON line"""
    sys.path.insert(0, os.path.join(os.path.abspath(root), "torus-fhe_amd"))
    import thfhe
    from thfhe import circuits as CI
    from thfhe import keygen, lut

    p = thfhe.make_params("SK-128")
    keys = keygen.SecretKeySet(p, seed=0x5EED0001)
    ck = thfhe.CloudKey(p, keys.bk, keys.ksk, device=device)
    rng = np.random.default_rng(0)
    x = rng.integers(-2**31, 2**31, (Q, 784, p.n + 1), dtype=np.int64).astype(np.int32)   # the timing does not depend on the words
    Wa = rng.integers(-1, 2, LAYER_A).astype(np.int32)
    Wn = [rng.integers(-1, 2, s).astype(np.int32) for s in NET]
    tv = lut.test_vector(lut.int_outputs(lambda m: min(m, P // 2 - 1), P), P)

    def tail(cir, scores):
        """circuits.dense_argmax, spelled out so that an older tree's package builds the same rows"""
        ge = cir.table(lut.test_vector(lut.bool_outputs(lambda s: s >= P // 2, P), P))
        n, beats, winners = len(scores), {}, []
        for i in range(n):
            for j in range(i + 1, n):
                beats[i, j] = cir.lut(ge, [scores[i], scores[j]], weights=(1, -1), bias=int(lut.encode(P // 2, P)))[0]
                beats[j, i] = cir.gate(thfhe.NOT, beats[i, j])
        for i in range(n):
            terms = [beats[i, j] for j in range(n) if j != i]
            w = terms[0]
            for t in terms[1:]:
                w = cir.gate(thfhe.AND, w, t)
            winners.append(w)
        return winners

    if side == "dag":
        ca = CI.Circuit()
        ia = ca.inputs(784)
        ca.table(tv)
        ca.dense(ca.dense_layer(Wa), ia)
        cb = CI.Circuit()
        ib = cb.inputs(784)
        t = cb.table(tv)
        outs = CI.dense_network(cb, ib, [(W, None, [t] * W.shape[0]) for W in Wn])
        win = tail(cb, outs[-1])
        runs = dict(a=lambda: CI.evaluate_batch(ck, ca, x, out_wires=list(range(784, 784 + 128))), b=lambda: CI.evaluate_batch(ck, cb, x, out_wires=win),
                    f=lambda: ck.linear_lut_bootstrap(tv[None], Wa, x)[:, :, 0])     # (a)'s flat call on THIS context: same process, same key in HBM
    else:
        ct = CI.Circuit()
        it = ct.inputs(10)
        win = tail(ct, it)

        def flat_net():
            h = x
            for W in Wn:
                h = ck.linear_lut_bootstrap(tv[None], W, h)[:, :, 0]
            return CI.evaluate_batch(ck, ct, np.ascontiguousarray(h), out_wires=win)
        runs = dict(a=lambda: ck.linear_lut_bootstrap(tv[None], Wa, x)[:, :, 0], b=flat_net)
    # the wall clock of the C entries alone: the rest of a call is Python marshalling
    L, c_ms = thfhe.lib(), {}
    for sym in ("thfhe_dag_run_dense_batch", "thfhe_dag_run_lut_batch", "thfhe_linear_lut_bootstrap"):
        if hasattr(L, sym):
            def timed(*a, _f=getattr(L, sym), _s=sym):
                t = time.perf_counter()
                r = _f(*a)
                c_ms[_s] = c_ms.get(_s, 0.0) + (time.perf_counter() - t) * 1e3
                return r
            setattr(L, sym, timed)
    print(json.dumps(dict(ready=side, lib=os.path.relpath(thfhe.LIB_PATH, os.path.abspath(root)))), flush=True)
    for line in sys.stdin:
        cmd = line.split()
        if not cmd or cmd[0] == "quit":
            break
        name, profiled = cmd[0], len(cmd) > 1
        ck.set_profiling(profiled)
        c_ms.clear()
        t0 = time.perf_counter()
        out = runs[name]()
        ms = (time.perf_counter() - t0) * 1e3
        ans = dict(ms=ms, crc=int(np.bitwise_xor.reduce(np.asarray(out, np.int32).reshape(-1).view(np.uint32))))
        if profiled:
            lt, c_wall = ck.linear_last_timings(), sum(c_ms.values())
            ans.update(python_ms=ms - c_wall, c_entries_ms=c_wall, linear_kernel_ms=lt["linear_ms"])
            if name in "af":                # the PBS stage of the layer: prologue | rotations | key switch (thfhe_last_timings)
                pt = ck.last_timings()
                ans.update(pbs_prologue_ms=pt["prologue_ms"], pbs_rotations_ms=pt["blind_rotate_ms"], pbs_keyswitch_ms=pt["keyswitch_ms"])
            if side == "dag" and name != "f":
                st = ck.dag_last_stage_ms()
                ans.update(host_before_events_ms=c_wall - sum(st.values()), upload_ms=st["upload_ms"], levels_ms=st["levels_ms"],
                           last_group_ms=ck.dag_last_group_ms(), gather_download_ms=st["download_ms"])
            elif name in "af":
                ans.update(input_upload_ms=lt["upload_ms"], upload_to_keyswitch_ms=lt["total_ms"], download_and_host_ms=c_wall - lt["total_ms"])
            ck.set_profiling(False)
        print(json.dumps(ans), flush=True)
    ck.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--flat-root", default=HERE)
    ap.add_argument("--flat-label", default="this tree")
    ap.add_argument("--bench-py-parent", nargs="*", default=[])
    ap.add_argument("--bench-py-this", nargs="*", default=[])
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "dag_dense_bench.json"))
    ap.add_argument("--worker", nargs=2, metavar=("SIDE", "ROOT"))
    args = ap.parse_args()
    if args.worker:
        return worker(args.worker[0], args.worker[1], args.device)

    def start(side, root):
        env = dict(os.environ)
        env.pop("THFHE_HIP_LIB", None)     # each side loads the library of its own tree
        pr = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--device", str(args.device), "--worker", side, root], stdin=subprocess.PIPE,
                              stdout=subprocess.PIPE, text=True, env=env)
        return pr, json.loads(pr.stdout.readline())

    def ask(pr, cmd):
        pr.stdin.write(cmd + "\n")
        pr.stdin.flush()
        line = pr.stdout.readline()
        if not line:
            raise RuntimeError("a worker ended early")
        return json.loads(line)

    dag, dag_hello = start("dag", HERE)
    flat, flat_hello = start("flat", args.flat_root)
    times, crc = {}, {}
    try:
        for name in "ab":                   # warm-up: code objects loaded, workspace and staging grown; the two forms agree before anything is timed
            crc[name] = [ask(pr, name)["crc"] for pr in (dag, flat)]
            assert crc[name][0] == crc[name][1], "the DAG run and the flat calls differ on workload (%s)" % name
        assert ask(dag, "f")["crc"] == crc["a"][0]
        # one form of a workload after the other, the order rotating from round to round: the rotation kernel's time depends by a few per cent
        # on what the device ran just before, and no form should always follow the same one
        forms = dict(a=[("a_dag_ms", dag, "a"), ("a_flat_ms", flat, "a"), ("a_flat_same_context_ms", dag, "f")], b=[("b_dag_ms", dag, "b"), ("b_flat_ms", flat, "b")])
        for r in range(args.reps):
            for name in "ab":
                order = forms[name][r % len(forms[name]):] + forms[name][:r % len(forms[name])]
                for key, pr, cmd in order:
                    times.setdefault(key, []).append(ask(pr, cmd)["ms"])
        stages = {}
        for r in range(args.reps):          # the stages, profiling on: the last DENSE group's kernel is the whole layer in (a), the last layer in (b)
            for name in "ab":
                order = forms[name][r % len(forms[name]):] + forms[name][:r % len(forms[name])]
                for key, pr, cmd in order:
                    for k, v in ask(pr, cmd + " profiled").items():
                        if k != "crc":
                            stages.setdefault(key[:-3], {}).setdefault(k, []).append(v)
    finally:
        for pr in (dag, flat):
            try:
                pr.stdin.write("quit\n")
                pr.stdin.flush()
            except OSError:
                pass
            pr.wait(timeout=60)
    med = {k: round(statistics.median(v), 3) for k, v in times.items()}
    res = dict(tool="dag_dense_bench", params="SK-128", instances=Q, device=args.device, reps=args.reps,
               workload_a="one %d -> %d DENSE node, %d rotations" % (LAYER_A[1], LAYER_A[0], Q * LAYER_A[0]),
               workload_b="%s network + argmax tail, %d rotations in the layers" % (" -> ".join([str(NET[0][1])] + [str(s[0]) for s in NET]), Q * sum(s[0] for s in NET)),
               timing="wall clock of whole calls (inputs up, records down), medians of alternating rounds after a warm-up, the order of the forms rotating "
                      "from round to round; stages by device events and host clocks in as many profiled rounds",
               dag_library="this tree: " + dag_hello["lib"], flat_library=args.flat_label + ": " + flat_hello["lib"],
               ms=med, ms_min={k: round(min(v), 3) for k, v in times.items()}, ms_max={k: round(max(v), 3) for k, v in times.items()},
               a_rotations_per_s=dict(dag=round(Q * LAYER_A[0] / med["a_dag_ms"] * 1e3, 1), flat=round(Q * LAYER_A[0] / med["a_flat_ms"] * 1e3, 1)),
               a_dag_vs_flat_rate=round(med["a_flat_ms"] / med["a_dag_ms"], 4), a_bar=0.95,
               a_dag_vs_flat_same_context_rate=round(med["a_flat_same_context_ms"] / med["a_dag_ms"], 4),
               b_dag_vs_flat=round(med["b_flat_ms"] / med["b_dag_ms"], 4),
               stages_note="medians of profiled rounds (profiling on adds event records; `ms` is the whole profiled call): python_ms = whole call "
                           "less its C entries; DAG: host_before_events_ms = C entry less (upload + levels + gather_download), last_group_ms inside "
                           "levels_ms, linear_kernel_ms inside last_group_ms; flat (a): download_and_host_ms = C entry less upload_to_keyswitch_ms",
               stages_ms={w: {k: round(statistics.median(v), 4) for k, v in d.items()} for w, d in stages.items()})
    res["a_below_bar"] = res["a_dag_vs_flat_rate"] < res["a_bar"]
    if args.bench_py_parent or args.bench_py_this:
        value = lambda f: round(json.loads(open(f).read().strip().splitlines()[-1])["value"], 1)
        first = json.loads(open((args.bench_py_this or args.bench_py_parent)[0]).read().strip().splitlines()[-1])
        res["bench_py"] = dict(command="bench.py --gpus 1 --steps %d --warmup %d" % (first["steps"], first["warmup"]),
                               order="the flat side's tree and this tree alternating in the same job, in the order given",
                               gates_per_s={args.flat_label: [value(f) for f in args.bench_py_parent], "this tree": [value(f) for f in args.bench_py_this]})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
