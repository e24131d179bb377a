"""The rotation-kernel rules of torus-fhe_amd/csrc/thfhe_launch_plan.h, checked on the CPU by tests/cpp/launch_plan_test.cpp under
AddressSanitizer + UBSan (the shape of every single-key plan), and every kernel name it reports compared with the rules the Python host
layer held before the library answered for itself: the four functions below are that layer's rules, frozen.  GPU twin:
tests/test_gpu_launch_plan.py."""
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SK_THRESHOLDS = [(768, 1024), (0, 0), (0, 1024), (768, 0), (1 << 20, 1024), (6, 6), (100, 6), (200, 1024), (300, 1024)]
ROTATIONS = (1, 256, 257, 5000)
PAIR_THRESHOLDS = (0, 256, 1 << 20)
CCS_SHAPES = [(2, 3), (8, 8), (9, 3), (16, 3), (4, 9)]


# ---- the frozen rules (CloudKey / MKCloudKey / KMSCloudKey / CCSCloudKey.rotation_kernel_name as they were) --------------------------------
def sk_name(l, rotations, coop=768, ring4=1024):
    r = rotations % 2048 if (coop or ring4) else 0
    if rotations >= 2048 or r == 0:
        return f"sk_blind_rotate_ring_kernel<{l}>"
    if r <= coop:
        return f"sk_blind_rotate_coop_kernel<{l}>"
    return f"sk_blind_rotate_ring_kernel<{l}, 4 waves>" if r <= ring4 + min(coop, 256) and ring4 else f"sk_blind_rotate_ring_kernel<{l}>"


def mk_name(N, l, Bgbit, rotations, pair_threshold=256):
    if N == 4096:
        return "r4k_rotate_kernel"
    if N == 2048:
        le = l * (((Bgbit + 8) // 9) if Bgbit > 10 else 1)
        pair = rotations > pair_threshold
        if le > 3:
            return "kms_tlev_rotate_pair_kernel" if pair else "kms_tlev_rotate_kernel"
        return f"mk_blind_rotate_{'pair2k' if pair else 'coop2k'}_kernel<{le}>"
    pair = l <= 3 and rotations > pair_threshold
    return f"mk_blind_rotate_{'pair' if pair else 'coop'}_kernel<{l}>"


def kms_name(rotations, pair_threshold=256):
    return "kms_tlev_rotate_pair_kernel" if rotations > pair_threshold else "kms_tlev_rotate_kernel"


def ccs_name(parties, l):
    return "ccs_blind_rotate_wide_kernel" if parties > 8 or l > 8 else "ccs_blind_rotate_kernel"


def three_gen_shapes():
    import thfhe
    return sorted({(s["N"], s["l"], s["Bgbit"]) for s in thfhe.PARAM_SETS.values() if s["torus_bits"] == 64})


def test_launch_plan_under_asan_names_what_the_python_rules_named(tmp_path):
    exe, names = str(tmp_path / "launch_plan_test"), str(tmp_path / "names.txt")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-fno-omit-frame-pointer", "-o", exe, os.path.join(ROOT, "tests", "cpp", "launch_plan_test.cpp")], check=True)
    shapes = three_gen_shapes()
    assert len(shapes) >= 8 and {N for N, _, _ in shapes} == {1024, 2048, 4096}
    r = subprocess.run([exe, names] + ["%d:%d:%d" % s for s in shapes], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["errors"] == 0 and res["sk_plans"] == len(SK_THRESHOLDS) * 6201

    expected = {}
    for coop, ring4 in SK_THRESHOLDS:
        for jobs in range(6201):
            for l in (1, 2, 3, 4):
                expected[f"sk {l} {coop} {ring4} {jobs}"] = sk_name(l, jobs, coop, ring4)
    for N, l, Bgbit in shapes:
        for thr in PAIR_THRESHOLDS:
            for rot in ROTATIONS:
                expected[f"mk {N} {l} {Bgbit} {thr} {rot}"] = mk_name(N, l, Bgbit, rot, thr)
    for thr in PAIR_THRESHOLDS:
        for rot in ROTATIONS:
            expected[f"kms {thr} {rot}"] = kms_name(rot, thr)
    for parties, l in CCS_SHAPES:
        expected[f"ccs {parties} {l}"] = ccs_name(parties, l)
    assert res["names"] == len(expected)

    got = {}
    with open(names) as f:
        for line in f:
            engine, *rest = line.rstrip("\n").split(" ", {"sk": 5, "mk": 6, "kms": 3, "ccs": 3}[line.split(" ", 1)[0]])
            got[" ".join([engine] + rest[:-1])] = rest[-1]
    assert got.keys() == expected.keys()
    wrong = [(k, got[k], expected[k]) for k in expected if got[k] != expected[k]]
    assert not wrong, (len(wrong), wrong[:10])
    # the grid reaches every name there is to report
    assert {n.split("<")[0] + ("<4w>" if "4 waves" in n else "") for n in got.values()} == {
        "sk_blind_rotate_ring_kernel", "sk_blind_rotate_ring_kernel<4w>", "sk_blind_rotate_coop_kernel", "mk_blind_rotate_coop_kernel",
        "mk_blind_rotate_pair_kernel", "mk_blind_rotate_coop2k_kernel", "mk_blind_rotate_pair2k_kernel", "kms_tlev_rotate_kernel",
        "kms_tlev_rotate_pair_kernel", "r4k_rotate_kernel", "ccs_blind_rotate_kernel", "ccs_blind_rotate_wide_kernel"}
