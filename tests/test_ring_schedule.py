"""The ring kernel's key hand-off schedule (torus-fhe_amd/csrc/thfhe_ring_schedule.h) replayed on the CPU by tests/cpp/ring_schedule_test.cpp
under AddressSanitizer + UBSan: l = 1 .. 4, four and eight waves, n = 1, 2, 3 and 630.  GPU twin: tests/test_gpu_ring_handoff.py."""
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_handoff_schedule_replay_under_asan(tmp_path):
    exe = str(tmp_path / "ring_schedule_test")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall","-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-fno-omit-frame-pointer", "-o", exe, os.path.join(ROOT, "tests", "cpp", "ring_schedule_test.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["errors"] == 0 and res["cases"] == 4 * 2 * 4
    assert res["broken"] == res["rejected"] > 0          # the checker rejects every broken schedule it is shown
    assert res["barriers_per_row"] == 3 and res["issues_per_row"] == 4
