"""Context lifetime on the GPU (pytest -m gpu): creating and destroying engine contexts returns all their device memory.  Every
destroy frees through the members' destructors (csrc/thfhe_devctx.h), so a buffer missing from a context would show up here."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Runs in a fresh process that imports torch before the engine, so that torch.cuda.mem_get_info sees the same HIP runtime as the
# library.  Keys are zeros of the right sizes: only the allocations matter.  One gate batch per context grows its workspace and staging.
CHILD = r"""
import sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1])
import thfhe

def sk128():
    p = thfhe.make_params("SK-128")
    ck = thfhe.CloudKey(p, np.zeros(p.n * 2 * p.l * 2 * p.N, np.int32), np.zeros(p.N * p.ks_t * 3 * (p.n + 1), np.int32))
    ck.gates(thfhe.NAND, np.zeros((64, ck.words), np.int32), np.zeros((64, ck.words), np.int32))
    return ck

def mk2():
    p = thfhe.make_params("MK2")
    ck = thfhe.MKCloudKey(p, np.zeros(p.parties * p.n * 4 * p.l * p.N, np.int64),
                          np.zeros(p.parties * p.N * p.ks_t * ((1 << p.ks_basebit) - 1) * (p.n + 1), np.int32))
    ck.gates(thfhe.NAND, np.zeros((64, ck.words), np.int32), np.zeros((64, ck.words), np.int32))
    return ck

def ccs():
    p = thfhe.make_params("CCS2", n=20)
    ck = thfhe.CCSCloudKey(p, np.zeros(p.parties * p.n * 3 * p.l * p.N, np.int32), np.zeros(p.parties * p.l * p.N, np.int32),
                           np.zeros(p.l * p.N, np.int32), np.zeros(p.parties * p.N * p.ks_t * 3 * (p.n + 1), np.int32))
    ck.gates(thfhe.NAND, np.zeros((16, ck.words), np.int32), np.zeros((16, ck.words), np.int32))
    return ck

def polymac():
    pm = thfhe.PolyMac(1024, 32)
    pm.mac(np.zeros((2, 1024), np.int32), np.zeros((2, 1024), np.int32), np.array([[0, 0, 0, 1], [1, 1, 1, -1]], np.int32), 2)
    return pm

torch.cuda.init()
makers = (sk128, mk2, ccs, polymac)
for make in makers:   # warm-up: code objects and runtime pools are loaded once per process
    make().close()
torch.cuda.synchronize()
free0 = torch.cuda.mem_get_info(0)[0]
for _ in range(3):
    for make in makers:
        make().close()
torch.cuda.synchronize()
free1 = torch.cuda.mem_get_info(0)[0]
print("free", free0, free1)
"""


def test_create_destroy_returns_device_memory():
    env = dict(os.environ, THFHE_TORCH_FIRST="1")
    r = subprocess.run([sys.executable, "-c", CHILD, os.path.join(ROOT, "torus-fhe_amd")], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    free0, free1 = (int(v) for v in r.stdout.split("free")[-1].split())
    assert abs(free0 - free1) <= 1 << 20, f"free device memory {free0} -> {free1} after 3 x (SK-128, MK2, CCS, polymac) create + destroy"
