#!/usr/bin/env python3
"""The multi-key two-digit tree on the CPU model with full-size keys (no GPU): every (hi, lo) of a bit table on p = 4 x 4
through tests/mk_pack_reference.py's tree -- level-1 rotations on the oracle, the packing key switch with a generated D = N key, the selection
rotation and the oracle's multi-key key switch -- with fresh inputs.  Prints, in torus units, the standard deviation of the packed tables' phase
error under Z = sum_q z_q, of the outputs' phase error against +-1/8, and how many outputs decrypt.

usage: python tools/mk_tree_noise.py [--digits 12] [--seed 1] [set ...]        (default sets: MK2 MK4)
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "torus-fhe_amd"))

import mk_lut_reference as R     # noqa: E402
import mk_pack_reference as MP   # noqa: E402
import oracle_lib as O           # noqa: E402
from support import pmap         # noqa: E402
from thfhe import keygen, lut    # noqa: E402


def measure(name, digits, seed):
    p = O.make_params(name)
    s = O.SIGMAS[name]
    K = O.MKKeys(p, seed, s["bk"], s["ks"])
    orc = O.MKOracle(p, K.bk, K.ksk)
    Z = K.rlwe_keys.sum(axis=0)
    pk = keygen.gen_mk_pack_key(np.random.default_rng(seed + 1), Z, K.rlwe_keys, digits, 1, s["bk"])
    f = lambda h, l: ((h * 5 + l * 3 + (h & l)) >> 1) & 1
    tv1 = np.stack([lut.test_vector(lut.bool_outputs(lambda l, h=h: f(h, l), 4, torus_bits=64), 4, N=p.N, torus_bits=64) for h in range(4)])
    pairs = [(h, l) for h in range(4) for l in range(4)]
    hi = R.encrypt_words(K, lut.encode([h for h, _ in pairs], 4), s["lwe"], seed + 2)
    lo = R.encrypt_words(K, lut.encode([l for _, l in pairs], 4), s["lwe"], seed + 3)
    t0 = time.perf_counter()
    res = pmap(lambda g: MP.tree(orc, pk, digits, 1, tv1, [lo[g]], [hi[g]], 4, parts=True), range(len(pairs)))
    want = np.array([f(h, l) for h, l in pairs]).astype(bool)
    out = np.stack([r[0] for r in res])
    err = (K.phases(out).astype(np.int64) - np.where(want, 1 << 29, -(1 << 29))) / 2.0**32
    tab = []
    for (h, l), r in zip(pairs, res):
        ph = (r[3].view(np.uint64) - keygen.polymul_small64(r[2][None], Z)[0].view(np.uint64)).view(np.int64)
        ideal = lut.test_vector(lut.bool_outputs(lambda hh: f(hh, l), 4, torus_bits=64), 4, N=p.N, torus_bits=64)
        tab.append((ph.view(np.uint64) - ideal.view(np.uint64)).view(np.int64) / 2.0**64)
    tab = np.stack(tab)
    ok = int((K.decrypt_bits(out) == want).sum())
    print(f"{name}: {digits} one-bit digits, key seed {seed}: packed table std {tab.std():.2e} (max {np.abs(tab).max():.2e}) over {tab.size} coefficients; "
          f"output std {err.std():.2e} (max {np.abs(err).max():.2e}), half-step / std {0.125 / err.std():.1f}; {ok} of {len(pairs)} outputs decrypt; "
          f"{time.perf_counter() - t0:.0f} s", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--digits", type=int, default=12)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("sets", nargs="*", default=["MK2", "MK4"])
    args = ap.parse_args()
    for name in args.sets:
        measure(name, args.digits, args.seed)


if __name__ == "__main__":
    main()
