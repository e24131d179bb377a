"""The parameter sets that earlier rounds only extrapolated or checked at reduced size, run at the reference's FULL size on one MI355X and
compared with the CPU oracle where the oracle affords it.  Every check function returns one record; the script prints it as one JSON line:
`python tests/full_size_checks.py <check> [...]` (not collected by pytest itself; it lives under tests/ because it calls the CPU oracle).
tests/test_gpu_full_size.py runs mk32 (with its LUT), kms2 and ccs4-oracle in the GPU suite through the same functions and asserts on the
records; the others stay script-only (40 - 190 s of key generation and oracle time each).  Checks:

  mk32      mktfhe_parameters_32party_3gen (mk_api.jl:225-231 region): P = 32, n = 620, N = 2048 -- a batch timed + decrypted, 2 gates word for word vs the oracle
  mk32-lut  mk32 on one key set, then a programmable bootstrap (theta = 2) on the pair kernel: 2 of 3 samples word for word vs tests/mk_lut_reference.py
  mk64 / mk128   the 64- and 128-party sets the same way (1 oracle gate each: 42 k / 86 k sequential CMuxes on one host thread)
  mk256     mktfhe_parameters_256party_3gen (mk_api.jl:304-310): P = 256, n = 740, N = 2048, l = 2, Bgbit = 18 -- the 185 GB of key spectra resident in
            HBM, one batch timed + decrypted, 1 gate vs the oracle at the full size (189 k CMuxes)
  kms2      mktfhe_parameters_2party_new (mk_api.jl:12-20) at n = 560: 8 gates (and 8 fast_boot gates) word for word vs the oracle, OpenMP over gates
  mk64fft / mk512   the sets on the ring of degree 4096 (mk_api.jl:277-283, 316-322): timing + decryption at full size (mk512: as many parties as fit)
  mk64fft-oracle   the 64-party set on the ring of degree 4096 with a VALID key set (from the oracle's key generation): 64 gates decrypted, 1 gate vs the oracle
  ccs{2,4,8,16}-oracle   the CCS sets (mk_api.jl:4-10, 56-62, 111-117, 185-191) at n = 560 with the oracle's keys: 8 / 4 / 2 / 1 gates vs the oracle
  kms4 / kms8   the 4- and 8-party KMS sets (mk_api.jl:64-72, 120-128) at n = 560: 2 / 1 gates vs the oracle
  ccs16     the 16-party CCS set (mk_api.jl:185-191), n = 560: timing + decryption at full size
Keys of the 3-gen sets are generated on the device (thfhe_pm_mac under thfhe/keygen.py) from the host's randomness, so the oracle sees the same key."""
import contextlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "torus-fhe_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))   # oracle_lib
import thfhe
from thfhe import keygen


def emit(**kw):
    print(json.dumps(kw), flush=True)


def note(msg):
    """progress on stderr: the GPU box takes a silent command for a hung one after a few minutes"""
    print(f"[full_size_checks {time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr, flush=True)


def _watch(msg):
    """a daemon thread that notes `msg` every 120 s until the returned event is set"""
    import threading
    stop = threading.Event()
    threading.Thread(target=lambda: [note(msg) for _ in iter(lambda: stop.wait(120), True)], daemon=True).start()
    return stop


@contextlib.contextmanager
def _oracle_threads(O, gates):
    """the oracle's OpenMP team sized for `gates` independent gates, the previous size restored after (the checks also run in the pytest suite)"""
    before = O.lib().oracle_max_threads()
    O.lib().oracle_set_threads(min(gates, O.usable_cpus()))
    try:
        yield
    finally:
        O.lib().oracle_set_threads(before)


def _gate_ids(oracle_gates):
    """`oracle_gates` as gate indices: a count means the leading gates"""
    return list(range(oracle_gates)) if isinstance(oracle_gates, int) else [int(g) for g in oracle_gates]


def mk_keys(name, parties=None):
    """Device key generation of a 3-gen set at full size and its evaluation context: (params, keys, context, keygen s, context s)."""
    over = dict(parties=parties) if parties else {}
    p = thfhe.make_params(name, **over)
    sig = thfhe.SIGMAS[name]
    t0 = time.time()
    K = keygen.MKSecretKeySet(p, seed=0x5EED0001, sigma_lwe=sig["lwe"], sigma_bk=sig["bk"], sigma_ks=sig["ks"], device=0)
    t_key = time.time() - t0
    note(f"{name}: keys generated in {t_key:.0f} s ({K.bk.nbytes / 1e9:.1f} GB of key coefficients)")
    t0 = time.time()
    ck = thfhe.MKCloudKey(p, K.bk, K.ksk, device=0)
    t_ctx = time.time() - t0
    note(f"{name}: key spectra resident after {t_ctx:.0f} s")
    return p, K, ck, t_key, t_ctx


def mk_check(name, batch, oracle_gates, parties=None, keys=None):
    """`batch` NANDs of a 3-gen set at full size, every output decrypted, the gates `oracle_gates` (a count of leading gates, or gate indices)
    word for word against the oracle.  keys: an mk_keys() result to use (its context stays open); else keys are made here.  Returns the record."""
    import oracle_lib as O
    over = dict(parties=parties) if parties else {}
    p, K, ck, t_key, t_ctx = keys if keys is not None else mk_keys(name, parties)
    rng = np.random.default_rng(0)
    a, b = rng.integers(0, 2, batch), rng.integers(0, 2, batch)
    xa, xb = K.encrypt(a, 1), K.encrypt(b, 2)
    ck.gates(thfhe.NAND, xa[:2], xb[:2])
    t0 = time.time()
    out = ck.gates(thfhe.NAND, xa, xb)
    dt = time.time() - t0
    note(f"{name}: {batch} gates in {dt:.2f} s")
    ok = bool(np.array_equal(K.decrypt(out), ~(a.astype(bool) & b.astype(bool))))
    rec = dict(check=name, workload=f"{batch} mk_gate_nand_3gen, {name} at full size (P={p.parties}, n={p.n}, N={p.N}, l={p.l}, Bgbit={p.Bgbit}, ks {p.ks_t}/{p.ks_basebit})",
               kernel=ck.rotation_kernel_name(batch), cmuxes_per_gate=p.parties * p.n, key_coefficients_gb=K.bk.nbytes / 1e9,
               gates_per_s=batch / dt, seconds=dt, keygen_s=t_key, ctx_create_s=t_ctx, all_decrypt_correct=ok)
    ids = _gate_ids(oracle_gates)
    if ids:
        po = O.make_params(name, **over)
        t0 = time.time()
        orc = O.MKOracle(po, K.bk, K.ksk)
        note(f"{name}: oracle evaluating {len(ids)} gate(s) of {p.parties * p.n} CMuxes")
        stop = _watch("oracle still running")
        with _oracle_threads(O, len(ids)):
            ref = orc.gates(O.NAND, xa[ids], xb[ids])
        stop.set()
        rec.update(oracle_gates=len(ids), oracle_seconds=time.time() - t0, words_equal_to_oracle=bool(np.array_equal(out[ids], ref)),
                   words_compared=int(ref.size))
        if ids != list(range(len(ids))):
            rec.update(oracle_gate_ids=ids)
    if keys is None:
        ck.close()
    return rec


def mk_lut_check(name, count, theta, picks, keys, pair_threshold=None):
    """Programmable bootstrap (thfhe_mk_lut_bootstrap) of `count` random records (two inputs, weights, bias, two tables picked per sample) on a
    3-gen set at full size: the samples `picks` word for word against tests/mk_lut_reference.py, in the _wo_keyswitch and the key-switched
    outputs.  keys: an mk_keys() result; pair_threshold: thfhe_mk_set_pair_threshold first (0: the two-jobs-per-workgroup kernel at any
    count).  Returns the record."""
    from concurrent.futures import ThreadPoolExecutor
    import mk_lut_reference as R
    import oracle_lib as O
    p, K, ck = keys[:3]
    if pair_threshold is not None:
        ck.set_pair_threshold(pair_threshold)
    rng = np.random.default_rng(9)
    recs = [rng.integers(-2**31, 2**31, (count, ck.words), dtype=np.int64).astype(np.int32) for _ in range(2)]
    weights, bias = (3, -5), int(rng.integers(-2**31, 2**31))
    tvs = rng.integers(-2**63, 2**63, (2, p.N), dtype=np.int64)
    idx = rng.integers(0, 2, count).astype(np.int32)
    kw = dict(weights=weights, bias=bias, theta=theta, lut_index=idx)
    t0 = time.time()
    wo = ck.lut_bootstrap_wo_keyswitch(tvs, *recs, **kw)
    ks = ck.lut_bootstrap(tvs, *recs, **kw)
    dt = time.time() - t0
    orc = O.MKOracle(O.make_params(**p.as_dict()), K.bk, K.ksk)
    note(f"{name}: reference of {len(picks)} LUT sample(s) of {p.parties * p.n} CMuxes")
    stop = _watch("LUT reference still running")
    t0 = time.time()
    with ThreadPoolExecutor(len(picks)) as pool:   # ctypes drops the GIL; the oracle's scratch is per thread
        ref = list(pool.map(lambda g: R.lut_bootstrap(orc, [r[g] for r in recs], weights, bias, tvs[idx[g]], theta, keyswitch=False), picks))
        ref_ks = list(pool.map(lambda u: np.stack([orc.keyswitch(v) for v in u]), ref))
    stop.set()
    return dict(check=name + "-lut", workload=f"{count} mk_lut_bootstrap (theta {theta}, 2 inputs), {name} at full size (P={p.parties}, n={p.n}, N={p.N})",
                kernel=ck.rotation_kernel_name(count), seconds=dt, reference_samples=list(picks), reference_seconds=time.time() - t0,
                wo_keyswitch_equal_to_reference=all(np.array_equal(wo[g], u) for g, u in zip(picks, ref)),
                keyswitched_equal_to_reference=all(np.array_equal(ks[g], u) for g, u in zip(picks, ref_ks)),
                words_compared=int(sum(u.size for u in ref) + sum(u.size for u in ref_ks)))


def kms2_check(gates=8, batch=256):
    """KMS2 (mk_gate_nand_new) at n = 560: `batch` gates and as many fast_boot gates decrypted, the first `gates` of each word for word
    against the oracle.  Returns the record."""
    import oracle_lib as O
    from thfhe import kms
    p = thfhe.make_kms_params("KMS2")
    t0 = time.time()
    K = keygen.KMSSecretKeySet(p, seed=1)
    t_key = time.time() - t0
    ck = kms.KMSCloudKey(p, K.gsw, K.uni, K.pk, K.crs, K.ksk, device=0)
    rng = np.random.default_rng(0)
    a, b = rng.integers(0, 2, batch), rng.integers(0, 2, batch)
    xa, xb = K.encrypt(a, 1), K.encrypt(b, 2)
    kms.mk_gate_nand_new(ck, xa[:4], xb[:4])
    t0 = time.time()
    out = kms.mk_gate_nand_new(ck, xa, xb)
    dt = time.time() - t0
    outf = kms.mk_gate_nand_new(ck, xa, xb, fast_boot=True)
    want = ~(a.astype(bool) & b.astype(bool))
    po = O.KmsParams(**{f: getattr(p, f) for f, _ in O.KmsParams._fields_})
    orc = O.KMSOracle(po, K.gsw, K.uni, K.pk, K.crs, K.ksk)
    t0 = time.time()
    with _oracle_threads(O, gates):
        ref = orc.gates(O.NAND, xa[:gates], xb[:gates])
        reff = orc.gates(O.NAND, xa[:gates], xb[:gates], fast_boot=True)
    t_or = time.time() - t0
    rec = dict(check="kms2", workload=f"{batch} mk_gate_nand_new, KMS2 at full size (P={p.parties}, n={p.n}, N={p.N}, gsw {p.l_gsw}/{p.bg_gsw}, lev {p.l_lev}/{p.bg_lev}, uni {p.l_uni}/{p.bg_uni})",
               gates_per_s=batch / dt, seconds=dt, host_keygen_s=t_key, all_decrypt_correct=bool(np.array_equal(K.decrypt(out), want)),
               fast_boot_all_decrypt_correct=bool(np.array_equal(K.decrypt(outf), want)), oracle_gates=gates, oracle_seconds=t_or,
               words_equal_to_oracle=bool(np.array_equal(out[:gates], ref)), fast_boot_words_equal_to_oracle=bool(np.array_equal(outf[:gates], reff)),
               words_compared=int(ref.size) * 2)
    ck.close()
    return rec


def ccs_oracle_check(name, batch, oracle_gates):
    """A CCS set (mk_gate_nand, J/mk_gates.jl:7-13) at its full size, key material from the oracle's key generation: the batch on the GPU, every
    output decrypted, `oracle_gates` gates word for word against the oracle.  Returns the record."""
    import oracle_lib as O
    p = O.make_params(name)
    s = O.SIGMAS[name]
    t0 = time.time()
    K = O.CCSKeys(p, 0x5EED0001, s["bk"], s["ks"])
    t_key = time.time() - t0
    note(f"{name}: keys from the oracle in {t_key:.0f} s")
    ck = thfhe.CCSCloudKey(thfhe.make_params(**p.as_dict()), K.bk, K.pk, K.crs, K.ksk, device=0)
    rng = np.random.default_rng(0)
    a, b = rng.integers(0, 2, batch), rng.integers(0, 2, batch)
    xa, xb = K.encrypt_bits(a, s["lwe"], 1), K.encrypt_bits(b, s["lwe"], 2)
    thfhe.mk_gate_nand(ck, xa[:2], xb[:2])
    t0 = time.time()
    out = thfhe.mk_gate_nand(ck, xa, xb)
    dt = time.time() - t0
    note(f"{name}: {batch} gates in {dt:.2f} s")
    orc = O.CCSOracle(p, K)
    stop = _watch(f"{name}: oracle gate(s) still running")
    t0 = time.time()
    with _oracle_threads(O, oracle_gates):
        ref = orc.gates(O.NAND, xa[:oracle_gates], xb[:oracle_gates])
    t_or = time.time() - t0
    stop.set()
    rec = dict(check=name, workload=f"{batch} mk_gate_nand (CCS), {name} at full size (P={p.parties}, n={p.n}, N={p.N}, l={p.l}, Bgbit={p.Bgbit}), keys from the oracle's key generation",
               gates_per_s=batch / dt, seconds=dt, oracle_keygen_s=t_key, all_decrypt_correct=bool(np.array_equal(K.decrypt_bits(out), ~(a.astype(bool) & b.astype(bool)))),
               oracle_gates=oracle_gates, oracle_seconds=t_or, words_equal_to_oracle=bool(np.array_equal(out[:oracle_gates], ref)), words_compared=int(ref.size))
    ck.close()
    return rec


def kms_check(name, batch, oracle_gates):
    """A KMS set (mk_gate_nand_new) at its full size: batch on the GPU, decrypted; `oracle_gates` gates word for word against the oracle.
    Returns the record."""
    import oracle_lib as O
    from thfhe import kms
    p = thfhe.make_kms_params(name)
    t0 = time.time()
    K = keygen.KMSSecretKeySet(p, seed=1)
    t_key = time.time() - t0
    note(f"{name}: host key generation {t_key:.0f} s")
    ck = kms.KMSCloudKey(p, K.gsw, K.uni, K.pk, K.crs, K.ksk, device=0)
    rng = np.random.default_rng(0)
    a, b = rng.integers(0, 2, batch), rng.integers(0, 2, batch)
    xa, xb = K.encrypt(a, 1), K.encrypt(b, 2)
    kms.mk_gate_nand_new(ck, xa[:2], xb[:2])
    t0 = time.time()
    out = kms.mk_gate_nand_new(ck, xa, xb)
    dt = time.time() - t0
    note(f"{name}: {batch} gates in {dt:.2f} s")
    po = O.KmsParams(**{f: getattr(p, f) for f, _ in O.KmsParams._fields_})
    orc = O.KMSOracle(po, K.gsw, K.uni, K.pk, K.crs, K.ksk)
    stop = _watch(f"{name}: oracle gate(s) still running")
    t0 = time.time()
    with _oracle_threads(O, oracle_gates):
        ref = orc.gates(O.NAND, xa[:oracle_gates], xb[:oracle_gates])
    t_or = time.time() - t0
    stop.set()
    rec = dict(check=name, workload=f"{batch} mk_gate_nand_new, {name} at full size (P={p.parties}, n={p.n}, N={p.N}, gsw {p.l_gsw}/{p.bg_gsw}, lev {p.l_lev}/{p.bg_lev}, uni {p.l_uni}/{p.bg_uni})",
               gates_per_s=batch / dt, seconds=dt, host_keygen_s=t_key, all_decrypt_correct=bool(np.array_equal(K.decrypt(out), ~(a.astype(bool) & b.astype(bool)))),
               oracle_gates=oracle_gates, oracle_seconds=t_or, words_equal_to_oracle=bool(np.array_equal(out[:oracle_gates], ref)), words_compared=int(ref.size))
    ck.close()
    return rec


def ccs16_check(batch=64):
    p = thfhe.make_params("CCS16")
    t0 = time.time()
    K = keygen.CCSSecretKeySet(p)
    t_key = time.time() - t0
    ck = thfhe.CCSCloudKey(p, K.bk, K.pk, K.crs, K.ksk, device=0)
    rng = np.random.default_rng(0)
    a, b = rng.integers(0, 2, batch), rng.integers(0, 2, batch)
    xa, xb = K.encrypt(a, 1), K.encrypt(b, 2)
    thfhe.mk_gate_nand(ck, xa[:2], xb[:2])
    t0 = time.time()
    out = thfhe.mk_gate_nand(ck, xa, xb)
    dt = time.time() - t0
    emit(check="ccs16", workload=f"{batch} mk_gate_nand (CCS), CCS16 at full size (P={p.parties}, n={p.n}, N={p.N}, l={p.l}, Bgbit={p.Bgbit})", gates_per_s=batch / dt, seconds=dt,
         host_keygen_s=t_key, all_decrypt_correct=bool(np.array_equal(K.decrypt(out), ~(a.astype(bool) & b.astype(bool)))))
    ck.close()


def mk_oracle_keys_check(name, batch, oracle_gates):
    """A set whose keys the device key generation cannot make (ring of degree 4096): key material from the ORACLE's key generation (single-threaded C,
    minutes at full size), the batch on the GPU, every output decrypted, `oracle_gates` gates word for word against the oracle."""
    import threading
    import oracle_lib as O
    p = O.make_params(name)
    s = O.SIGMAS[name]
    stop = threading.Event()
    threading.Thread(target=lambda: [note(f"{name}: oracle key generation still running") for _ in iter(lambda: stop.wait(120), True)], daemon=True).start()
    t0 = time.time()
    K = O.MKKeys(p, 0x5EED0001, s["bk"], s["ks"])
    t_key = time.time() - t0
    stop.set()
    note(f"{name}: keys generated by the oracle in {t_key:.0f} s ({K.bk.nbytes / 1e9:.1f} GB + {K.ksk.nbytes / 1e9:.1f} GB)")
    t0 = time.time()
    ck = thfhe.MKCloudKey(thfhe.make_params(name), K.bk, K.ksk, device=0)
    t_ctx = time.time() - t0
    rng = np.random.default_rng(0)
    a, b = rng.integers(0, 2, batch), rng.integers(0, 2, batch)
    xa, xb = K.encrypt_bits(a, s["lwe"], 1), K.encrypt_bits(b, s["lwe"], 2)
    ck.gates(thfhe.NAND, xa[:2], xb[:2])
    t0 = time.time()
    out = ck.gates(thfhe.NAND, xa, xb)
    dt = time.time() - t0
    note(f"{name}: {batch} gates in {dt:.2f} s")
    ok = bool(np.array_equal(K.decrypt_bits(out), ~(a.astype(bool) & b.astype(bool))))
    orc = O.MKOracle(p, K.bk, K.ksk)
    O.lib().oracle_set_threads(min(oracle_gates, O.usable_cpus()))
    stop = threading.Event()
    threading.Thread(target=lambda: [note(f"{name}: oracle gate(s) still running") for _ in iter(lambda: stop.wait(120), True)], daemon=True).start()
    t0 = time.time()
    ref = orc.gates(O.NAND, xa[:oracle_gates], xb[:oracle_gates])
    t_or = time.time() - t0
    stop.set()
    emit(check=name, workload=f"{batch} mk_gate_nand_3gen, {name} at full size (P={p.parties}, n={p.n}, N={p.N}, l={p.l}, Bgbit={p.Bgbit}, ks {p.ks_t}/{p.ks_basebit}), keys from the oracle's key generation",
         kernel=ck.rotation_kernel_name(batch), cmuxes_per_gate=p.parties * p.n, key_coefficients_gb=K.bk.nbytes / 1e9, gates_per_s=batch / dt, seconds=dt,
         oracle_keygen_s=t_key, ctx_create_s=t_ctx, all_decrypt_correct=ok, oracle_gates=oracle_gates, oracle_seconds=t_or,
         words_equal_to_oracle=bool(np.array_equal(out[:oracle_gates], ref)), words_compared=int(ref.size))
    ck.close()


def mk_timing_synthetic(name, batch, parties=None):
    """Timing of a set whose key generation is not available at full size in this tree (the device key-generation products stop at N = 2048 and
    the host path needs hours at N = 4096): key tables of the right SHAPE filled with random words / zeros.  Kernel time does not depend on key
    values; outputs are not checked here (the kernel is compared with the oracle at reduced size in tests/test_gpu_parity_mk.py)."""
    over = dict(parties=parties) if parties else {}
    p = thfhe.make_params(name, **over)
    rng = np.random.default_rng(1)
    t0 = time.time()
    bk = rng.integers(-2**63, 2**63, size=(p.parties, p.n, 4, p.l, p.N), dtype=np.int64)
    ksk = np.zeros((p.parties, p.N, p.ks_t, (1 << p.ks_basebit) - 1, p.n + 1), np.int32)
    t_key = time.time() - t0
    t0 = time.time()
    ck = thfhe.MKCloudKey(p, bk, ksk, device=0)
    t_ctx = time.time() - t0
    x = rng.integers(-2**31, 2**31, size=(batch, p.parties * p.n + 1), dtype=np.int64).astype(np.int32)
    ck.gates(thfhe.NAND, x[:2], x[:2])
    ck.set_profiling(True)
    t0 = time.time()
    ck.gates(thfhe.NAND, x, x)
    dt = time.time() - t0
    tm = ck.last_timings()
    emit(check=name + "-timing", workload=f"{batch} mk_gate_nand_3gen, {name} shape at full size (P={p.parties}, n={p.n}, N={p.N}, l={p.l}, Bgbit={p.Bgbit}, ks {p.ks_t}/{p.ks_basebit}), "
         "SYNTHETIC key tables (random words): timing only", kernel=ck.rotation_kernel_name(batch), cmuxes_per_gate=p.parties * p.n,
         key_coefficients_gb=bk.nbytes / 1e9, ksk_gb=ksk.nbytes / 1e9, gates_per_s=batch / dt, seconds=dt, blind_rotate_ms=tm["blind_rotate_ms"],
         keyswitch_ms=tm["keyswitch_ms"], cmux_per_s=batch * p.parties * p.n / (tm["blind_rotate_ms"] * 1e-3), table_fill_s=t_key, ctx_create_s=t_ctx)
    ck.close()


def mk32_with_lut():
    keys = mk_keys("MK32")
    emit(**mk_check("MK32", 512, 2, keys=keys))
    emit(**mk_lut_check("MK32", 3, 2, (0, 2), keys, pair_threshold=0))
    keys[2].close()


CHECKS = {
    "mk32": lambda: emit(**mk_check("MK32", 512, 2)),
    "mk32-lut": mk32_with_lut,
    "mk64": lambda: emit(**mk_check("MK64", 512, 1)),
    "mk128": lambda: emit(**mk_check("MK128", 512, 1)),
    "mk256": lambda: emit(**mk_check("MK256", 512, 1)),
    "mk256-nooracle": lambda: emit(**mk_check("MK256", 512, 0)),
    "kms2": lambda: emit(**kms2_check()),
    "mk64fft": lambda: mk_timing_synthetic("MK64-fft", 256),
    "mk512": lambda: mk_timing_synthetic("MK512", 256, parties=int(os.environ.get("MK512_PARTIES", "128"))),
    "ccs16": ccs16_check,
    "mk64fft-oracle": lambda: mk_oracle_keys_check("MK64-fft", 64, 1),
    "ccs2-oracle": lambda: emit(**ccs_oracle_check("CCS2", 256, 8)),
    "ccs4-oracle": lambda: emit(**ccs_oracle_check("CCS4", 128, 4)),
    "ccs8-oracle": lambda: emit(**ccs_oracle_check("CCS8", 64, 2)),
    "ccs16-oracle": lambda: emit(**ccs_oracle_check("CCS16", 32, 1)),
    "kms4": lambda: emit(**kms_check("KMS4", 64, 2)),
    "kms8": lambda: emit(**kms_check("KMS8", 32, 1)),
}

if __name__ == "__main__":
    for name in sys.argv[1:] or ["mk32", "kms2"]:
        CHECKS[name]()
