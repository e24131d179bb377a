"""thfhe -- Python host layer over the C ABI of libthfhe_hip.so (include/thfhe_hip.h).

Mirrors the reference's gate/bootstrapping interface for the hot path (3-gen-mk-tfhe/src/gates.jl,
bootstrap.jl, keyswitch.jl, 3gen_mk_gates.jl, 3gen_mk_internals.jl): same function names, argument
order and meaning, with numpy int32 LWE records ([..., n+1] = a..., b) instead of Julia structs.
There is no CPU fallback: importing works anywhere (so the ABI can be inspected), but creating a
context or evaluating a gate without a usable HIP device raises ThfheError.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("THFHE_HIP_LIB", os.path.join(os.path.dirname(_HERE), "lib", "libthfhe_hip.so"))

# gate opcodes (include/thfhe_hip.h enum thfhe_gate)
NAND, OR, AND, XOR, XNOR, NOR, ANDNY, ANDYN, ORNY, ORYN, MUX, NOT, COPY, AND3 = range(14)
LUT, LUT_OUT = 14, 15   # gate-DAG LUT node and its outputs j > 0 (dag_run_lut_batch, dag_run_tree_batch)
LUT_ENC, SELECT, TREE = 16, 17, 18   # gate-DAG encrypted-table, select and tree nodes (CloudKey.dag_run_tree_batch, dag_run_mv_batch)
MV, TREE_MV = 19, 20                 # gate-DAG multi-value and k-output multi-value tree nodes (CloudKey.dag_run_mv_batch, dag_run_lhe_batch; MV: MKCloudKey.dag_run_mv_batch)
LHE_LOOKUP, LHE_GATHER, LHE_WFA = 21, 22, 23   # gate-DAG leveled nodes on TGSW-encrypted bits (CloudKey.dag_run_lhe_batch only)
CB = 24                                        # gate-DAG node: wires -> a computed TGSW set by circuit bootstrapping (CloudKey.dag_run_cb_batch only)
DENSE = 25                                     # gate-DAG node: an encrypted dense layer on K operand wires (CloudKey / MKCloudKey.dag_run_dense_batch only)

MU8 = 1 << 29     # encode_message(1, 8), Torus32      (numeric-functions.jl:86-89)
MU8_64 = 1 << 61  # encode_message64(1, 8), Torus64    (numeric-functions.jl:92-95)


class ThfheError(RuntimeError):
    pass


class Params(C.Structure):
    """thfhe_params (include/thfhe_hip.h)."""
    _fields_ = [(f, C.c_int32) for f in
                ("n", "N", "k", "l", "Bgbit", "ks_t", "ks_basebit", "torus_bits", "parties")]

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


# the reference's parameter tables for this path (api.jl:76-115, src/libthfhe.cpp:316-338, mk_api.jl:32-146)
PARAM_SETS = {
    "SK-80": dict(n=500, N=1024, k=1, l=2, Bgbit=10, ks_t=8, ks_basebit=2, torus_bits=32, parties=1),
    "SK-128": dict(n=630, N=1024, k=1, l=3, Bgbit=7, ks_t=8, ks_basebit=2, torus_bits=32, parties=1),
    "SK-lib": dict(n=1024, N=1024, k=1, l=3, Bgbit=7, ks_t=8, ks_basebit=2, torus_bits=32, parties=1),
    "MK2": dict(n=520, N=1024, k=1, l=2, Bgbit=7, ks_t=3, ks_basebit=3, torus_bits=64, parties=2),
    "MK3": dict(n=510, N=1024, k=1, l=2, Bgbit=7, ks_t=5, ks_basebit=2, torus_bits=64, parties=3),
    "MK4": dict(n=510, N=1024, k=1, l=3, Bgbit=6, ks_t=5, ks_basebit=2, torus_bits=64, parties=4),
    "MK5": dict(n=520, N=1024, k=1, l=3, Bgbit=6, ks_t=5, ks_basebit=2, torus_bits=64, parties=5),   # mk_api.jl:98-104
    "MK8": dict(n=540, N=1024, k=1, l=4, Bgbit=4, ks_t=5, ks_basebit=2, torus_bits=64, parties=8),   # mk_api.jl:140-146
    # BASELINE.json configs[4] wording ("4-party 3-gen MK-TFHE, N=2048 l=3"): the reference's 4-party set on the larger ring
    "MK4-N2048": dict(n=510, N=2048, k=1, l=3, Bgbit=6, ks_t=5, ks_basebit=2, torus_bits=64, parties=4),
    # the 16 .. 128-party 3-gen sets: ring degree 2048, ONE decomposition level with a 24 .. 26-bit base (mk_api.jl:214-220, 246-252, 268-274, 292-298)
    "MK16": dict(n=590, N=2048, k=1, l=1, Bgbit=26, ks_t=4, ks_basebit=3, torus_bits=64, parties=16),
    "MK32": dict(n=620, N=2048, k=1, l=1, Bgbit=26, ks_t=4, ks_basebit=3, torus_bits=64, parties=32),
    "MK64": dict(n=650, N=2048, k=1, l=1, Bgbit=25, ks_t=4, ks_basebit=3, torus_bits=64, parties=64),
    "MK128": dict(n=670, N=2048, k=1, l=1, Bgbit=24, ks_t=5, ks_basebit=3, torus_bits=64, parties=128),
    "MK32-fft": dict(n=680, N=2048, k=1, l=1, Bgbit=25, ks_t=5, ks_basebit=3, torus_bits=64, parties=32),   # mktfhe_parameters_32party_3gen_for_fft, mk_api.jl:255-261
    # 256 parties: TWO levels with an 18-bit base (mk_api.jl:304-310) -> two 9-bit parts per level, eight row parts: the batched N = 2048 rotation
    "MK256": dict(n=740, N=2048, k=1, l=2, Bgbit=18, ks_t=8, ks_basebit=2, torus_bits=64, parties=256),
    # the ring of degree 4096: mktfhe_parameters_64party_3gen_for_fft, mktfhe_parameters_512party_3gen (mk_api.jl:277-283, 316-322); 27-bit base -> three 9-bit parts
    "MK64-fft": dict(n=720, N=4096, k=1, l=1, Bgbit=27, ks_t=5, ks_basebit=3, torus_bits=64, parties=64),
    "MK512": dict(n=730, N=4096, k=1, l=1, Bgbit=27, ks_t=5, ks_basebit=3, torus_bits=64, parties=512),
    # CCS scheme (mk_bootstrap / mk_gate_nand): mktfhe_parameters_2party / _4party, mk_api.jl:4-10,56-62
    "CCS2": dict(n=560, N=1024, k=1, l=3, Bgbit=9, ks_t=8, ks_basebit=2, torus_bits=32, parties=2),
    "CCS4": dict(n=560, N=1024, k=1, l=4, Bgbit=8, ks_t=8, ks_basebit=2, torus_bits=32, parties=4),
    "CCS8": dict(n=560, N=1024, k=1, l=5, Bgbit=6, ks_t=8, ks_basebit=2, torus_bits=32, parties=8),   # mktfhe_parameters_8party, mk_api.jl:111-117
    "CCS16": dict(n=560, N=1024, k=1, l=12, Bgbit=2, ks_t=8, ks_basebit=2, torus_bits=32, parties=16),   # mktfhe_parameters_16party, mk_api.jl:185-191
}


# Noise standard deviations of the reference's parameter sets (lwe = fresh ciphertexts and key-switch key, bk = bootstrapping key):
# api.jl:76-115, mk_api.jl:4-10,32-38,44-50,56-62,84-90,98-104,111-117,140-146,214-220,246-252,268-274,292-298; SK-lib = libthfhe.cpp:316-338.
# MK4-N2048 (BASELINE.json configs[4] wording) inherits the 4-party set's.  Indexed with [] on purpose: an unknown set must raise.
SIGMAS = {
    "SK-80": dict(lwe=2.0**-15, bk=9.0e-9, ks=2.44e-5),
    "SK-128": dict(lwe=2.0**-15, bk=2.0**-25, ks=2.0**-15),
    "SK-lib": dict(lwe=2.0**-15, bk=2.0**-25, ks=2.0**-15),
    "MK2": dict(lwe=2.0**-13.52, bk=2.0**-30.70, ks=2.0**-13.52),
    "MK3": dict(lwe=2.0**-13.26, bk=2.0**-30.70, ks=2.0**-13.26),
    "MK4": dict(lwe=2.0**-13.26, bk=2.0**-30.70, ks=2.0**-13.26),
    "MK5": dict(lwe=2.0**-13.52, bk=2.0**-30.70, ks=2.0**-13.52),
    "MK8": dict(lwe=2.0**-14.04, bk=2.0**-30.70, ks=2.0**-14.04),
    "MK4-N2048": dict(lwe=2.0**-13.26, bk=2.0**-30.70, ks=2.0**-13.26),
    "MK16": dict(lwe=2.0**-15.34, bk=2.0**-62.0, ks=2.0**-15.34),
    "MK32": dict(lwe=2.0**-16.12, bk=2.0**-62.0, ks=2.0**-16.12),
    "MK64": dict(lwe=2.0**-16.90, bk=2.0**-62.0, ks=2.0**-16.90),
    "MK128": dict(lwe=2.0**-17.42, bk=2.0**-62.0, ks=2.0**-17.42),
    "MK32-fft": dict(lwe=2.0**-17.68, bk=2.0**-62.0, ks=2.0**-17.68),
    "MK256": dict(lwe=2.0**-19.24, bk=2.0**-62.0, ks=2.0**-19.24),
    "MK64-fft": dict(lwe=2.0**-18.72, bk=2.0**-62.0, ks=2.0**-18.72),
    "MK512": dict(lwe=2.0**-18.98, bk=2.0**-62.0, ks=2.0**-18.98),
    "CCS2": dict(lwe=3.05e-5, bk=3.72e-9, ks=3.05e-5),
    "CCS4": dict(lwe=3.05e-5, bk=3.72e-9, ks=3.05e-5),
    "CCS8": dict(lwe=3.05e-5, bk=3.72e-9, ks=3.05e-5),
    "CCS16": dict(lwe=3.05e-5, bk=3.72e-9, ks=3.05e-5),
}


# Level-2 sets of circuit bootstrapping: a one-party 3-gen (Torus64) context on the ring of degree 2048 whose LWE key is the gate
# set's (keygen.MKSecretKeySet(..., lwe_keys=...)); l = 2 with an 18-bit base is the shape of MK256, served by the batched N = 2048 rotation.  A table
# of its own: PARAM_SETS is what the tests of the named sets iterate over.  The key-switch fields are MK256's and are not used (the level-2 records
# go to the private key switch).  Made with make_params(**CB_PARAM_SETS[name]).
CB_PARAM_SETS = {
    "CB-128": dict(n=630, N=2048, k=1, l=2, Bgbit=18, ks_t=8, ks_basebit=2, torus_bits=64, parties=1),   # level 2 of SK-128
    "CB-80": dict(n=500, N=2048, k=1, l=2, Bgbit=18, ks_t=8, ks_basebit=2, torus_bits=64, parties=1),    # level 2 of SK-80
}
CB_BATCH_MIN_INPUTS = 3   # kCbBatchMinInputs (csrc/thfhe_cb.h): records per launch from which the private key switch runs on the matrix cores
CB_PER_LEVEL, CB_ONE_ROTATION = 0, 1   # stage A of circuit bootstrapping: l level-2 rotations per bit, or one (include/thfhe_hip.h)
CB_SIGMAS = {
    "CB-128": dict(lwe=2.0**-15, bk=2.0**-62.0, ks=2.0**-15),
    "CB-80": dict(lwe=2.0**-15, bk=2.0**-62.0, ks=2.0**-15),
}


class KmsParams(C.Structure):
    """thfhe_kms_params (include/thfhe_hip.h): the KMS scheme (mk_bootstrap_new) has three gadget families -- gsw (per-party TGSW blind
    rotation of the TLev accumulator), lev (the TLev accumulator), uni (uni-encryption / public keys) -- on a Torus64 ring."""
    _fields_ = [(f, C.c_int32) for f in ("n", "N", "parties", "l_gsw", "bg_gsw", "l_lev", "bg_lev", "l_uni", "bg_uni", "ks_t", "ks_basebit")]

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


# mktfhe_parameters_{2,4,8}party_new and _fast, mk_api.jl:12-30, 64-82, 120-138 (noise: lwe / ks 3.05e-5, gsw / uni 4.63e-18)
KMS_PARAM_SETS = {
    "KMS2": dict(n=560, N=2048, parties=2, l_gsw=3, bg_gsw=13, l_lev=2, bg_lev=7, l_uni=2, bg_uni=13, ks_t=8, ks_basebit=2),
    "KMS2-fast": dict(n=560, N=2048, parties=2, l_gsw=3, bg_gsw=13, l_lev=2, bg_lev=7, l_uni=3, bg_uni=10, ks_t=8, ks_basebit=2),
    "KMS4": dict(n=560, N=2048, parties=4, l_gsw=5, bg_gsw=8, l_lev=2, bg_lev=8, l_uni=5, bg_uni=8, ks_t=8, ks_basebit=2),
    "KMS8": dict(n=560, N=2048, parties=8, l_gsw=4, bg_gsw=11, l_lev=3, bg_lev=6, l_uni=8, bg_uni=4, ks_t=8, ks_basebit=2),
    "KMS16": dict(n=560, N=2048, parties=16, l_gsw=5, bg_gsw=9, l_lev=3, bg_lev=6, l_uni=9, bg_uni=4, ks_t=8, ks_basebit=2),    # mk_api.jl:194-202
    "KMS32": dict(n=560, N=2048, parties=32, l_gsw=6, bg_gsw=8, l_lev=3, bg_lev=7, l_uni=16, bg_uni=2, ks_t=8, ks_basebit=2),   # mk_api.jl:225-233
    # the `_fast` twins (mk_api.jl:74-82, 130-138, 204-212, 235-243): other uni-encryption gadgets, same rotation; the 32-party one equals `_new`
    "KMS4-fast": dict(n=560, N=2048, parties=4, l_gsw=5, bg_gsw=8, l_lev=2, bg_lev=8, l_uni=7, bg_uni=6, ks_t=8, ks_basebit=2),
    "KMS8-fast": dict(n=560, N=2048, parties=8, l_gsw=4, bg_gsw=11, l_lev=3, bg_lev=6, l_uni=7, bg_uni=4, ks_t=8, ks_basebit=2),
    "KMS16-fast": dict(n=560, N=2048, parties=16, l_gsw=5, bg_gsw=9, l_lev=3, bg_lev=6, l_uni=7, bg_uni=4, ks_t=8, ks_basebit=2),
    "KMS32-fast": dict(n=560, N=2048, parties=32, l_gsw=6, bg_gsw=8, l_lev=3, bg_lev=7, l_uni=16, bg_uni=2, ks_t=8, ks_basebit=2),
}


def make_kms_params(name=None, **kw):
    d = dict(KMS_PARAM_SETS[name]) if name else {}
    d.update(kw)
    return KmsParams(**d)


def make_params(name=None, **kw):
    d = dict(PARAM_SETS[name]) if name else {}
    d.update(kw)
    return Params(**d)


class LutSpec(C.Structure):
    """thfhe_lut_spec (include/thfhe_hip.h): prologue x = sum w_q in_q + (0, bias) over n_inputs inputs, theta outputs per rotation."""
    _fields_ = [("n_inputs", C.c_int32), ("weights", C.c_int32 * 3), ("bias", C.c_int32), ("theta", C.c_int32)]


class TreeSpec(C.Structure):
    """thfhe_tree_spec (include/thfhe_hip.h): the `lo` (level 1, TREE nodes only) and `hi` (selection rotation) prologues and the digit modulus p_hi
    of the SELECT / TREE nodes of one launch group."""
    _fields_ = [("lo", LutSpec), ("hi", LutSpec), ("p_hi", C.c_int32)]


class MvSpec(C.Structure):
    """thfhe_mv_spec (include/thfhe_hip.h): the prologues, shape (p taps, q outputs or p_hi, k tables per node), base vector and factor tables of the
    MV / TREE_MV nodes of one launch group."""
    _fields_ = [("lo", LutSpec), ("hi", LutSpec)] + [(f, C.c_int32) for f in ("p", "q", "k", "base", "factors_off", "n_tables")]


class DagLheSpec(C.Structure):
    """thfhe_dag_lhe_spec (include/thfhe_hip.h): the set and shape (d_tree, d_rot, theta) of the LHE_LOOKUP / LHE_GATHER nodes of one launch group."""
    _fields_ = [(f, C.c_int32) for f in ("set", "d_tree", "d_rot", "theta")]


class DagWfaSpec(C.Structure):
    """thfhe_dag_wfa_spec (include/thfhe_hip.h): the shape, sets and word-pool slices of the LHE_WFA nodes of one launch group."""
    _fields_ = [(f, C.c_int32) for f in ("n_steps", "n_states", "theta", "n_out", "set0", "n_sets", "trans_off", "step_off", "start_off")]


class DagLheFamilies(C.Structure):
    """thfhe_dag_lhe_families (include/thfhe_hip.h)."""
    _fields_ = [("sets", C.POINTER(C.c_void_p)), ("n_sets", C.c_int32), ("lks", C.POINTER(DagLheSpec)), ("n_lks", C.c_int32),
                ("tab_a", C.POINTER(C.c_int32)), ("tab_b", C.POINTER(C.c_int32)), ("n_tab_rows", C.c_int32),
                ("wfas", C.POINTER(DagWfaSpec)), ("n_wfas", C.c_int32), ("wfa_words", C.POINTER(C.c_int32)), ("n_wfa_words", C.c_size_t),
                ("fin_a", C.POINTER(C.c_int32)), ("fin_b", C.POINTER(C.c_int32)), ("n_fin_rows", C.c_int32)]


class DagCbSpec(C.Structure):
    """thfhe_dag_cb_spec (include/thfhe_hip.h): the bits of one computed set and its slice of the wire pool."""
    _fields_ = [("d", C.c_int32), ("wire_off", C.c_int32)]


class DagCbFamilies(C.Structure):
    """thfhe_dag_cb_families (include/thfhe_hip.h)."""
    _fields_ = [("sets", C.POINTER(DagCbSpec)), ("n_sets", C.c_int32), ("cb_wires", C.POINTER(C.c_int32)), ("n_cb_wires", C.c_size_t),
                ("mode", C.c_int32), ("words", C.POINTER(C.POINTER(C.c_int32)))]


class DagDenseSpec(C.Structure):
    """thfhe_dag_dense_spec (include/thfhe_hip.h): the shape of one dense layer and its slices of the word pool (bias_off / lut_off -1: none)."""
    _fields_ = [(f, C.c_int32) for f in ("M", "K", "theta", "w_off", "bias_off", "lut_off")]


class DagDenseFamilies(C.Structure):
    """thfhe_dag_dense_families (include/thfhe_hip.h)."""
    _fields_ = [("layers", C.POINTER(DagDenseSpec)), ("n_layers", C.c_int32), ("words", C.POINTER(C.c_int32)), ("n_words", C.c_size_t),
                ("wires", C.POINTER(C.c_int32)), ("n_wires", C.c_size_t)]


def _dense_families(layers, words, wires):
    """(DagDenseFamilies or None, the arrays it points into) from DagDenseSpec or (M, K, theta, w_off, bias_off, lut_off) tuples, the word pool and
    the pool of operand wire ids; None without any of the three."""
    if not len(layers) and words is None and wires is None:
        return None, ()
    ls = (DagDenseSpec * len(layers))(*[l if isinstance(l, DagDenseSpec) else DagDenseSpec(*[int(v) for v in l]) for l in layers]) if len(layers) else None
    w = None if words is None else np.ascontiguousarray(words, np.int32).reshape(-1)
    pool = None if wires is None else np.ascontiguousarray(wires, np.int32).reshape(-1)
    fam = DagDenseFamilies(ls, len(layers), _p32(w), 0 if w is None else w.shape[0], _p32(pool), 0 if pool is None else pool.shape[0])
    return fam, (ls, w, pool)


def _lut_spec(s):
    """LutSpec from a (n_inputs, (w0, w1, w2), bias, theta) tuple (or a LutSpec)."""
    if isinstance(s, LutSpec):
        return s
    return LutSpec(int(s[0]), (C.c_int32 * 3)(*[_wrap32(w) for w in (list(s[1]) + [0, 0, 0])[:3]]), _wrap32(s[2]), int(s[3]))



_NO_SPEC = (1, (0, 0, 0), 0, 1)   # stands for the half of a TreeSpec / MvSpec that its rows do not use


def _mv_specs(mvs):
    """MvSpec array from MvSpec or (lo, hi, p, q, k, base, factors_off, n_tables) tuples (hi may be None: MV only); None without any."""
    if not len(mvs):
        return None
    return (MvSpec * len(mvs))(*[m if isinstance(m, MvSpec) else MvSpec(_lut_spec(m[0]), _lut_spec(m[1] or _NO_SPEC), *[int(v) for v in m[2:]]) for m in mvs])

_lib = None

_i32p = C.POINTER(C.c_int32)
_i64p = C.POINTER(C.c_int64)
_vp = C.c_void_p

# symbol -> (restype, argtypes); tests/test_abi.py checks every symbol declared in include/*.h is exported
SIGNATURES = {
    "thfhe_last_error": (C.c_char_p, []),
    "thfhe_device_count": (C.c_int, []),
    "thfhe_device_pci_bus_id": (C.c_int, [C.c_int, C.c_char_p, C.c_int]),
    "thfhe_ctx_create": (C.c_int, [C.POINTER(Params), _i32p, _i32p, C.c_int, C.POINTER(_vp)]),
    "thfhe_ctx_destroy": (None, [_vp]),
    "thfhe_ctx_params": (C.c_int, [_vp, C.POINTER(Params)]),
    "thfhe_gates": (C.c_int, [_vp, C.c_int, _i32p, _i32p, _i32p, _i32p, C.c_size_t]),
    "thfhe_gates_mixed": (C.c_int, [_vp, _i32p, _i32p, _i32p, _i32p, C.c_size_t]),
    "thfhe_dag_run": (C.c_int, [_vp, _i32p, C.c_size_t, _i32p, C.c_size_t, _i64p]),
    "thfhe_set_dag_slice": (C.c_int, [_vp, C.c_size_t]),
    "thfhe_mk_set_dag_slice": (C.c_int, [_vp, C.c_size_t]),
    "thfhe_dag_run_batch": (C.c_int, [_vp, _i32p, C.c_size_t, _i32p, C.c_size_t, C.c_size_t, _i32p, C.c_size_t, _i32p, _i64p]),
    "thfhe_dag_run_lut_batch": (C.c_int, [_vp, _i32p, C.c_size_t, _i32p, C.c_size_t, C.POINTER(LutSpec), C.c_int, _i32p, C.c_int, C.c_size_t, _i32p,
                                          C.c_size_t, _i32p, _i64p]),
    "thfhe_dag_run_tree_batch": (C.c_int, [_vp, _vp, _i32p, C.c_size_t, _i32p, C.c_size_t, C.POINTER(LutSpec), C.c_int, _i32p, C.c_int, _i32p, _i32p, C.c_int,
                                           C.POINTER(TreeSpec), C.c_int, _i32p, C.c_int, C.c_size_t, _i32p, C.c_size_t, _i32p, _i64p]),
    "thfhe_dag_run_mv_batch": (C.c_int, [_vp, _vp, _i32p, C.c_size_t, _i32p, C.c_size_t, C.POINTER(LutSpec), C.c_int, _i32p, C.c_int, _i32p, _i32p, C.c_int,
                                         C.POINTER(TreeSpec), C.c_int, _i32p, C.c_int, C.POINTER(MvSpec), C.c_int, _i32p, C.c_int, _i32p, C.c_size_t,
                                         C.c_size_t, _i32p, C.c_size_t, _i32p, _i64p]),
    "thfhe_dag_run_lhe_batch": (C.c_int, [_vp, _vp, _i32p, C.c_size_t, _i32p, C.c_size_t, C.POINTER(LutSpec), C.c_int, _i32p, C.c_int, _i32p, _i32p, C.c_int,
                                          C.POINTER(TreeSpec), C.c_int, _i32p, C.c_int, C.POINTER(MvSpec), C.c_int, _i32p, C.c_int, _i32p, C.c_size_t,
                                          C.POINTER(DagLheFamilies), C.c_size_t, _i32p, C.c_size_t, _i32p, _i64p]),
    "thfhe_dag_last_group_ms": (C.c_int, [_vp, C.POINTER(C.c_float)]),
    "thfhe_dag_last_stage_ms": (C.c_int, [_vp, C.POINTER(C.c_float)]),
    "thfhe_dag_run_cb_batch": (C.c_int, [_vp, _vp, _vp, _i32p, C.c_size_t, _i32p, C.c_size_t, C.POINTER(LutSpec), C.c_int, _i32p, C.c_int, _i32p, _i32p, C.c_int,
                                         C.POINTER(TreeSpec), C.c_int, _i32p, C.c_int, C.POINTER(MvSpec), C.c_int, _i32p, C.c_int, _i32p, C.c_size_t,
                                         C.POINTER(DagLheFamilies), C.POINTER(DagCbFamilies), C.c_size_t, _i32p, C.c_size_t, _i32p, _i64p]),
    "thfhe_dag_run_dense_batch": (C.c_int, [_vp, _vp, _vp, _i32p, C.c_size_t, _i32p, C.c_size_t, C.POINTER(LutSpec), C.c_int, _i32p, C.c_int, _i32p, _i32p, C.c_int,
                                            C.POINTER(TreeSpec), C.c_int, _i32p, C.c_int, C.POINTER(MvSpec), C.c_int, _i32p, C.c_int, _i32p, C.c_size_t,
                                            C.POINTER(DagLheFamilies), C.POINTER(DagCbFamilies), C.POINTER(DagDenseFamilies), C.c_size_t, _i32p, C.c_size_t, _i32p,
                                            _i64p]),
    "thfhe_dag_cb_release": (C.c_int, [_vp]),
    "thfhe_bootstrap": (C.c_int, [_vp, C.c_int32, _i32p, _i32p, C.c_size_t]),
    "thfhe_bootstrap_wo_keyswitch": (C.c_int, [_vp, C.c_int32, _i32p, _i32p, C.c_size_t]),
    "thfhe_keyswitch": (C.c_int, [_vp, _i32p, _i32p, C.c_size_t]),
    "thfhe_lut_bootstrap": (C.c_int, [_vp, C.POINTER(LutSpec), _i32p, C.c_int, _i32p, _i32p, _i32p, _i32p, _i32p, C.c_size_t]),
    "thfhe_lut_bootstrap_wo_keyswitch": (C.c_int, [_vp, C.POINTER(LutSpec), _i32p, C.c_int, _i32p, _i32p, _i32p, _i32p, _i32p, C.c_size_t]),
    "thfhe_lut_bootstrap_enc": (C.c_int, [_vp, C.POINTER(LutSpec), _i32p, _i32p, C.c_int, _i32p, _i32p, _i32p, _i32p, _i32p, C.c_size_t]),
    "thfhe_lut_bootstrap_enc_wo_keyswitch": (C.c_int, [_vp, C.POINTER(LutSpec), _i32p, _i32p, C.c_int, _i32p, _i32p, _i32p, _i32p, _i32p, C.c_size_t]),
    "thfhe_tree_lut_bootstrap": (C.c_int, [_vp, _vp, C.POINTER(LutSpec), C.POINTER(LutSpec), C.c_int, _i32p, C.c_int, _i32p, _i32p, _i32p, _i32p, _i32p,
                                           _i32p, _i32p, _i32p, C.c_size_t]),
    "thfhe_set_tree_slice": (C.c_int, [_vp, C.c_size_t]),
    "thfhe_mv_lut_bootstrap": (C.c_int, [_vp, C.POINTER(LutSpec), _i32p, _i32p, C.c_int, C.c_int, C.c_int, _i32p, _i32p, _i32p, _i32p, _i32p, C.c_size_t]),
    "thfhe_mv_lut_bootstrap_wo_keyswitch": (C.c_int, [_vp, C.POINTER(LutSpec), _i32p, _i32p, C.c_int, C.c_int, C.c_int, _i32p, _i32p, _i32p, _i32p, _i32p,
                                                      C.c_size_t]),
    "thfhe_tree_lut_bootstrap_mv": (C.c_int, [_vp, _vp, C.POINTER(LutSpec), C.POINTER(LutSpec), C.c_int, C.c_int, _i32p, _i32p, C.c_int, _i32p, _i32p, _i32p,
                                              _i32p, _i32p, _i32p, _i32p, _i32p, C.c_size_t]),
    "thfhe_tree_lut_bootstrap_mvk": (C.c_int, [_vp, _vp, C.POINTER(LutSpec), C.POINTER(LutSpec), C.c_int, C.c_int, C.c_int, _i32p, _i32p, C.c_int, _i32p, _i32p,
                                               _i32p, _i32p, _i32p, _i32p, _i32p, _i32p, C.c_size_t]),
    "thfhe_tgsw_set_create": (C.c_int, [_vp, _i32p, C.c_size_t, C.c_int, C.POINTER(_vp)]),
    "thfhe_tgsw_set_destroy": (None, [_vp]),
    "thfhe_lhe_cmux": (C.c_int, [_vp, _vp, C.c_int, _i32p, _i32p, _i32p, _i32p, _i32p, _i32p, C.c_size_t]),
    "thfhe_lhe_lookup": (C.c_int, [_vp, _vp, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_int, _i32p, _i32p, C.c_int, _i32p, _i32p]),
    "thfhe_lhe_lookup_wo_keyswitch": (C.c_int, [_vp, _vp, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_int, _i32p, _i32p, C.c_int, _i32p, _i32p]),
    "thfhe_lhe_demux": (C.c_int, [_vp, _vp, C.c_int, _i32p, _i32p, _i32p, _i32p, _i32p, _i32p, C.c_size_t]),
    "thfhe_lhe_scatter": (C.c_int, [_vp, _vp, C.c_size_t, C.c_size_t, C.c_int, C.c_int, _i32p, _i32p, C.c_int, _i32p, C.c_int, _i32p, _i32p, _i32p]),
    "thfhe_lhe_wfa": (C.c_int, [_vp, C.POINTER(_vp), C.c_int, C.c_size_t, C.c_size_t, C.c_int, C.c_int, _i32p, _i32p, _i32p, _i32p, C.c_int, _i32p, C.c_int,
                                _i32p, C.c_int, _i32p]),
    "thfhe_lhe_wfa_wo_keyswitch": (C.c_int, [_vp, C.POINTER(_vp), C.c_int, C.c_size_t, C.c_size_t, C.c_int, C.c_int, _i32p, _i32p, _i32p, _i32p, C.c_int, _i32p,
                                             C.c_int, _i32p, C.c_int, _i32p]),
    "thfhe_set_wfa_chunk": (C.c_int, [_vp, C.c_int]),
    "thfhe_dev_alloc": (_vp, [_vp, C.c_size_t]),
    "thfhe_dev_free": (None, [_vp, _vp]),
    "thfhe_copy_h2d": (C.c_int, [_vp, _vp, _vp, C.c_size_t]),
    "thfhe_copy_d2h": (C.c_int, [_vp, _vp, _vp, C.c_size_t]),
    "thfhe_reserve": (C.c_int, [_vp, C.c_size_t]),
    "thfhe_gates_dev": (C.c_int, [_vp, C.c_int, _vp, _vp, _vp, _vp, C.c_size_t]),
    "thfhe_sync": (C.c_int, [_vp]),
    "thfhe_set_coop_threshold": (C.c_int, [_vp, C.c_int]),
    "thfhe_set_ring4_threshold": (C.c_int, [_vp, C.c_int]),
    "thfhe_rotation_kernel_name": (C.c_int, [_vp, C.c_size_t, C.c_char_p, C.c_int]),
    "thfhe_mk_rotation_kernel_name": (C.c_int, [_vp, C.c_size_t, C.c_char_p, C.c_int]),
    "thfhe_kms_rotation_kernel_name": (C.c_int, [_vp, C.c_size_t, C.c_char_p, C.c_int]),
    "thfhe_ccs_rotation_kernel_name": (C.c_int, [_vp, C.c_char_p, C.c_int]),
    "thfhe_set_profiling": (C.c_int, [_vp, C.c_int]),
    "thfhe_last_timings": (C.c_int, [_vp, C.POINTER(C.c_float)]),
    "thfhe_ccs_ctx_create": (C.c_int, [C.POINTER(Params), _i32p, _i32p, _i32p, _i32p, C.c_int, C.POINTER(_vp)]),
    "thfhe_ccs_ctx_destroy": (None, [_vp]),
    "thfhe_ccs_gates": (C.c_int, [_vp, C.c_int, _i32p, _i32p, _i32p, C.c_size_t]),
    "thfhe_ccs_bootstrap": (C.c_int, [_vp, C.c_int32, _i32p, _i32p, C.c_size_t]),
    "thfhe_poly_ctx_create": (C.c_int, [C.c_int, C.c_int, C.POINTER(_vp)]),
    "thfhe_poly_ctx_destroy": (None, [_vp]),
    "thfhe_tlwe_from_lwe": (C.c_int, [_vp, _i32p, _i32p, _i32p, C.c_size_t]),
    "thfhe_partial_decrypt": (C.c_int, [_vp, _i32p, _i32p, _i32p, _i32p, C.c_size_t]),
    "thfhe_final_decrypt": (C.c_int, [_vp, _i32p, _i32p, C.c_int, _i32p, _i32p, C.c_size_t]),
    "thfhe_pack_key_set": (C.c_int, [_vp, _i32p, C.c_int, C.c_int, C.c_int]),
    "thfhe_pack_lwe": (C.c_int, [_vp, _i32p, C.c_size_t, C.c_int, _i32p, _i32p]),
    "thfhe_pack_boxes": (C.c_int, [_vp, _i32p, C.c_size_t, C.c_int, _i32p, _i32p]),
    "thfhe_kms_ctx_create": (C.c_int, [_vp, _i64p, _i32p, C.c_int, C.POINTER(_vp)]),
    "thfhe_kms_ctx_destroy": (None, [_vp]),
    "thfhe_kms_tlev_rotate": (C.c_int, [_vp, C.c_int, _i32p, _i64p, C.c_size_t]),
    "thfhe_kms_rlwe_rotate": (C.c_int, [_vp, C.c_int, _i32p, _i64p, C.c_size_t]),
    "thfhe_kms_set_relin_keys": (C.c_int, [_vp, _i64p, _i64p, _i64p]),
    "thfhe_kms_lev_rlwe_mul": (C.c_int, [_vp, C.c_int, _i64p, _i64p, C.c_size_t]),
    "thfhe_kms_bootstrap": (C.c_int, [_vp, C.c_int64, _i32p, _i32p, _i32p, C.c_size_t, C.c_int]),
    "thfhe_kms_gates": (C.c_int, [_vp, C.c_int, _i32p, _i32p, _i32p, C.c_size_t, C.c_int]),
    "thfhe_kms_rotate_parties_dev": (C.c_int, [_vp, C.c_int, _vp, _vp, C.c_int, C.c_int, _vp, C.c_size_t]),
    "thfhe_kms_finish_dev": (C.c_int, [_vp, C.c_int, _vp, _vp, _vp, _vp, C.c_size_t]),
    "thfhe_kms_set_stream": (C.c_int, [_vp, _vp]),
    "thfhe_kms_set_pair_threshold": (C.c_int, [_vp, C.c_long]),
    "thfhe_kms_keyswitch": (C.c_int, [_vp, _i32p, _i32p, C.c_size_t]),
    "thfhe_pm_ctx_create": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(_vp)]),
    "thfhe_pm_ctx_destroy": (None, [_vp]),
    "thfhe_pm_mac": (C.c_int, [_vp, _i32p, C.c_size_t, _vp, C.c_size_t, _i32p, C.c_size_t, _vp, _vp, C.c_size_t]),
    "thfhe_mk_ctx_create": (C.c_int, [C.POINTER(Params), _i64p, _i32p, C.c_int, C.POINTER(_vp)]),
    "thfhe_mk_ctx_destroy": (None, [_vp]),
    "thfhe_mk_ctx_info": (C.c_int, [_vp, C.POINTER(Params), C.POINTER(C.c_int)]),
    "thfhe_cb_key_set": (C.c_int, [_vp, _i32p, C.c_int, C.c_int, C.c_int]),
    "thfhe_cb_private_keyswitch": (C.c_int, [_vp, _i32p, C.c_size_t, _i32p]),
    "thfhe_cb_set_batch_threshold": (C.c_int, [_vp, C.c_long]),
    "thfhe_circuit_bootstrap": (C.c_int, [_vp, _vp, _i32p, C.c_size_t, C.c_int, _i32p, C.POINTER(_vp)]),
    "thfhe_circuit_bootstrap_mode": (C.c_int, [_vp, _vp, _i32p, C.c_size_t, C.c_int, C.c_int, _i32p, C.POINTER(_vp)]),
    "thfhe_cb_stage_a": (C.c_int, [_vp, _vp, _i32p, C.c_size_t, C.c_int, _i32p]),
    "thfhe_mk_gates": (C.c_int, [_vp, C.c_int, _i32p, _i32p, _i32p, _i32p, C.c_size_t]),
    "thfhe_mk_gates_mixed": (C.c_int, [_vp, _i32p, _i32p, _i32p, _i32p, C.c_size_t]),
    "thfhe_mk_dag_run": (C.c_int, [_vp, _i32p, C.c_size_t, _i32p, C.c_size_t, _i64p]),
    "thfhe_mk_dag_run_batch": (C.c_int, [_vp, _i32p, C.c_size_t, _i32p, C.c_size_t, C.c_size_t, _i32p, C.c_size_t, _i32p, _i64p]),
    "thfhe_mk_dag_run_lut_batch": (C.c_int, [_vp, _i32p, C.c_size_t, _i32p, C.c_size_t, C.POINTER(LutSpec), C.c_int, _i64p, C.c_int, C.c_size_t,
                                             _i32p, C.c_size_t, _i32p, _i64p]),
    "thfhe_mk_bootstrap": (C.c_int, [_vp, C.c_int64, _i32p, _i32p, C.c_size_t]),
    "thfhe_mk_lut_bootstrap": (C.c_int, [_vp, C.POINTER(LutSpec), _i64p, C.c_int, _i32p, _i32p, _i32p, _i32p, _i32p, C.c_size_t]),
    "thfhe_mk_lut_bootstrap_wo_keyswitch": (C.c_int, [_vp, C.POINTER(LutSpec), _i64p, C.c_int, _i32p, _i32p, _i32p, _i32p, _i32p, C.c_size_t]),
    "thfhe_mk_mv_lut_bootstrap": (C.c_int, [_vp, C.POINTER(LutSpec), _i64p, _i32p, C.c_int, C.c_int, C.c_int, _i32p, C.c_int64, _i32p, _i32p, _i32p, _i32p,
                                            C.c_size_t]),
    "thfhe_mk_mv_lut_bootstrap_wo_keyswitch": (C.c_int, [_vp, C.POINTER(LutSpec), _i64p, _i32p, C.c_int, C.c_int, C.c_int, _i32p, C.c_int64, _i32p, _i32p, _i32p,
                                                         _i32p, C.c_size_t]),
    "thfhe_mk_set_mv_slice": (C.c_int, [_vp, C.c_size_t]),
    "thfhe_mk_pack_key_set": (C.c_int, [_vp, _i64p, C.c_int, C.c_int, C.c_int]),
    "thfhe_mk_pack_boxes": (C.c_int, [_vp, _i32p, C.c_size_t, C.c_int, _i64p, _i64p]),
    "thfhe_mk_lut_bootstrap_enc": (C.c_int, [_vp, C.POINTER(LutSpec), _i64p, _i64p, C.c_int, _i32p, _i32p, _i32p, _i32p, _i32p, C.c_size_t]),
    "thfhe_mk_lut_bootstrap_enc_wo_keyswitch": (C.c_int, [_vp, C.POINTER(LutSpec), _i64p, _i64p, C.c_int, _i32p, _i32p, _i32p, _i32p, _i32p, C.c_size_t]),
    "thfhe_mk_tree_lut_bootstrap": (C.c_int, [_vp, C.POINTER(LutSpec), C.POINTER(LutSpec), C.c_int, _i64p, C.c_int, _i32p, _i32p, _i32p, _i32p, _i32p, _i32p,
                                              _i32p, _i32p, C.c_size_t]),
    "thfhe_mk_set_tree_slice": (C.c_int, [_vp, C.c_size_t]),
    "thfhe_mk_tgsw_set_create": (C.c_int, [_vp, _i64p, C.c_size_t, C.c_int, C.POINTER(_vp)]),
    "thfhe_mk_tgsw_set_destroy": (None, [_vp]),
    "thfhe_mk_lhe_cmux": (C.c_int, [_vp, _vp, C.c_int, _i64p, _i64p, _i64p, _i64p, _i64p, _i64p, C.c_size_t]),
    "thfhe_mk_lhe_lookup": (C.c_int, [_vp, _vp, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_int, _i64p, _i64p, C.c_int, _i32p, _i32p]),
    "thfhe_mk_lhe_lookup_wo_keyswitch": (C.c_int, [_vp, _vp, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_int, _i64p, _i64p, C.c_int, _i32p, _i32p]),
    "thfhe_lwe_linear": (C.c_int, [_vp, _i32p, _i32p, C.c_int, C.c_int, _i32p, _i32p, C.c_size_t]),
    "thfhe_linear_lut_bootstrap": (C.c_int, [_vp, _i32p, _i32p, C.c_int, C.c_int, C.c_int, _i32p, C.c_int, _i32p, _i32p, _i32p, C.c_size_t]),
    "thfhe_linear_lut_bootstrap_wo_keyswitch": (C.c_int, [_vp, _i32p, _i32p, C.c_int, C.c_int, C.c_int, _i32p, C.c_int, _i32p, _i32p, _i32p, C.c_size_t]),
    "thfhe_set_linear_slice": (C.c_int, [_vp, C.c_size_t]),
    "thfhe_linear_last_timings": (C.c_int, [_vp, C.POINTER(C.c_float)]),
    "thfhe_linear_tile": (C.c_int, [C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "thfhe_mk_lwe_linear": (C.c_int, [_vp, _i32p, _i32p, C.c_int, C.c_int, _i32p, _i32p, C.c_size_t]),
    "thfhe_mk_linear_lut_bootstrap": (C.c_int, [_vp, _i32p, _i32p, C.c_int, C.c_int, C.c_int, _i64p, C.c_int, _i32p, _i32p, _i32p, C.c_size_t]),
    "thfhe_mk_linear_lut_bootstrap_wo_keyswitch": (C.c_int, [_vp, _i32p, _i32p, C.c_int, C.c_int, C.c_int, _i64p, C.c_int, _i32p, _i32p, _i32p, C.c_size_t]),
    "thfhe_mk_set_linear_slice": (C.c_int, [_vp, C.c_size_t]),
    "thfhe_mk_linear_last_timings": (C.c_int, [_vp, C.POINTER(C.c_float)]),
    "thfhe_mk_tree_lut_bootstrap_mvk": (C.c_int, [_vp, C.POINTER(LutSpec), C.POINTER(LutSpec), C.c_int, C.c_int, C.c_int, _i64p, _i32p, C.c_int, _i32p, C.c_int64,
                                                  _i32p, _i32p, _i32p, _i32p, _i32p, _i32p, _i32p, C.c_size_t]),
    "thfhe_mk_set_pack_wide_threshold": (C.c_int, [_vp, C.c_size_t]),
    "thfhe_mk_pack_kernel_name": (C.c_int, [_vp, C.c_size_t, C.c_char_p, C.c_int]),
    "thfhe_mk_dag_run_mv_batch": (C.c_int, [_vp, _i32p, C.c_size_t, _i32p, C.c_size_t, C.POINTER(LutSpec), C.c_int, _i64p, C.c_int, C.POINTER(MvSpec), C.c_int,
                                            _i64p, C.c_int, _i32p, C.c_size_t, _i64p, C.c_size_t, _i32p, C.c_size_t, _i32p, _i64p]),
    "thfhe_mk_dag_run_tree_batch": (C.c_int, [_vp, _i32p, C.c_size_t, _i32p, C.c_size_t, C.POINTER(LutSpec), C.c_int, _i64p, C.c_int, _i64p, _i64p, C.c_int,
                                              C.POINTER(TreeSpec), C.c_int, _i64p, C.c_int, C.POINTER(MvSpec), C.c_int, _i64p, C.c_int, _i32p, C.c_size_t, _i64p,
                                              C.c_size_t, _i32p, C.c_size_t, _i32p, _i64p]),
    "thfhe_mk_dag_run_dense_batch": (C.c_int, [_vp, _i32p, C.c_size_t, _i32p, C.c_size_t, C.POINTER(LutSpec), C.c_int, _i64p, C.c_int, _i64p, _i64p, C.c_int,
                                               C.POINTER(TreeSpec), C.c_int, _i64p, C.c_int, C.POINTER(MvSpec), C.c_int, _i64p, C.c_int, _i32p, C.c_size_t, _i64p,
                                               C.POINTER(DagDenseFamilies), C.c_size_t, _i32p, C.c_size_t, _i32p, _i64p]),
    "thfhe_mk_prologue_dev": (C.c_int, [_vp, C.c_int, C.c_int, _vp, _vp, _vp, C.c_int, C.c_int, _vp, _vp, C.c_size_t]),
    "thfhe_mk_set_stream": (C.c_int, [_vp, _vp]),
    "thfhe_mk_set_pair_threshold": (C.c_int, [_vp, C.c_long]),
    "thfhe_mk_rotate_partial_dev": (C.c_int, [_vp, _vp, _vp, C.c_int64, _vp, _vp, C.c_size_t]),
    "thfhe_mk_extract_dev": (C.c_int, [_vp, _vp, _vp, C.c_size_t]),
    "thfhe_mk_lut_rotate_dev": (C.c_int, [_vp, _vp, C.c_int, _vp, _vp, C.c_size_t]),
    "thfhe_mk_keyswitch_dev": (C.c_int, [_vp, _vp, _vp, C.c_size_t]),
    "thfhe_mk_dev_alloc": (_vp, [_vp, C.c_size_t]),
    "thfhe_mk_dev_free": (None, [_vp, _vp]),
    "thfhe_mk_copy_h2d": (C.c_int, [_vp, _vp, _vp, C.c_size_t]),
    "thfhe_mk_copy_d2h": (C.c_int, [_vp, _vp, _vp, C.c_size_t]),
    "thfhe_mk_reserve": (C.c_int, [_vp, C.c_size_t]),
    "thfhe_mk_gates_dev": (C.c_int, [_vp, C.c_int, _vp, _vp, _vp, _vp, C.c_size_t]),
    "thfhe_mk_sync": (C.c_int, [_vp]),
    "thfhe_mk_set_profiling": (C.c_int, [_vp, C.c_int]),
    "thfhe_mk_last_timings": (C.c_int, [_vp, C.POINTER(C.c_float)]),
}


torch_loaded_first = None  # set by lib(): whether torch's HIP runtime was already in the process when the engine was loaded


def _needs_torch_first():
    """Multi-rank jobs run under torch.distributed (RCCL).  torch bundles its own HIP runtime; if libthfhe_hip.so (rpath
    /opt/rocm/lib) is loaded BEFORE torch, torch's later-loaded runtime sees no GPU.  So in a multi-rank job -- or whenever the
    caller asks with THFHE_TORCH_FIRST=1 -- torch is imported first, and both share torch's runtime."""
    import importlib.util
    import sys
    if "torch" in sys.modules:
        return False
    want = os.environ.get("THFHE_TORCH_FIRST")
    if want is None:
        want = "1" if int(os.environ.get("WORLD_SIZE", "1") or 1) > 1 else "0"
    return want == "1" and importlib.util.find_spec("torch") is not None


def lib():
    """Load libthfhe_hip.so (built in-tree by __graft_entry__.build()); fail loudly if it is missing."""
    global _lib, torch_loaded_first
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ThfheError(f"{LIB_PATH} not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                             "(hipcc --offload-arch=gfx950); there is no CPU fallback")
        if _needs_torch_first():
            import torch  # noqa: F401  (runtime-order rule above)
        import sys
        torch_loaded_first = "torch" in sys.modules
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            f = getattr(L, name)
            f.restype, f.argtypes = res, args
        _lib = L
    return _lib


def _check(rc):
    if rc != 0:
        raise ThfheError(f"libthfhe_hip error {rc}: {lib().thfhe_last_error().decode()}")


def _p32(a):
    return a.ctypes.data_as(_i32p) if a is not None else None


def _wrap32(v):
    """An integer taken mod 2^32 as a signed int32 (weights and Torus32 constants)."""
    v = int(v) & 0xFFFFFFFF
    return v - (1 << 32) if v >= 1 << 31 else v


def _wrap64(v):
    """An integer taken mod 2^64 as a signed int64 (Torus64 constants)."""
    v = int(v) & 0xFFFFFFFFFFFFFFFF
    return v - (1 << 64) if v >= 1 << 63 else v


def _rec(a, words):
    a = np.ascontiguousarray(a, dtype=np.int32)
    if a.shape[-1] != words:
        raise ValueError(f"expected records of {words} int32 words, got shape {a.shape}")
    return a.reshape(-1, words)


def _same_count(x, *others):
    """The C side copies x.shape[0] records from every operand: a shorter one would be read out of bounds."""
    for o in others:
        if o is not None and o.shape[0] != x.shape[0]:
            raise ValueError(f"operand batches differ in length: {x.shape[0]} vs {o.shape[0]} records")


def _index(name, v, count):
    """A per-sample index (lut_index, table_index, val_index) as int32[count]; None stays None."""
    if v is None:
        return None
    v = np.ascontiguousarray(v, np.int32).reshape(-1)
    if v.shape[0] != count:
        raise ValueError(f"{name} holds {v.shape[0]} entries for {count} samples")
    return v


def _as_tuple(v):
    """The operands of one tree level, one record array or a tuple of 1 .. 3, as a 3-tuple padded with None."""
    return tuple(v) + (None,) * (3 - len(v)) if isinstance(v, (tuple, list)) else (v, None, None)


def _theta_records(theta):
    """Records per sample of the output array: theta, or 1 for a theta the library is going to refuse."""
    return int(theta) if theta in (1, 2, 4) else 1


class DeviceBuffer:
    """A device allocation owned by a context (records resident in HBM)."""

    def __init__(self, ctx, nbytes):
        self.ctx, self.nbytes = ctx, nbytes
        self.ptr = ctx._alloc(nbytes)
        if not self.ptr:
            raise ThfheError("device allocation failed")

    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        assert arr.nbytes <= self.nbytes
        self.ctx._h2d(self.ptr, arr)
        return self

    def download(self, shape, dtype=np.int32):
        out = np.empty(shape, dtype)
        assert out.nbytes <= self.nbytes
        self.ctx._d2h(out, self.ptr)
        return out

    def free(self):
        if self.ptr:
            self.ctx._free(self.ptr)
            self.ptr = None


class _Handle:
    """Owner of one native context handle: close() destroys it once; garbage collection closes it too."""

    h = None
    _destroy = None

    def _own(self, h, destroy):
        self.h, self._destroy = h, destroy

    def close(self):
        h, self.h = self.h, None
        if h and self._destroy is not None:
            self._destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter teardown
            pass

    def _kernel_name(self, fn, *args):
        """The answer of one of the library's thfhe_*_rotation_kernel_name calls for this context (the rule is csrc/thfhe_launch_plan.h's)."""
        buf = C.create_string_buffer(64)
        _check(fn(self.h, *args, buf, len(buf)))
        return buf.value.decode()


class _TgswSetBase(_Handle):
    """What TgswSet and MKTgswSet share: the address bits of `count` samples, d bits each, resident on the device of the key `ck` in the key's
    ring word.  A subclass names the layout of the samples: _layout(params) = (words per bit, the shape text of the refusal)."""

    def __init__(self, ck, samples, d):
        d = int(d)
        a = np.ascontiguousarray(samples, ck._tv_dtype)
        per_bit, shape = self._layout(ck.params)
        if d < 1 or a.size == 0 or a.size % (per_bit * d):
            raise ValueError(f"samples: expected {shape} with d = {d}")
        self.ck, self.d, self.count = ck, d, a.size // (per_bit * d)   # the key is kept alive for as long as the set
        h = _vp()
        _check(ck._fn("tgsw_set_create")(ck.h, ck._ptv(a), self.count, d, C.byref(h)))
        self._own(h, ck._fn("tgsw_set_destroy"))

    @classmethod
    def _adopt(cls, ck, h, count, d):
        """A set the library made itself (thfhe_circuit_bootstrap)."""
        self = cls.__new__(cls)
        self.ck, self.d, self.count = ck, d, count
        self._own(h, ck._fn("tgsw_set_destroy"))
        return self

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class TgswSet(_TgswSetBase):
    """TGSW samples resident on a CloudKey's device (thfhe_tgsw_set_create): the address bits of `count` samples, d bits each."""

    @staticmethod
    def _layout(p):
        return 2 * p.l * 2 * p.N, f"int32[count * d][{2 * p.l}][2][{p.N}]"


class MKTgswSet(_TgswSetBase):
    """TGSW samples resident on an MKCloudKey's device (thfhe_mk_tgsw_set_create): the address bits of `count` samples, d bits each."""

    @staticmethod
    def _layout(p):
        return 4 * p.l * p.N, f"int64[count * d][4][{p.l}][{p.N}]"


class _EvalKey(_Handle):
    """What CloudKey and MKCloudKey share: the same calls under the C symbol prefix `_prefix` (thfhe_ / thfhe_mk_)."""

    _prefix = None

    def _fn(self, name):
        return getattr(lib(), self._prefix + name)

    # -- host-buffer calls -------------------------------------------------------------------------
    def gates(self, op, x, y=None, z=None):
        x = _rec(x, self.words)
        y = _rec(y, self.words) if y is not None else None
        z = _rec(z, self.words) if z is not None else None
        _same_count(x, y, z)
        out = np.empty_like(x)
        _check(self._fn("gates")(self.h, op, _p32(x), _p32(y), _p32(z), _p32(out), x.shape[0]))
        return out

    def gates_mixed(self, ops, x, y):
        """One launch for a DAG level: gate g applies ops[g] (a two-input bootstrapped gate) to (x[g], y[g])."""
        x, y = _rec(x, self.words), _rec(y, self.words)
        ops = np.ascontiguousarray(ops, np.int32)
        _same_count(x, y, ops)
        out = np.empty_like(x)
        _check(self._fn("gates_mixed")(self.h, _p32(ops), _p32(x), _p32(y), _p32(out), x.shape[0]))
        return out

    def dag_run(self, input_records, gates):
        """Native levelising scheduler + device-resident executor.  gates: int32[n_gates][4] = (op, in0, in1, in2).
        Returns (wires int32[n_inputs + n_gates][words], stats dict)."""
        x = _rec(input_records, self.words)
        g = np.ascontiguousarray(gates, np.int32).reshape(-1, 4)
        wires = np.zeros((x.shape[0] + g.shape[0], self.words), np.int32)
        wires[:x.shape[0]] = x
        st = np.zeros(4, np.int64)
        _check(self._fn("dag_run")(self.h, _p32(wires), x.shape[0], _p32(g), g.shape[0], st.ctypes.data_as(_i64p)))
        return wires, dict(levels=int(st[0]), launches=int(st[1]), rotations=int(st[2]), widest_level=int(st[3]))

    def _dag_run(self, what, fn, ctxs, input_records, nodes, cols, families, out_wires, n_stats=4):
        """The marshalling every dag_run_*_batch shares: fn(*ctxs, inputs, the node rows of `cols` words, *families(), instances, out_wires, outputs, stats).
        families: called after the input records and the rows are checked.  Returns (outputs, the stats dictionary)."""
        words = self.words
        x = np.ascontiguousarray(input_records, np.int32)
        if x.ndim != 3 or x.shape[2] != words:
            raise ValueError("%s: input records must be int32[instances][n_inputs][%d]" % (what, words))
        g = np.ascontiguousarray(nodes, np.int32).reshape(-1, cols)
        fam = families()
        q, n_in = x.shape[0], x.shape[1]
        sel = None if out_wires is None else np.ascontiguousarray(out_wires, np.int32).reshape(-1)
        out = np.zeros((q, g.shape[0] if sel is None else sel.shape[0], words), np.int32)
        st = np.zeros(n_stats, np.int64)
        _check(fn(*ctxs, _p32(x), n_in, _p32(g), g.shape[0], *fam, q, _p32(sel), 0 if sel is None else sel.shape[0], _p32(out), st.ctypes.data_as(_i64p)))
        stats = dict(levels=int(st[0]), launches=int(st[1]), rotations=int(st[2]) * q, widest_level=int(st[3]) * q, instances=q)
        if n_stats > 4:   # thfhe_dag_run_cb_batch: the level-2 rotations of the CB nodes
            stats["level2_rotations"] = int(st[4]) * q
        return out, stats

    def dag_run_batch(self, input_records, gates, out_wires=None):
        """`instances` evaluations of one gate list side by side (the reference's loop over test records,
        src/KNN_medical_data.cpp:676-691).  input_records: int32[instances][n_inputs][words]; out_wires: wire ids to return (None = every
        gate wire).  Returns (int32[instances][len(out_wires) or n_gates][words], stats)."""
        return self._dag_run("dag_run_batch", self._fn("dag_run_batch"), (self.h,), input_records, gates, 4, tuple, out_wires)

    def dag_run_lut_batch(self, input_records, nodes, specs, tv, out_wires=None):
        """dag_run_batch with LUT nodes (thfhe_dag_run_lut_batch / thfhe_mk_dag_run_lut_batch).  nodes: int32[n_nodes][6] =
        (op, in0, in1, in2, spec, lut); specs: (n_inputs, (w0, w1, w2), bias, theta) tuples or LutSpec; tv: [n_luts][N] test vectors of the
        ring's torus (int32 for CloudKey, int64 for MKCloudKey).  Returns (int32[instances][len(out_wires) or n_nodes][words], stats)."""
        def families():
            sp = (LutSpec * len(specs))(*[_lut_spec(s) for s in specs])
            t = np.ascontiguousarray(tv, self._tv_dtype).reshape(-1, self.params.N)
            return sp, len(specs), self._ptv(t), t.shape[0]
        return self._dag_run("dag_run_lut_batch", self._fn("dag_run_lut_batch"), (self.h,), input_records, nodes, 6, families, out_wires)

    def _bootstrap(self, x, mu):
        x = _rec(x, self.words)
        out = np.empty_like(x)
        _check(self._fn("bootstrap")(self.h, mu, _p32(x), _p32(out), x.shape[0]))
        return out

    # -- programmable bootstrap (thfhe_lut_bootstrap / thfhe_mk_lut_bootstrap) ---------------------------------------------------
    def lut_bootstrap(self, tv, x, y=None, z=None, *, weights=(1,), bias=0, theta=1, lut_index=None):
        """Programmable bootstrap (include/thfhe_hip.h, thfhe_lut_bootstrap / thfhe_mk_lut_bootstrap): sample g evaluates test vector
        tv[lut_index[g]] (table 0 without an index) on x = sum_q weights[q] * (x, y, z)[q] + (0, bias), theta outputs per rotation.
        tv: [n_luts][N] test vectors of the ring's torus (thfhe.lut.test_vector): int32 for CloudKey, int64 (torus_bits=64) for MKCloudKey.
        Returns int32[count, theta, words] (words = n+1, or P*n+1 for the multi-key scheme)."""
        return self._lut(tv, x, y, z, weights, bias, theta, lut_index, True)

    def lut_bootstrap_wo_keyswitch(self, tv, x, y=None, z=None, *, weights=(1,), bias=0, theta=1, lut_index=None):
        """lut_bootstrap without the key switch: int32[count, theta, N+1] records under the ring key."""
        return self._lut(tv, x, y, z, weights, bias, theta, lut_index, False)

    _tv_dtype = np.int32   # the ring's torus: Torus32 test vectors (MKCloudKey: Torus64)

    def _ptv(self, a):
        return a.ctypes.data_as(_i64p if self._tv_dtype == np.int64 else _i32p)

    def _lut(self, tv, x, y, z, weights, bias, theta, lut_index, keyswitch):
        ins, spec, p = self._lut_args((x, y, z), weights, bias, theta)
        tv = np.ascontiguousarray(tv, self._tv_dtype).reshape(-1, self.params.N)
        count = ins[0].shape[0]
        idx = _index("lut_index", lut_index, count)
        out = np.empty((count, _theta_records(theta), self.words if keyswitch else self.params.N + 1), np.int32)
        fn = self._fn("lut_bootstrap" if keyswitch else "lut_bootstrap_wo_keyswitch")
        _check(fn(self.h, C.byref(spec), self._ptv(tv), tv.shape[0], _p32(idx), p[0], p[1], p[2], _p32(out), count))
        return out

    # -- leveled CMux and table lookup on TGSW-encrypted address bits (tgsw_set_create, lhe_cmux, lhe_lookup), in the ring's word:
    #    int32 and N = 1024 on a CloudKey, int64 and N = 2048 on an MKCloudKey -------------------------------------------------------------------
    _tgsw_set_class = None   # TgswSet / MKTgswSet

    def tgsw_set(self, samples, d):
        """Device-resident address bits of the samples, kept as spectra; each key class states its layout and sizes."""
        return self._tgsw_set_class(self, samples, d)

    def lhe_cmux(self, tset, bit, d1_a, d1_b, d0_a, d0_b):
        """(out_a, out_b) [count][N] in the ring's word: sample s gets d0[s] + C_(s,bit) (.) (d1[s] - d0[s])."""
        N = self.params.N
        arrs = [np.ascontiguousarray(v, self._tv_dtype).reshape(-1, N) for v in (d1_a, d1_b, d0_a, d0_b)]
        _same_count(*arrs)
        out_a, out_b = np.empty_like(arrs[0]), np.empty_like(arrs[0])
        _check(self._fn("lhe_cmux")(self.h, tset.h, int(bit), *[self._ptv(v) for v in arrs], self._ptv(out_a), self._ptv(out_b), arrs[0].shape[0]))
        return out_a, out_b

    def lhe_lookup(self, tset, tab_b, *, d_tree, d_rot, theta=1, tab_a=None, table_index=None, first=0, count=None):
        """Leveled lookup in the table tab_b [n_tables][2^d_tree][N] in the ring's word; returns key-switched records int32[count, theta, n+1]."""
        return self._lhe_lookup(tset, tab_b, d_tree, d_rot, theta, tab_a, table_index, first, count, True)

    def lhe_lookup_wo_keyswitch(self, tset, tab_b, *, d_tree, d_rot, theta=1, tab_a=None, table_index=None, first=0, count=None):
        """lhe_lookup without the key switch: int32[count, theta, N+1] records under the ring key."""
        return self._lhe_lookup(tset, tab_b, d_tree, d_rot, theta, tab_a, table_index, first, count, False)

    def _lhe_lookup(self, tset, tab_b, d_tree, d_rot, theta, tab_a, table_index, first, count, keyswitch):
        N = self.params.N
        if not 0 <= int(d_tree) <= 6:
            raise ValueError("d_tree must be 0 .. 6")
        leaves = 1 << int(d_tree)
        tab_b = np.ascontiguousarray(tab_b, self._tv_dtype)
        if tab_b.size == 0 or tab_b.size % (leaves * N):
            raise ValueError(f"tab_b: expected {np.dtype(self._tv_dtype).name}[n_tables][{leaves}][{N}]")
        if tab_a is not None:
            tab_a = np.ascontiguousarray(tab_a, self._tv_dtype)
            if tab_a.size != tab_b.size:
                raise ValueError("tab_a and tab_b differ in size")
        first = int(first)
        count = tset.count - first if count is None else int(count)
        if first < 0 or count < 0:
            raise ValueError("first and count must not be negative")
        idx = _index("table_index", table_index, count)
        out = np.empty((count, _theta_records(theta), self.words if keyswitch else N + 1), np.int32)
        fn = self._fn("lhe_lookup" if keyswitch else "lhe_lookup_wo_keyswitch")
        _check(fn(self.h, tset.h, first, count, int(d_tree), int(d_rot), int(theta), None if tab_a is None else self._ptv(tab_a), self._ptv(tab_b),
                  tab_b.size // (leaves * N), _p32(idx), _p32(out)))
        return out

    def _lut_args(self, ins, weights, bias, theta, what=None):
        """(records, LutSpec, the three operand pointers) of the operands `ins` = (x, y, z); what: the call, named in front of the error text."""
        given = [v for v in ins if v is not None]
        if any(v is None for v in ins[:len(given)]) or len(given) != len(weights):
            raise ValueError(f"{what}: give the inputs in order and one weight per input" if what else
                             "give the inputs in order (x, then y, then z) and one weight per input")
        recs = [_rec(v, self.words) for v in given]
        _same_count(*recs)
        w = list(weights) + [0] * (3 - len(weights))
        spec = LutSpec(len(recs), (C.c_int32 * 3)(*[_wrap32(v) for v in w]), _wrap32(bias), int(theta))
        return recs, spec, [_p32(v) for v in recs] + [None] * (3 - len(recs))

    # -- encrypted tables and the two-digit tree (thfhe_lut_bootstrap_enc / thfhe_mk_lut_bootstrap_enc) -----------------------
    def lut_bootstrap_enc(self, tv_a, tv_b, x, y=None, z=None, *, weights=(1,), bias=0, theta=1, lut_index=None):
        """lut_bootstrap with ENCRYPTED tables: table t is the ring sample (tv_a[t], tv_b[t]) of [N] words each; up to 262 144 tables, so every
        sample may bring its own.  CloudKey: int32 TLWE samples under the bootstrapping ring key (thfhe.lut.encrypt_table, or PackBoxes' output),
        returns int32[count, theta, n+1].  MKCloudKey: int64 RLWE samples under the summed ring key (thfhe.lut.encrypt_table(..., torus_bits=64),
        or pack_boxes' output), returns int32[count, theta, P*n+1]."""
        return self._lut_enc(tv_a, tv_b, x, y, z, weights, bias, theta, lut_index, True)

    def lut_bootstrap_enc_wo_keyswitch(self, tv_a, tv_b, x, y=None, z=None, *, weights=(1,), bias=0, theta=1, lut_index=None):
        """lut_bootstrap_enc without the key switch: int32[count, theta, N+1] records under the (MKCloudKey: coefficients of the summed) ring key."""
        return self._lut_enc(tv_a, tv_b, x, y, z, weights, bias, theta, lut_index, False)

    def _lut_enc(self, tv_a, tv_b, x, y, z, weights, bias, theta, lut_index, keyswitch):
        ins, spec, p = self._lut_args((x, y, z), weights, bias, theta, "lut_bootstrap_enc")
        N = self.params.N
        tv_a = np.ascontiguousarray(tv_a, self._tv_dtype).reshape(-1, N)
        tv_b = np.ascontiguousarray(tv_b, self._tv_dtype).reshape(-1, N)
        if tv_a.shape != tv_b.shape:
            raise ValueError(f"tv_a and tv_b differ in shape: {tv_a.shape} vs {tv_b.shape}")
        count = ins[0].shape[0]
        idx = _index("lut_index", lut_index, count)
        out = np.empty((count, _theta_records(theta), self.words if keyswitch else N + 1), np.int32)
        fn = self._fn("lut_bootstrap_enc" if keyswitch else "lut_bootstrap_enc_wo_keyswitch")
        _check(fn(self.h, C.byref(spec), self._ptv(tv_a), self._ptv(tv_b), tv_a.shape[0], _p32(idx), p[0], p[1], p[2], _p32(out), count))
        return out

    def _tree(self, ctxs, tv1, lo, hi, p_hi, weights_lo, bias_lo, theta, weights_hi, bias_hi, table_index):
        """The marshalling both tree_lut_bootstrap methods share; ctxs: the contexts the engine's entry takes (CloudKey: its own and the packing context)."""
        lo_r, spec_lo, plo = self._lut_args(_as_tuple(lo), weights_lo, bias_lo, theta, "tree_lut_bootstrap (lo)")
        hi_r, spec_hi, phi = self._lut_args(_as_tuple(hi), weights_hi, bias_hi, 1, "tree_lut_bootstrap (hi)")
        _same_count(lo_r[0], hi_r[0])
        count = lo_r[0].shape[0]
        R = int(p_hi) // int(theta) if theta in (1, 2, 4) else 1
        tv1 = np.ascontiguousarray(tv1, self._tv_dtype)
        if R < 1 or tv1.size == 0 or tv1.size % (R * self.params.N):
            raise ValueError(f"tv1: expected {np.dtype(self._tv_dtype).name}[n_tables][{R}][{self.params.N}]")
        idx = _index("table_index", table_index, count)
        out = np.empty((count, self.words), np.int32)
        _check(self._fn("tree_lut_bootstrap")(*ctxs, C.byref(spec_lo), C.byref(spec_hi), int(p_hi), self._ptv(tv1), tv1.size // (R * self.params.N),
                                              _p32(idx), plo[0], plo[1], plo[2], phi[0], phi[1], phi[2], _p32(out), count))
        return out

    # -- multi-value bootstrapping (thfhe_mv_lut_bootstrap / thfhe_mk_mv_lut_bootstrap) -------------------------------------------------------
    def _mv_tables(self, factors, tv0, table_index, count):
        w = np.ascontiguousarray(factors, np.int32)
        if w.ndim == 2:
            w = w[None]
        if w.ndim != 3 or w.size == 0:
            raise ValueError("factors: expected int32[q][p] or int32[n_tables][q][p]")
        tv0 = np.ascontiguousarray(tv0, self._tv_dtype).reshape(-1)
        if tv0.shape[0] != self.params.N:
            raise ValueError(f"tv0: expected {np.dtype(self._tv_dtype).name}[{self.params.N}]")
        return w, tv0, _index("table_index", table_index, count)

    def _mv(self, factors, x, y, z, tv0, weights, bias, table_index, keyswitch, *extra):
        """extra: what the engine's entry takes after table_index (MKCloudKey: out_bias)"""
        ins, spec, p = self._lut_args((x, y, z), weights, bias, 1, "mv_lut_bootstrap")
        count = ins[0].shape[0]
        w, tv0, idx = self._mv_tables(factors, tv0, table_index, count)
        out = np.empty((count, w.shape[1], self.words if keyswitch else self.params.N + 1), np.int32)
        fn = self._fn("mv_lut_bootstrap" if keyswitch else "mv_lut_bootstrap_wo_keyswitch")
        _check(fn(self.h, C.byref(spec), self._ptv(tv0), _p32(w), w.shape[2], w.shape[1], w.shape[0], _p32(idx), *extra, p[0], p[1], p[2], _p32(out), count))
        return out

    # -- encrypted dense layers (thfhe_lwe_linear, thfhe_linear_lut_bootstrap and their thfhe_mk_ forms) --------------------------
    def lwe_linear(self, W, x, bias=None):
        """An integer matrix times a vector of records, word-wise mod 2^32: out[s][m] = sum_k W[m][k] * x[s][k] + (0, bias[m]).
        W: int32[M][K] (any int32 values, the products wrap); x: int32[count][K][words]; bias: M Torus32 words or None.
        Returns int32[count, M, words]."""
        W, x, b = self._linear_args(W, x, bias)
        out = np.empty((x.shape[0], W.shape[0], self.words), np.int32)
        _check(self._fn("lwe_linear")(self.h, _p32(W), _p32(b), W.shape[0], W.shape[1], _p32(x), _p32(out), x.shape[0]))
        return out

    def linear_lut_bootstrap(self, tv, W, x, bias=None, theta=1, lut_index=None):
        """A dense layer and its activation in one call: lwe_linear(W, x, bias), then output m of every sample bootstrapped on table
        tv[lut_index[m]] (table 0 without an index), theta records each; the sums never leave the device.  Word for word what lwe_linear followed by
        lut_bootstrap(tv, sums, theta=theta) returns.  tv: [n_luts][N] test vectors of the ring's torus; lut_index: M entries, one per OUTPUT.
        Every reachable sum of messages must stay in [0, p) of the tables' encoding (thfhe.circuits.dense_bias).  Returns int32[count, M, theta, words]."""
        return self._linear_lut(tv, W, x, bias, theta, lut_index, True)

    def linear_lut_bootstrap_wo_keyswitch(self, tv, W, x, bias=None, theta=1, lut_index=None):
        """linear_lut_bootstrap without the key switch: int32[count, M, theta, N+1] records under the ring key."""
        return self._linear_lut(tv, W, x, bias, theta, lut_index, False)

    def _linear_args(self, W, x, bias):
        W = np.ascontiguousarray(W, np.int32)
        x = np.ascontiguousarray(x, np.int32)
        if W.ndim != 2 or W.size == 0:
            raise ValueError("W: expected int32[M][K]")
        if x.ndim == 2:
            x = x[None]
        if x.ndim != 3 or x.shape[1] != W.shape[1] or x.shape[2] != self.words:
            raise ValueError(f"x: expected int32[count][{W.shape[1]}][{self.words}], got shape {x.shape}")
        b = None
        if bias is not None:
            b = np.array([_wrap32(v) for v in np.asarray(bias).reshape(-1)], np.int32)
            if b.shape[0] != W.shape[0]:
                raise ValueError(f"bias holds {b.shape[0]} entries for {W.shape[0]} outputs")
        return W, x, b

    def _linear_lut(self, tv, W, x, bias, theta, lut_index, keyswitch):
        W, x, b = self._linear_args(W, x, bias)
        tv = np.ascontiguousarray(tv, self._tv_dtype).reshape(-1, self.params.N)
        idx = _index("lut_index", lut_index, W.shape[0])
        out = np.empty((x.shape[0], W.shape[0], _theta_records(theta), self.words if keyswitch else self.params.N + 1), np.int32)
        fn = self._fn("linear_lut_bootstrap" if keyswitch else "linear_lut_bootstrap_wo_keyswitch")
        _check(fn(self.h, _p32(W), _p32(b), W.shape[0], W.shape[1], int(theta), self._ptv(tv), tv.shape[0], _p32(idx), _p32(x), _p32(out), x.shape[0]))
        return out

    def set_linear_slice(self, jobs):
        """The most PBS jobs (samples x outputs) of one slice of a dense-layer call; a slice holds whole samples, at least one.  The result does not
        depend on it."""
        _check(self._fn("set_linear_slice")(self.h, int(jobs)))

    def linear_last_timings(self):
        """Device-event times of the last slice of the last dense-layer call made with profiling on: the input upload, lwe_linear_kernel, and upload
        start .. end of the key switch (the kernel's end for a call without one)."""
        ms = (C.c_float * 3)()
        _check(self._fn("linear_last_timings")(self.h, ms))
        return dict(upload_ms=ms[0], linear_ms=ms[1], total_ms=ms[2])

    @staticmethod
    def linear_tile():
        """(tile_m, tile_k): the outputs and the reduction steps lwe_linear_kernel handles per pass (where a test places its edges)."""
        tm, tk = C.c_int(), C.c_int()
        _check(lib().thfhe_linear_tile(C.byref(tm), C.byref(tk)))
        return tm.value, tk.value

    # -- device-buffer calls -----------------------------------------------------------------------
    def _alloc(self, n):
        return self._fn("dev_alloc")(self.h, n)

    def _free(self, p):
        self._fn("dev_free")(self.h, p)

    def _h2d(self, dptr, arr):
        _check(self._fn("copy_h2d")(self.h, dptr, arr.ctypes.data_as(_vp), arr.nbytes))

    def _d2h(self, arr, dptr):
        _check(self._fn("copy_d2h")(self.h, arr.ctypes.data_as(_vp), dptr, arr.nbytes))

    def device_records(self, count):
        return DeviceBuffer(self, count * self.words * 4)

    def reserve(self, max_count):
        _check(self._fn("reserve")(self.h, max_count))

    def gates_dev(self, op, dx, dy, dz, dout, count):
        _check(self._fn("gates_dev")(self.h, op, dx.ptr, dy.ptr if dy else None, dz.ptr if dz else None, dout.ptr, count))

    def sync(self):
        _check(self._fn("sync")(self.h))

    def set_dag_slice(self, max_gates):
        """Gates per launch of a DAG level (dag_run_batch cuts wider levels into slices)."""
        _check(self._fn("set_dag_slice")(self.h, int(max_gates)))

    def set_profiling(self, on):
        _check(self._fn("set_profiling")(self.h, int(bool(on))))

    def last_timings(self):
        ms = (C.c_float * 4)()
        _check(self._fn("last_timings")(self.h, ms))
        return dict(prologue_ms=ms[0], blind_rotate_ms=ms[1], keyswitch_ms=ms[2], total_ms=ms[3])


class CloudKey(_EvalKey):
    """Single-key evaluation context = the reference's CloudKey (api.jl:215-231): bootstrap key + keyswitch key,
    held on one MI355X in the engine's transformed layout.

    bk_coeff: int32[n][(k+1)l][k+1][N] coefficient-domain TGSW rows; ksk: int32[N][t][base-1][n+1].
    """

    _prefix = "thfhe_"
    _tgsw_set_class = TgswSet

    def __init__(self, params, bk_coeff, ksk, device=0):
        self.params = params
        bk = np.ascontiguousarray(bk_coeff, np.int32)
        ks = np.ascontiguousarray(ksk, np.int32)
        p = params
        if bk.size != p.n * (p.k + 1) * p.l * (p.k + 1) * p.N:
            raise ValueError("bk_coeff has the wrong size for these parameters")
        if ks.size != p.N * p.k * p.ks_t * ((1 << p.ks_basebit) - 1) * (p.n + 1):
            raise ValueError("ksk has the wrong size for these parameters")
        h = _vp()
        _check(lib().thfhe_ctx_create(C.byref(p), _p32(bk), _p32(ks), device, C.byref(h)))
        self._own(h, lib().thfhe_ctx_destroy)
        self.words = p.n + 1

    def bootstrap(self, x, mu=MU8):
        return self._bootstrap(x, mu)

    def bootstrap_wo_keyswitch(self, x, mu=MU8):
        x = _rec(x, self.words)
        out = np.empty((x.shape[0], self.params.N + 1), np.int32)
        _check(lib().thfhe_bootstrap_wo_keyswitch(self.h, mu, _p32(x), _p32(out), x.shape[0]))
        return out

    def keyswitch(self, u):
        u = _rec(u, self.params.N + 1)
        out = np.empty((u.shape[0], self.words), np.int32)
        _check(lib().thfhe_keyswitch(self.h, _p32(u), _p32(out), u.shape[0]))
        return out

    # -- the two-digit tree (thfhe_tree_lut_bootstrap); lut_bootstrap_enc takes int32 TLWE tables here ----------------------------
    def tree_lut_bootstrap(self, poly_ctx, tv1, lo, hi, *, p_hi, weights_lo=(1,), bias_lo=0, theta=1, weights_hi=(1,), bias_hi=0, table_index=None):
        """Two-digit tree PBS (thfhe_tree_lut_bootstrap): sample s gets f_table[s](hi, lo) as one record int32[count, n+1].  lo, hi: one record
        array or a tuple of 1 .. 3 (weighted by weights_lo / weights_hi); tv1: int32[n_tables][p_hi / theta][N] (thfhe.lut.tree_test_vectors);
        poly_ctx: a threshold.PolyContext holding the packing key from this key set's LWE key to its bootstrapping ring key."""
        return self._tree((self.h, poly_ctx.h), tv1, lo, hi, p_hi, weights_lo, bias_lo, theta, weights_hi, bias_hi, table_index)

    # -- multi-value bootstrapping with factored test vectors (thfhe_mv_lut_bootstrap, thfhe_tree_lut_bootstrap_mv) ---------
    def mv_lut_bootstrap(self, factors, x, y=None, z=None, *, tv0, weights=(1,), bias=0, table_index=None):
        """q functions of one encrypted digit from ONE blind rotation: the base vector tv0 int32[N] (thfhe.lut.mv_base) is rotated by
        x = sum_q weights[q] * (x, y, z)[q] + (0, bias) at theta = 1, and output j of sample s is coefficient 0 of ACC_s * F_j, F_j built from the p
        taps factors[table_index[s]][j] (thfhe.lut.mv_factors).  factors: int32[q][p] or int32[n_tables][q][p].  Returns int32[count, q, n+1]."""
        return self._mv(factors, x, y, z, tv0, weights, bias, table_index, True)

    def mv_lut_bootstrap_wo_keyswitch(self, factors, x, y=None, z=None, *, tv0, weights=(1,), bias=0, table_index=None):
        """mv_lut_bootstrap without the key switch: int32[count, q, N+1] records under the ring key."""
        return self._mv(factors, x, y, z, tv0, weights, bias, table_index, False)

    def tree_lut_bootstrap_mv(self, poly_ctx, factors, lo, hi, *, tv0, weights_lo=(1,), bias_lo=0, weights_hi=(1,), bias_hi=0, table_index=None):
        """tree_lut_bootstrap with level 1 as ONE multi-value rotation per sample (thfhe_tree_lut_bootstrap_mv): 1 + 1 rotations whatever p_hi is.
        tv0, factors int32[p_hi][p_lo] or int32[n_tables][p_hi][p_lo]: thfhe.lut.tree_mv_factors.  int32[count, n+1]."""
        lo_r, spec_lo, plo = self._lut_args(_as_tuple(lo), weights_lo, bias_lo, 1, "tree_lut_bootstrap_mv (lo)")
        hi_r, spec_hi, phi = self._lut_args(_as_tuple(hi), weights_hi, bias_hi, 1, "tree_lut_bootstrap_mv (hi)")
        _same_count(lo_r[0], hi_r[0])
        count = lo_r[0].shape[0]
        w, tv0, idx = self._mv_tables(factors, tv0, table_index, count)
        out = np.empty((count, self.words), np.int32)
        _check(lib().thfhe_tree_lut_bootstrap_mv(self.h, poly_ctx.h, C.byref(spec_lo), C.byref(spec_hi), w.shape[1], w.shape[2], _p32(tv0), _p32(w), w.shape[0],
                                                 _p32(idx), plo[0], plo[1], plo[2], phi[0], phi[1], phi[2], _p32(out), count))
        return out

    def tree_lut_bootstrap_mvk(self, poly_ctx, factors, lo, hi, *, tv0, weights_lo=(1,), bias_lo=0, weights_hi=(1,), bias_hi=0, table_index=None):
        """tree_lut_bootstrap_mv with k tables per sample (thfhe_tree_lut_bootstrap_mvk): out[s][j] = f_j(hi_s, lo_s) in 1 + k rotations.
        tv0, factors int32[k][p_hi][p_lo] or int32[n_tables][k][p_hi][p_lo]: thfhe.lut.tree_mvk_factors; k p_hi <= 64.  int32[count, k, n+1]."""
        lo_r, spec_lo, plo = self._lut_args(_as_tuple(lo), weights_lo, bias_lo, 1, "tree_lut_bootstrap_mvk (lo)")
        hi_r, spec_hi, phi = self._lut_args(_as_tuple(hi), weights_hi, bias_hi, 1, "tree_lut_bootstrap_mvk (hi)")
        _same_count(lo_r[0], hi_r[0])
        count = lo_r[0].shape[0]
        w = np.ascontiguousarray(factors, np.int32)
        if w.ndim == 3:
            w = w[None]
        if w.ndim != 4 or w.size == 0:
            raise ValueError("factors: expected int32[k][p_hi][p_lo] or int32[n_tables][k][p_hi][p_lo]")
        _, tv0, idx = self._mv_tables(w[0], tv0, table_index, count)
        out = np.empty((count, w.shape[1], self.words), np.int32)
        _check(lib().thfhe_tree_lut_bootstrap_mvk(self.h, poly_ctx.h, C.byref(spec_lo), C.byref(spec_hi), w.shape[2], w.shape[3], w.shape[1], _p32(tv0), _p32(w),
                                                  w.shape[0], _p32(idx), plo[0], plo[1], plo[2], phi[0], phi[1], phi[2], _p32(out), count))
        return out

    def dag_run_mv_batch(self, input_records, nodes, specs=(), tv=None, enc_a=None, enc_b=None, trees=(), tv1=None, mvs=(), mv_tv0=None, mv_factors=None,
                         out_wires=None, pack=None):
        """dag_run_tree_batch with multi-value nodes (thfhe_dag_run_mv_batch).  mvs: MvSpec or (lo, hi, p, q, k, base, factors_off, n_tables)
        tuples (hi may be None: MV only); mv_tv0: int32[n_bases][N] base vectors; mv_factors: int32[words], the taps of every spec."""
        mv = _mv_specs(mvs)
        tv0 = None if mv_tv0 is None else np.ascontiguousarray(mv_tv0, np.int32).reshape(-1, self.params.N)
        fac = None if mv_factors is None else np.ascontiguousarray(mv_factors, np.int32).reshape(-1)
        families = (mv, len(mvs), _p32(tv0), 0 if tv0 is None else tv0.shape[0], _p32(fac), 0 if fac is None else fac.shape[0])
        return self._dag_run_ext(lib().thfhe_dag_run_mv_batch, families, input_records, nodes, specs, tv, enc_a, enc_b, trees, tv1, out_wires, pack)

    def dag_run_lhe_batch(self, input_records, nodes, specs=(), tv=None, enc_a=None, enc_b=None, trees=(), tv1=None, mvs=(), mv_tv0=None, mv_factors=None,
                          tgsw_sets=(), lks=(), tab_b=None, tab_a=None, wfas=(), wfa_words=None, fin_b=None, fin_a=None, out_wires=None, pack=None):
        """dag_run_mv_batch with leveled nodes on TGSW-encrypted bits (thfhe_dag_run_lhe_batch).  tgsw_sets: the TgswSets of this key,
        instance q reads sample q of each; lks: DagLheSpec or (set, d_tree, d_rot, theta) tuples; tab_b / tab_a: int32[rows][N] table polynomials
        (tab_a None: public); wfas: DagWfaSpec or (n_steps, n_states, theta, n_out, set0, n_sets, trans_off, step_off, start_off) tuples; wfa_words:
        int32[words], their pool; fin_b / fin_a: int32[rows][N] final weights; pack: needed when an LHE_GATHER node is present.  Without any leveled
        family the call is dag_run_mv_batch."""
        return self._dag_run_leveled(None, input_records, nodes, specs, tv, enc_a, enc_b, trees, tv1, mvs, mv_tv0, mv_factors, tgsw_sets, lks, tab_b, tab_a, wfas,
                                     wfa_words, fin_b, fin_a, out_wires, pack)

    def _dag_run_leveled(self, cb, input_records, nodes, specs=(), tv=None, enc_a=None, enc_b=None, trees=(), tv1=None, mvs=(), mv_tv0=None, mv_factors=None,
                         tgsw_sets=(), lks=(), tab_b=None, tab_a=None, wfas=(), wfa_words=None, fin_b=None, fin_a=None, out_wires=None, pack=None, dense=None):
        """What dag_run_lhe_batch (cb = None) and dag_run_cb_batch share: the leveled families.  cb = (the level-2 key or None, a pointer to the
        DagCbFamilies or None): the run goes through thfhe_dag_run_cb_batch with the level-2 context after the other two and a fifth statistic.
        dense = (a pointer to the DagDenseFamilies or None,): the run goes through thfhe_dag_run_dense_batch, the pointer after cb's."""
        N = self.params.N
        mv = _mv_specs(mvs)
        tv0 = None if mv_tv0 is None else np.ascontiguousarray(mv_tv0, np.int32).reshape(-1, N)
        fac = None if mv_factors is None else np.ascontiguousarray(mv_factors, np.int32).reshape(-1)
        tab = lambda a: None if a is None else np.ascontiguousarray(a, np.int32).reshape(-1, N)
        rows = lambda a: 0 if a is None else a.shape[0]
        tab_a, tab_b, fin_a, fin_b = tab(tab_a), tab(tab_b), tab(fin_a), tab(fin_b)
        if (tab_a is not None and (tab_b is None or tab_a.shape != tab_b.shape)) or (fin_a is not None and (fin_b is None or fin_a.shape != fin_b.shape)):
            raise ValueError("tab_a / fin_a need tab_b / fin_b of the same shape")
        words = None if wfa_words is None else np.ascontiguousarray(wfa_words, np.int32).reshape(-1)
        hs = (_vp * len(tgsw_sets))(*[t.h for t in tgsw_sets]) if len(tgsw_sets) else None
        lk = (DagLheSpec * len(lks))(*[k if isinstance(k, DagLheSpec) else DagLheSpec(*[int(v) for v in k]) for k in lks]) if len(lks) else None
        wf = (DagWfaSpec * len(wfas))(*[a if isinstance(a, DagWfaSpec) else DagWfaSpec(*[int(v) for v in a]) for a in wfas]) if len(wfas) else None
        fam = DagLheFamilies(hs, len(tgsw_sets), lk, len(lks), _p32(tab_a), _p32(tab_b), rows(tab_b), wf, len(wfas), _p32(words),
                             0 if words is None else words.shape[0], _p32(fin_a), _p32(fin_b), rows(fin_b))
        leveled = len(tgsw_sets) or len(lks) or len(wfas) or tab_b is not None or fin_b is not None or words is not None
        families = (mv, len(mvs), _p32(tv0), rows(tv0), _p32(fac), 0 if fac is None else fac.shape[0], C.byref(fam) if leveled else None)
        if cb is None:
            return self._dag_run_ext(lib().thfhe_dag_run_lhe_batch, families, input_records, nodes, specs, tv, enc_a, enc_b, trees, tv1, out_wires, pack)
        level2, cb_fam = cb
        if dense is not None:
            return self._dag_run_ext(lib().thfhe_dag_run_dense_batch, families + (cb_fam, dense[0]), input_records, nodes, specs, tv, enc_a, enc_b, trees, tv1, out_wires,
                                     pack, more_ctxs=(None if level2 is None else level2.h,), n_stats=5)
        return self._dag_run_ext(lib().thfhe_dag_run_cb_batch, families + (cb_fam,), input_records, nodes, specs, tv, enc_a, enc_b, trees, tv1, out_wires, pack,
                                 more_ctxs=(None if level2 is None else level2.h,), n_stats=5)

    def dag_run_cb_batch(self, input_records, nodes, cb_sets=(), cb_wires=(), one_rotation=False, return_words=False, level2=None, **kw):
        """dag_run_lhe_batch with circuit-bootstrap nodes (thfhe_dag_run_cb_batch): a CB row turns d wires of the run into the TGSW bits
        of a computed set, which leveled rows read under set index len(tgsw_sets) + c.  cb_sets: (d, wire_off) tuples or DagCbSpec, one per computed
        set; cb_wires: the pool of wire ids they slice; one_rotation: stage A from one level-2 rotation per bit (gate-encoded operands only);
        return_words: also the rows of every computed set, a list of int32[instances][d][2l][2][N], as (outputs, stats, words); level2: the level-2
        MKCloudKey (default: the one cb_key_set named); the other arguments are dag_run_lhe_batch's.  Without cb_sets the call is dag_run_lhe_batch
        through the new entry.  stats gains level2_rotations."""
        p = self.params
        l2 = level2 if level2 is not None else getattr(self, "_cb_level2", None)
        if not len(cb_sets):
            return self._dag_run_leveled((l2, None), input_records, nodes, **kw)
        q = np.asarray(input_records).shape[0]
        cs = (DagCbSpec * len(cb_sets))(*[s if isinstance(s, DagCbSpec) else DagCbSpec(int(s[0]), int(s[1])) for s in cb_sets])
        pool = np.ascontiguousarray(cb_wires, np.int32).reshape(-1)
        words = [np.zeros((q, s.d, 2 * p.l, 2, p.N), np.int32) for s in cs] if return_words else None
        wp = (C.POINTER(C.c_int32) * len(cs))(*[_p32(w) for w in words]) if return_words else None
        fam = DagCbFamilies(cs, len(cs), _p32(pool), pool.shape[0], CB_ONE_ROTATION if one_rotation else CB_PER_LEVEL, wp)
        out, st = self._dag_run_leveled((l2, C.byref(fam)), input_records, nodes, **kw)
        return (out, st, words) if return_words else (out, st)

    def dag_run_dense_batch(self, input_records, nodes, dense_layers=(), dense_words=None, dense_wires=None, **kw):
        """dag_run_cb_batch with dense-layer nodes (thfhe_dag_run_dense_batch): a DENSE row (DENSE, wire_off, -1, -1, layer, -1) and its
        M theta - 1 LUT_OUT rows are linear_lut_bootstrap of layer `layer` on the K wires dense_wires[wire_off .. wire_off + K), the M theta records
        on consecutive wires.  dense_layers: DagDenseSpec or (M, K, theta, w_off, bias_off, lut_off) tuples into dense_words (int32: weights, bias
        words, table indices; an offset of -1: none); tv (keyword) holds the tables.  The other arguments are dag_run_cb_batch's.  Without the three
        the call is dag_run_cb_batch through the new entry."""
        fam, keep = _dense_families(dense_layers, dense_words, dense_wires)
        return self.dag_run_cb_batch(input_records, nodes, dense=(None if fam is None else C.byref(fam),), **kw)

    def dag_cb_release(self):
        """Free the computed sets the CB nodes of earlier dag_run_cb_batch calls left on this key (thfhe_dag_cb_release); the next run allocates again."""
        _check(lib().thfhe_dag_cb_release(self.h))

    def dag_last_group_ms(self):
        """Device time of the last SELECT / TREE / MV / TREE_MV / leveled group of the last dag_run_*_batch with set_profiling(True) (thfhe_dag_last_group_ms)."""
        ms = C.c_float()
        _check(lib().thfhe_dag_last_group_ms(self.h, C.byref(ms)))
        return ms.value

    def dag_last_stage_ms(self):
        """Device-event times of the stages of the last dag_run_lut_batch ... dag_run_dense_batch made with set_profiling(True)
        (thfhe_dag_last_stage_ms): the uploads (inputs, index table, output wire list), the levels, the output gather and download."""
        ms = (C.c_float * 3)()
        _check(lib().thfhe_dag_last_stage_ms(self.h, ms))
        return dict(upload_ms=ms[0], levels_ms=ms[1], download_ms=ms[2])

    def dag_run_tree_batch(self, input_records, nodes, specs=(), tv=None, enc_a=None, enc_b=None, trees=(), tv1=None, out_wires=None, pack=None):
        """dag_run_lut_batch with encrypted-table, select and tree nodes (thfhe_dag_run_tree_batch).  nodes: int32[n_nodes][6];
        specs, tv: as dag_run_lut_batch, both may be absent; enc_a, enc_b: int32[n_enc][N] encrypted tables; trees: (lo, hi, p_hi) tuples of spec
        tuples (lo may be None: SELECT only) or TreeSpec; tv1: int32[rows][N] level-1 rows; pack: the threshold.PolyContext holding the packing key
        (needed when a SELECT or TREE node is present).  Returns (int32[instances][len(out_wires) or n_nodes][words], stats)."""
        return self._dag_run_ext(lib().thfhe_dag_run_tree_batch, (), input_records, nodes, specs, tv, enc_a, enc_b, trees, tv1, out_wires, pack)

    def _dag_run_ext(self, fn, families, input_records, nodes, specs, tv, enc_a, enc_b, trees, tv1, out_wires, pack, more_ctxs=(), n_stats=4):
        """What dag_run_tree_batch and dag_run_mv_batch share: fn(contexts, inputs, nodes, the earlier table families, `families` -- the multi-value
        arguments of thfhe_dag_run_mv_batch, none for thfhe_dag_run_tree_batch --, instances, outputs, stats)."""
        def earlier():
            sp = (LutSpec * len(specs))(*[_lut_spec(s) for s in specs]) if len(specs) else None
            tr = (TreeSpec * len(trees))(*[t if isinstance(t, TreeSpec) else TreeSpec(_lut_spec(t[0] or _NO_SPEC), _lut_spec(t[1]), int(t[2])) for t in trees]) if len(trees) else None
            tab = lambda a: None if a is None else np.ascontiguousarray(a, np.int32).reshape(-1, self.params.N)
            t, ea, eb, t1 = tab(tv), tab(enc_a), tab(enc_b), tab(tv1)
            if (ea is None) != (eb is None) or (ea is not None and ea.shape != eb.shape):
                raise ValueError("enc_a and enc_b must both be given, with the same shape")
            rows = lambda a: 0 if a is None else a.shape[0]
            return (sp, len(specs), _p32(t), rows(t), _p32(ea), _p32(eb), rows(ea), tr, len(trees), _p32(t1), rows(t1)) + tuple(families)
        ctxs = (self.h, None if pack is None else pack.h) + tuple(more_ctxs)   # thfhe_dag_run_cb_batch: the level-2 context after the two
        return self._dag_run("dag_run_tree_batch / dag_run_mv_batch", fn, ctxs, input_records, nodes, 6, earlier, out_wires, n_stats)

    # -- leveled table lookup on TGSW-encrypted address bits (thfhe_tgsw_set_create, thfhe_lhe_cmux, thfhe_lhe_lookup): the bodies are
    #    _EvalKey's, the wording about this ring's layout and sizes is kept here ----------------------------------------------------------------
    def tgsw_set(self, samples, d):
        """Device-resident address bits: samples int32[count * d][2l][2][N] (SecretKeySet.tgsw_encrypt of the bits, sample-major: bit i of sample s
        is row s d + i), kept as spectra, count d 2l 32 KiB.  Returns a TgswSet: close() it (or use `with`) before this key is closed."""
        return super().tgsw_set(samples, d)

    def lhe_cmux(self, tset, bit, d1_a, d1_b, d0_a, d0_b):
        """(out_a, out_b) int32[count][N]: sample s gets d0[s] + C_(s,bit) (.) (d1[s] - d0[s]) -- d1 where its address bit `bit` is 1, else d0."""
        return super().lhe_cmux(tset, bit, d1_a, d1_b, d0_a, d0_b)

    def lhe_lookup(self, tset, tab_b, *, d_tree, d_rot, theta=1, tab_a=None, table_index=None, first=0, count=None):
        """Leveled lookup of samples first .. first+count-1 of the set (default: all from `first`) in the table tab_b int32[n_tables][2^d_tree][N]
        (thfhe.lut.lhe_table; tab_a: the masks of an encrypted table, None: public): d_tree + d_rot CMuxes, theta functions per sample.
        Returns key-switched records int32[count, theta, n+1]."""
        return self._lhe_lookup(tset, tab_b, d_tree, d_rot, theta, tab_a, table_index, first, count, True)

    # -- layered automata on TGSW-encrypted bits (thfhe_lhe_wfa) ------------------------------------------------------------------
    def lhe_wfa(self, sets, trans, step_bit, fin_b, start, *, theta=1, fin_a=None, table_index=None, first=0, count=None):
        """Evaluate a layered automaton on samples first .. first+count-1 of `sets` (a list of TgswSet of this key with one count; step j reads
        bit step_bit[j] & 15 of set step_bit[j] >> 4): trans int32[n_steps][n_states][2], fin_b int32[n_tables][n_states][N] the final weights
        (thfhe.lut.wfa_finals; fin_a: their masks, None: trivial samples), start int32[n_out].  One CMux per state and step (a copy where both
        transitions agree).  Returns key-switched records int32[count, n_out, theta, n+1]."""
        return self._lhe_wfa(sets, trans, step_bit, fin_b, start, theta, fin_a, table_index, first, count, True)

    def lhe_wfa_wo_keyswitch(self, sets, trans, step_bit, fin_b, start, *, theta=1, fin_a=None, table_index=None, first=0, count=None):
        """lhe_wfa without the key switch: int32[count, n_out, theta, N+1] records under the ring key."""
        return self._lhe_wfa(sets, trans, step_bit, fin_b, start, theta, fin_a, table_index, first, count, False)

    def _lhe_wfa(self, sets, trans, step_bit, fin_b, start, theta, fin_a, table_index, first, count, keyswitch):
        N = self.params.N
        sets = list(sets)
        if not sets:
            raise ValueError("sets: expected at least one TgswSet")
        trans = np.ascontiguousarray(trans, np.int32)
        if trans.ndim != 3 or trans.shape[2] != 2 or trans.size == 0:
            raise ValueError("trans: expected int32[n_steps][n_states][2]")
        n_steps, n_states = trans.shape[:2]
        step_bit = np.ascontiguousarray(step_bit, np.int32).reshape(-1)
        if step_bit.shape[0] != n_steps:
            raise ValueError(f"step_bit holds {step_bit.shape[0]} entries for {n_steps} steps")
        fin_b = np.ascontiguousarray(fin_b, np.int32)
        if fin_b.size == 0 or fin_b.size % (n_states * N):
            raise ValueError(f"fin_b: expected int32[n_tables][{n_states}][{N}]")
        if fin_a is not None:
            fin_a = np.ascontiguousarray(fin_a, np.int32)
            if fin_a.size != fin_b.size:
                raise ValueError("fin_a and fin_b differ in size")
        start = np.ascontiguousarray(start, np.int32).reshape(-1)
        first = int(first)
        count = sets[0].count - first if count is None else int(count)
        if first < 0 or count < 0:
            raise ValueError("first and count must not be negative")
        idx = _index("table_index", table_index, count)
        hs = (_vp * len(sets))(*[t.h for t in sets])
        out = np.empty((count, max(start.shape[0], 1), _theta_records(theta), self.words if keyswitch else N + 1), np.int32)
        fn = lib().thfhe_lhe_wfa if keyswitch else lib().thfhe_lhe_wfa_wo_keyswitch
        _check(fn(self.h, hs, len(sets), first, count, n_steps, n_states, _p32(trans), _p32(step_bit), _p32(fin_a), _p32(fin_b),
                  fin_b.size // (n_states * N), _p32(idx), int(theta), _p32(start), start.shape[0], _p32(out)))
        return out

    # -- leveled scatter: demux trees that write at TGSW-encrypted addresses (thfhe_lhe_demux, thfhe_lhe_scatter) -----------------
    def lhe_demux(self, tset, bit, x_b, x_a=None):
        """(out0_a, out0_b, out1_a, out1_b) int32[count][N]: sample s gets out1 = C_(s,bit) (.) x[s] and out0 = x[s] - out1 -- x in out1 where its
        address bit `bit` is 1, in out0 where it is 0, an encryption of zero in the other.  x_a None: the trivial samples (0, x_b)."""
        N = self.params.N
        x_b = np.ascontiguousarray(x_b, np.int32).reshape(-1, N)
        if x_a is not None:
            x_a = np.ascontiguousarray(x_a, np.int32).reshape(-1, N)
            _same_count(x_a, x_b)
        outs = [np.empty_like(x_b) for _ in range(4)]
        _check(lib().thfhe_lhe_demux(self.h, tset.h, int(bit), _p32(x_a), _p32(x_b), *[_p32(v) for v in outs], x_b.shape[0]))
        return tuple(outs)

    def lhe_scatter(self, tset, val_b, *, d_tree, d_rot, val_a=None, val_index=None, n_tables=1, table_index=None, first=0, count=None):
        """Leveled scatter of samples first .. first+count-1 of the set (default: all from `first`): sample s adds its value -- val_b
        int32[n_vals][N] (thfhe.lut.lhe_value; val_a: the masks, None: trivial samples), value val_index[s], or value s when n_vals == count, or the
        one value when n_vals == 1 -- into entry `address of s` of table table_index[s] (None: table 0) of n_tables tables that start from zero:
        d_rot + 2^d_tree - 1 external products per sample.  Returns (tab_a, tab_b) int32[n_tables][2^d_tree][N], TLWE samples in the layout of
        thfhe.lut.lhe_table: lhe_lookup(tset2, tab_b, tab_a=tab_a, ...) reads them."""
        N = self.params.N
        if not 0 <= int(d_tree) <= 6:
            raise ValueError("d_tree must be 0 .. 6")
        if int(n_tables) < 1:
            raise ValueError("n_tables must be at least 1")
        val_b = np.ascontiguousarray(val_b, np.int32)
        if val_b.size == 0 or val_b.size % N:
            raise ValueError(f"val_b: expected int32[n_vals][{N}]")
        if val_a is not None:
            val_a = np.ascontiguousarray(val_a, np.int32)
            if val_a.size != val_b.size:
                raise ValueError("val_a and val_b differ in size")
        first = int(first)
        count = tset.count - first if count is None else int(count)
        if first < 0 or count < 0:
            raise ValueError("first and count must not be negative")
        idx = [_index("val_index", val_index, count), _index("table_index", table_index, count)]
        tab_a = np.empty((int(n_tables), 1 << int(d_tree), N), np.int32)
        tab_b = np.empty_like(tab_a)
        _check(lib().thfhe_lhe_scatter(self.h, tset.h, first, count, int(d_tree), int(d_rot), _p32(val_a), _p32(val_b), val_b.size // N, _p32(idx[0]),
                                       int(n_tables), _p32(idx[1]), _p32(tab_a), _p32(tab_b)))
        return tab_a, tab_b

    # -- circuit bootstrapping: LWE gate outputs -> TGSW address bits (thfhe_cb_key_set, thfhe_circuit_bootstrap) -----------------
    def cb_key_set(self, level2_cloud_key, pks, t, basebit):
        """Upload the private key-switching key pks int32[2][D][t][2][N] (thfhe.keygen.gen_cb_key, from the level-2 ring key to this key's ring key)
        and name the level-2 context: an MKCloudKey of one party on this device whose LWE key is this key's (CB_PARAM_SETS).  It is kept alive for
        as long as this key.  A second call replaces both."""
        p = self.params
        pks = np.ascontiguousarray(pks, np.int32)
        if pks.ndim != 5 or pks.shape[0] != 2 or pks.shape[2:] != (int(t), 2, p.N):
            raise ValueError(f"pks: expected int32[2][D][{t}][2][{p.N}], got shape {pks.shape}")
        _check(lib().thfhe_cb_key_set(self.h, _p32(pks), pks.shape[1], int(t), int(basebit)))
        self._cb_level2, self._cb_D = level2_cloud_key, pks.shape[1]

    def cb_private_keyswitch(self, lwe2):
        """Stage B of circuit bootstrapping alone: lwe2 int32[count][l][D+1], LWE samples under the level-2 ring key (record (s, j) of m g_j) ->
        int32[count][2l][2][N], the TGSW rows of thfhe.keygen.SecretKeySet.tgsw_encrypt's layout."""
        D = getattr(self, "_cb_D", None)
        if D is None:
            raise ThfheError("no circuit-bootstrap key: call cb_key_set first")
        p = self.params
        lwe2 = np.ascontiguousarray(lwe2, np.int32)
        if lwe2.size % (p.l * (D + 1)) or lwe2.shape[-1] != D + 1:
            raise ValueError(f"lwe2: expected int32[count][{p.l}][{D + 1}], got shape {lwe2.shape}")
        count = lwe2.size // (p.l * (D + 1))
        out = np.empty((count, 2 * p.l, 2, p.N), np.int32)
        _check(lib().thfhe_cb_private_keyswitch(self.h, _p32(lwe2), count, _p32(out)))
        return out

    def cb_set_batch_threshold(self, min_inputs):
        """Inputs (records of a launch) from which the private key switch runs on the matrix cores; 0 restores the default.  No word depends on it."""
        _check(lib().thfhe_cb_set_batch_threshold(self.h, int(min_inputs)))

    def circuit_bootstrap(self, recs, d, return_words=False, one_rotation=False):
        """recs int32[count * d][n+1], gate-encoded records under this key's LWE key (sample-major: bit i of sample s is record s d + i) -> a TgswSet
        of count samples of d bits, device-resident, for lhe_cmux / lhe_lookup / lhe_wfa / lhe_demux / lhe_scatter and the leveled DAG entry.
        return_words: also the rows int32[count * d][2l][2][N], as (set, words).
        one_rotation: the l records of a bit from ONE level-2 rotation instead of l (THFHE_CB_ONE_ROTATION): other words, the same rotation noise,
        a theta = 2 or 4 times coarser mod-switch of the input -- for gate-encoded inputs (+-1/8) only."""
        l2 = getattr(self, "_cb_level2", None)
        if l2 is None:
            raise ThfheError("no circuit-bootstrap key: call cb_key_set first")
        p = self.params
        d = int(d)
        recs = _rec(recs, self.words)
        if d < 1 or recs.shape[0] == 0 or recs.shape[0] % d:
            raise ValueError(f"recs: expected int32[count * d][{self.words}] with d = {d}")
        count = recs.shape[0] // d
        words = np.empty((count * d, 2 * p.l, 2, p.N), np.int32) if return_words else None
        h = _vp()
        if one_rotation:
            _check(lib().thfhe_circuit_bootstrap_mode(self.h, l2.h, _p32(recs), count, d, CB_ONE_ROTATION, _p32(words), C.byref(h)))
        else:
            _check(lib().thfhe_circuit_bootstrap(self.h, l2.h, _p32(recs), count, d, _p32(words), C.byref(h)))
        tset = TgswSet._adopt(self, h, count, d)
        return (tset, words) if return_words else tset

    def cb_stage_a(self, recs, one_rotation=False):
        """Stage A of circuit bootstrapping alone: recs int32[count][n+1], gate-encoded records -> int32[count][l][D+1], record (s, j) an LWE sample
        of m g_j under the level-2 ring key: the input of cb_private_keyswitch.  one_rotation as in circuit_bootstrap."""
        l2, D = getattr(self, "_cb_level2", None), getattr(self, "_cb_D", None)
        if l2 is None:
            raise ThfheError("no circuit-bootstrap key: call cb_key_set first")
        recs = _rec(recs, self.words)
        out = np.empty((recs.shape[0], self.params.l, D + 1), np.int32)
        _check(lib().thfhe_cb_stage_a(self.h, l2.h, _p32(recs), recs.shape[0], CB_ONE_ROTATION if one_rotation else CB_PER_LEVEL, _p32(out)))
        return out

    def set_wfa_chunk(self, g):
        """States per workgroup of a step of lhe_wfa, 1 .. 64; 0: automatic.  No output word depends on it."""
        _check(lib().thfhe_set_wfa_chunk(self.h, int(g)))

    def set_tree_slice(self, max_candidates):
        """Level-1 candidates (samples x p_hi, x k for tree_lut_bootstrap_mvk) per slice of tree_lut_bootstrap(_mv, _mvk): bounds its workspace (8 KiB of packing scratch per candidate);
        also the output records (samples x q) per slice of mv_lut_bootstrap."""
        _check(lib().thfhe_set_tree_slice(self.h, int(max_candidates)))

    def set_ring4_threshold(self, max_jobs):
        """Remainders (batch mod 2048) above the cooperative threshold and <= max_jobs rotations use the four-wave ring kernel; 0 disables it."""
        _check(lib().thfhe_set_ring4_threshold(self.h, int(max_jobs)))

    def set_coop_threshold(self, max_jobs):
        """Remainders (batch mod 2048) of <= max_jobs rotations use the cooperative latency kernel; 0 disables it."""
        _check(lib().thfhe_set_coop_threshold(self.h, int(max_jobs)))

    def rotation_kernel_name(self, rotations):
        """The blind-rotation kernel that does most of a batch of `rotations`, as the library's launcher decides it (for profiles and bench.py)."""
        return self._kernel_name(lib().thfhe_rotation_kernel_name, int(rotations))


# ---- the reference's single-key gate API (gates.jl:15-177), batched over the leading axis -------------
def gate_nand(ck, x, y): return ck.gates(NAND, x, y)
def gate_or(ck, x, y): return ck.gates(OR, x, y)
def gate_and(ck, x, y): return ck.gates(AND, x, y)
def gate_xor(ck, x, y): return ck.gates(XOR, x, y)
def gate_xnor(ck, x, y): return ck.gates(XNOR, x, y)
def gate_nor(ck, x, y): return ck.gates(NOR, x, y)
def gate_andny(ck, x, y): return ck.gates(ANDNY, x, y)
def gate_andyn(ck, x, y): return ck.gates(ANDYN, x, y)
def gate_orny(ck, x, y): return ck.gates(ORNY, x, y)
def gate_oryn(ck, x, y): return ck.gates(ORYN, x, y)
def gate_mux(ck, x, y, z): return ck.gates(MUX, x, y, z)
def gate_not(ck, x): return ck.gates(NOT, x)


def gate_constant(ck, value):
    """gates.jl:91-93: noiseless trivial sample of +-1/8 (not encrypted)."""
    r = np.zeros(ck.words, np.int32)
    r[-1] = MU8 if value else -MU8
    return r


def bootstrap(ck, mu, x): return ck.bootstrap(x, mu)                              # bootstrap.jl:98-101
def bootstrap_wo_keyswitch(ck, mu, x): return ck.bootstrap_wo_keyswitch(x, mu)    # bootstrap.jl:75-88
def keyswitch(ck, u): return ck.keyswitch(u)                                      # keyswitch.jl:45-80


# ---- 3-gen multi-key -------------------------------------------------------------------------------------
class MKCloudKey(_EvalKey):
    """Evaluation context of the 3rd-generation multi-key scheme: the parties' TransformedBootstrapKeyPart_3gen
    (3gen_mk_internals.jl:45-56) and KeyswitchKey tables on one MI355X.

    bk_coeff: int64[P][n][4][l][N] (part_1..part_4 of every TGswSample_3gen, coefficient domain);
    ksk: int32[P][N][t][base-1][n+1].  Records are int32[P*n+1] = a[p*n+i], b (MKLweSample, mk_internals.jl:23-37).
    """

    _prefix = "thfhe_mk_"
    _tv_dtype = np.int64   # the 3-gen accumulator is Torus64
    _tgsw_set_class = MKTgswSet

    def __init__(self, params, bk_coeff, ksk, device=0):
        self.params = p = params
        bk = np.ascontiguousarray(bk_coeff, np.int64)
        ks = np.ascontiguousarray(ksk, np.int32)
        if bk.size != p.parties * p.n * 4 * p.l * p.N:
            raise ValueError("bk_coeff has the wrong size for these parameters")
        if ks.size != p.parties * p.N * p.ks_t * ((1 << p.ks_basebit) - 1) * (p.n + 1):
            raise ValueError("ksk has the wrong size for these parameters")
        h = _vp()
        _check(lib().thfhe_mk_ctx_create(C.byref(p), bk.ctypes.data_as(_i64p), _p32(ks), device, C.byref(h)))
        self._own(h, lib().thfhe_mk_ctx_destroy)
        self.words = p.parties * p.n + 1

    def bootstrap(self, x, mu=MU8_64):
        return self._bootstrap(x, mu)

    def set_pair_threshold(self, max_single_jobs):
        """Batches of <= max_single_jobs rotations run one gate per workgroup; larger ones two gates per workgroup."""
        _check(lib().thfhe_mk_set_pair_threshold(self.h, int(max_single_jobs)))

    # -- multi-value bootstrapping on Torus64 (thfhe_mk_mv_lut_bootstrap) ---------------------------------------------------
    def mv_lut_bootstrap(self, factors, x, y=None, z=None, *, tv0, weights=(1,), bias=0, table_index=None, out_bias=0):
        """q functions of one encrypted digit from ONE multi-key blind rotation: the base vector tv0 int64[N] (thfhe.lut.mv_base(step, N, torus_bits=64))
        is rotated by x = sum_q weights[q] * (x, y, z)[q] + (0, bias) at theta = 1; output j of sample s combines p extractions of the Torus64
        accumulator with the taps factors[table_index[s]][j] (thfhe.lut.mv_factors, mv_bool_factors), adds out_bias (a Torus64 word) to the body and
        converts once.  factors: int32[q][p] or int32[n_tables][q][p].  Returns int32[count, q, P*n+1]."""
        return self._mv(factors, x, y, z, tv0, weights, bias, table_index, True, _wrap64(out_bias))

    def mv_lut_bootstrap_wo_keyswitch(self, factors, x, y=None, z=None, *, tv0, weights=(1,), bias=0, table_index=None, out_bias=0):
        """mv_lut_bootstrap without the key switch: int32[count, q, N+1] records under the ring key."""
        return self._mv(factors, x, y, z, tv0, weights, bias, table_index, False, _wrap64(out_bias))

    def set_mv_slice(self, max_records):
        """Output records (samples x q) per slice of mv_lut_bootstrap and of an MV launch group: (N + 1) x 4 B of workspace each; default 4096."""
        _check(lib().thfhe_mk_set_mv_slice(self.h, int(max_records)))

    # -- packing key switch, encrypted tables and the two-digit tree on Torus64 ------------------------------------------------
    def pack_key_set(self, pk, t, basebit):
        """Upload the multi-key packing key pk int64[D][t][2^basebit - 1][2][N] (thfhe.keygen.gen_mk_pack_key): D = P*n packs key-switched records and
        gate outputs, D = N packs _wo_keyswitch records (the tree's key).  A second call replaces the key."""
        p = self.params
        R = (1 << int(basebit)) - 1
        pk = np.ascontiguousarray(pk, np.int64)
        if pk.ndim != 5 or pk.shape[1:] != (int(t), R, 2, p.N):
            raise ValueError(f"pk: expected int64[D][{t}][{R}][2][{p.N}], got shape {pk.shape}")
        _check(lib().thfhe_mk_pack_key_set(self.h, pk.ctypes.data_as(_i64p), pk.shape[0], int(t), int(basebit)))
        self._pack_D = pk.shape[0]

    def pack_boxes(self, recs, p):
        """p records -> one encrypted test vector (thfhe_mk_pack_boxes): recs int32[count][D+1] with D the packing key's, count a multiple of p.
        Returns (tv_a, tv_b) int64[count / p][N]: RLWE samples under the summed ring key, ready for lut_bootstrap_enc."""
        D = getattr(self, "_pack_D", None)
        if D is None:
            raise ValueError("pack_boxes: no packing key set (pack_key_set)")
        recs = _rec(recs, D + 1)
        p = int(p)
        tabs = recs.shape[0] // p if p > 0 else 0
        tv_a, tv_b = np.empty((tabs, self.params.N), np.int64), np.empty((tabs, self.params.N), np.int64)
        _check(lib().thfhe_mk_pack_boxes(self.h, _p32(recs), recs.shape[0], p, tv_a.ctypes.data_as(_i64p), tv_b.ctypes.data_as(_i64p)))
        return tv_a, tv_b

    def tree_lut_bootstrap(self, tv1, lo, hi, *, p_hi, weights_lo=(1,), bias_lo=0, theta=1, weights_hi=(1,), bias_hi=0, table_index=None):
        """Two-digit tree PBS (thfhe_mk_tree_lut_bootstrap): sample s gets f_table[s](hi, lo) as one record int32[count, P*n+1].  lo, hi: one record
        array or a tuple of 1 .. 3 (weighted by weights_lo / weights_hi); tv1: int64[n_tables][p_hi / theta][N]
        (thfhe.lut.tree_test_vectors(..., torus_bits=64)).  Needs a packing key with D = N (pack_key_set).  lut_bootstrap_enc takes int64 RLWE tables."""
        return self._tree((self.h,), tv1, lo, hi, p_hi, weights_lo, bias_lo, theta, weights_hi, bias_hi, table_index)

    def set_tree_slice(self, max_candidates):
        """Level-1 candidates (samples x p_hi) per slice of tree_lut_bootstrap and records per slice of pack_boxes: 2N x 8 B of workspace each;
        default 16384."""
        _check(lib().thfhe_mk_set_tree_slice(self.h, int(max_candidates)))

    # -- multi-value two-digit trees on Torus64 (thfhe_mk_tree_lut_bootstrap_mvk) -----------------------------------------------
    def tree_lut_bootstrap_mvk(self, factors, lo, hi, *, tv0, weights_lo=(1,), bias_lo=0, weights_hi=(1,), bias_hi=0, table_index=None, out_bias=0):
        """k functions of two encrypted digits in 1 + k rotations: out[s][j] = f_j(hi_s, lo_s) from ONE multi-value level-1 rotation on `lo`, the packing
        of its k p_hi candidates and k selections on `hi`.  tv0 int64[N], factors int32[k][p_hi][p_lo] or int32[n_tables][k][p_hi][p_lo]
        (thfhe.lut.tree_mvk_factors(..., torus_bits=64), tree_mvk_bool_factors); k p_hi <= 64; out_bias: a Torus64 word added to every candidate's body.
        Needs a packing key with D = N (pack_key_set).  Returns int32[count, k, P*n+1]."""
        lo_r, spec_lo, plo = self._lut_args(_as_tuple(lo), weights_lo, bias_lo, 1, "tree_lut_bootstrap_mvk (lo)")
        hi_r, spec_hi, phi = self._lut_args(_as_tuple(hi), weights_hi, bias_hi, 1, "tree_lut_bootstrap_mvk (hi)")
        _same_count(lo_r[0], hi_r[0])
        count = lo_r[0].shape[0]
        w = np.ascontiguousarray(factors, np.int32)
        if w.ndim == 3:
            w = w[None]
        if w.ndim != 4 or w.size == 0:
            raise ValueError("factors: expected int32[k][p_hi][p_lo] or int32[n_tables][k][p_hi][p_lo]")
        _, tv0, idx = self._mv_tables(w[0], tv0, table_index, count)
        out = np.empty((count, w.shape[1], self.words), np.int32)
        _check(lib().thfhe_mk_tree_lut_bootstrap_mvk(self.h, C.byref(spec_lo), C.byref(spec_hi), w.shape[2], w.shape[3], w.shape[1], self._ptv(tv0), _p32(w),
                                                     w.shape[0], _p32(idx), _wrap64(out_bias), plo[0], plo[1], plo[2], phi[0], phi[1], phi[2], _p32(out), count))
        return out

    def tree_lut_bootstrap_mv(self, factors, lo, hi, *, tv0, weights_lo=(1,), bias_lo=0, weights_hi=(1,), bias_hi=0, table_index=None, out_bias=0):
        """tree_lut_bootstrap_mvk with k = 1: 1 + 1 rotations whatever p_hi is.  factors int32[p_hi][p_lo] or int32[n_tables][p_hi][p_lo]
        (thfhe.lut.tree_mv_factors(..., torus_bits=64)).  Returns int32[count, P*n+1]."""
        w = np.ascontiguousarray(factors, np.int32)
        if w.ndim not in (2, 3) or w.size == 0:
            raise ValueError("factors: expected int32[p_hi][p_lo] or int32[n_tables][p_hi][p_lo]")
        w = w[None, None] if w.ndim == 2 else w[:, None]
        return self.tree_lut_bootstrap_mvk(w, lo, hi, tv0=tv0, weights_lo=weights_lo, bias_lo=bias_lo, weights_hi=weights_hi, bias_hi=bias_hi,
                                           table_index=table_index, out_bias=out_bias)[:, 0]

    def set_pack_wide_threshold(self, min_records):
        """Packing calls of at least min_records records (per slice) run mk_pack_rows_wide_kernel, smaller ones mk_pack_rows_kernel; 0 = never the
        wide one.  Both give the same words."""
        _check(lib().thfhe_mk_set_pack_wide_threshold(self.h, int(min_records)))

    def pack_kernel_name(self, count):
        """The packing-rows kernel a packing of `count` records is dispatched to, as mk_pack_enqueue in thfhe_mk.hip decides it."""
        return self._kernel_name(lib().thfhe_mk_pack_kernel_name, int(count))

    def dag_run_mv_batch(self, input_records, nodes, specs=(), tv=None, mvs=(), mv_tv0=None, mv_factors=None, mv_out_bias=None, out_wires=None):
        """dag_run_lut_batch with multi-value nodes (thfhe_mk_dag_run_mv_batch).  mvs: MvSpec or (lo, hi, p, q, k, base, factors_off,
        n_tables) tuples (hi None, k 1); mv_tv0: int64[n_bases][N] base vectors; mv_factors: int32[words], the taps of every spec; mv_out_bias: one
        Torus64 word per spec (None: 0).  specs and tv may be absent."""
        def families():
            N = self.params.N
            sp = (LutSpec * len(specs))(*[_lut_spec(s) for s in specs]) if len(specs) else None
            t = None if tv is None else np.ascontiguousarray(tv, np.int64).reshape(-1, N)
            mv = _mv_specs(mvs)
            tv0 = None if mv_tv0 is None else np.ascontiguousarray(mv_tv0, np.int64).reshape(-1, N)
            fac = None if mv_factors is None else np.ascontiguousarray(mv_factors, np.int32).reshape(-1)
            ob = None if mv_out_bias is None else np.array([_wrap64(v) for v in np.ravel(mv_out_bias)], np.int64)
            if ob is not None and ob.shape[0] != len(mvs):
                raise ValueError(f"mv_out_bias holds {ob.shape[0]} words for {len(mvs)} specs")
            p64 = lambda a: None if a is None else a.ctypes.data_as(_i64p)
            return (sp, len(specs), p64(t), 0 if t is None else t.shape[0], mv, len(mvs), p64(tv0), 0 if tv0 is None else tv0.shape[0], _p32(fac),
                    0 if fac is None else fac.shape[0], p64(ob))
        return self._dag_run("dag_run_mv_batch", lib().thfhe_mk_dag_run_mv_batch, (self.h,), input_records, nodes, 6, families, out_wires)

    def dag_run_dense_batch(self, input_records, nodes, dense_layers=(), dense_words=None, dense_wires=None, **kw):
        """dag_run_tree_batch with dense-layer nodes (thfhe_mk_dag_run_dense_batch): CloudKey.dag_run_dense_batch on int64 tables and
        records of P n + 1 words.  Without the three dense arguments the call is dag_run_tree_batch through the new entry."""
        fam, keep = _dense_families(dense_layers, dense_words, dense_wires)
        return self.dag_run_tree_batch(input_records, nodes, _dense=(None if fam is None else C.byref(fam),), **kw)

    def dag_run_tree_batch(self, input_records, nodes, specs=(), tv=None, enc_a=None, enc_b=None, trees=(), tv1=None, mvs=(), mv_tv0=None, mv_factors=None,
                           mv_out_bias=None, out_wires=None, _dense=None):
        """dag_run_mv_batch with encrypted-table, tree and multi-value tree nodes (thfhe_mk_dag_run_tree_batch).  enc_a, enc_b:
        int64[n_enc][N] RLWE tables; trees: TreeSpec or (lo, hi, p_hi) tuples; tv1: int64[rows][N] level-1 rows; mvs entries may carry hi and k
        (TREE_MV).  TREE and TREE_MV rows need a packing key with D = N (pack_key_set); SELECT rows are refused."""
        def families():
            N = self.params.N
            p64 = lambda a: None if a is None else a.ctypes.data_as(_i64p)
            a64 = lambda a: None if a is None else np.ascontiguousarray(a, np.int64).reshape(-1, N)
            sp = (LutSpec * len(specs))(*[_lut_spec(s) for s in specs]) if len(specs) else None
            t, ea, eb, rows, tv0 = a64(tv), a64(enc_a), a64(enc_b), a64(tv1), a64(mv_tv0)
            if (ea is None) != (eb is None) or (ea is not None and ea.shape != eb.shape):
                raise ValueError("enc_a and enc_b: give both, int64[n_enc][N]")
            tr = (TreeSpec * len(trees))(*[t if isinstance(t, TreeSpec) else TreeSpec(_lut_spec(t[0] or _NO_SPEC), _lut_spec(t[1]), int(t[2])) for t in trees]) if len(trees) else None
            mv = _mv_specs(mvs)
            fac = None if mv_factors is None else np.ascontiguousarray(mv_factors, np.int32).reshape(-1)
            ob = None if mv_out_bias is None else np.array([_wrap64(v) for v in np.ravel(mv_out_bias)], np.int64)
            if ob is not None and ob.shape[0] != len(mvs):
                raise ValueError(f"mv_out_bias holds {ob.shape[0]} words for {len(mvs)} specs")
            n = lambda a: 0 if a is None else a.shape[0]
            return (sp, len(specs), p64(t), n(t), p64(ea), p64(eb), n(ea), tr, len(trees), p64(rows), n(rows), mv, len(mvs), p64(tv0), n(tv0), _p32(fac),
                    n(fac), p64(ob)) + (() if _dense is None else (_dense[0],))
        fn = lib().thfhe_mk_dag_run_tree_batch if _dense is None else lib().thfhe_mk_dag_run_dense_batch
        return self._dag_run("dag_run_tree_batch", fn, (self.h,), input_records, nodes, 6, families, out_wires)

    # -- leveled CMux and table lookup on the ring of degree 2048 (thfhe_mk_tgsw_set_create, thfhe_mk_lhe_cmux, thfhe_mk_lhe_lookup):
    #    the bodies are _EvalKey's, the wording about this ring's layout and sizes is kept here ---------------------------------------------------
    def tgsw_set(self, samples, d):
        """Device-resident address bits: samples int64[count * d][4][l][N] (MKSecretKeySet.tgsw_encrypt of the bits, sample-major: bit i of sample s
        is row s d + i), kept as spectra, 1 MiB per bit on the CB sets.  Returns an MKTgswSet: close() it (or use `with`) before this key is closed.
        One-party contexts on the batched N = 2048 path only (CB_PARAM_SETS)."""
        return super().tgsw_set(samples, d)

    def lhe_cmux(self, tset, bit, d1_a, d1_b, d0_a, d0_b):
        """(out_a, out_b) int64[count][N]: sample s gets d0[s] + C_(s,bit) (.) (d1[s] - d0[s]) -- d1 where its address bit `bit` is 1, else d0."""
        return super().lhe_cmux(tset, bit, d1_a, d1_b, d0_a, d0_b)

    def lhe_lookup(self, tset, tab_b, *, d_tree, d_rot, theta=1, tab_a=None, table_index=None, first=0, count=None):
        """Leveled lookup of samples first .. first+count-1 of the set (default: all from `first`) in the table tab_b int64[n_tables][2^d_tree][N]
        (thfhe.lut.lhe_table with N = 2048, torus_bits = 64; tab_a: the masks of an encrypted table, None: public): d_tree + d_rot CMuxes, theta
        functions per sample.  Returns key-switched records int32[count, theta, n+1]."""
        return self._lhe_lookup(tset, tab_b, d_tree, d_rot, theta, tab_a, table_index, first, count, True)

    def rotation_kernel_name(self, rotations):
        """The blind-rotation kernel a batch of `rotations` is dispatched to, as mk_launch_rotation in thfhe_mk.hip decides it."""
        return self._kernel_name(lib().thfhe_mk_rotation_kernel_name, int(rotations))


class PolyMac(_Handle):
    """Device engine for the key-generation products (thfhe_pm_mac): out[j] = addend[j] + sum_terms sign * small[s] (*) torus[t], exact."""

    def __init__(self, N, torus_bits, device=0):
        h = _vp()
        _check(lib().thfhe_pm_ctx_create(device, N, torus_bits, C.byref(h)))
        self._own(h, lib().thfhe_pm_ctx_destroy)
        self.N, self.dtype = N, (np.int32 if torus_bits == 32 else np.int64)

    def mac(self, small, torus, terms, n_out, addend=None):
        small = np.ascontiguousarray(small, np.int32).reshape(-1, self.N)
        torus = np.ascontiguousarray(torus).view(self.dtype).reshape(-1, self.N)
        terms = np.ascontiguousarray(terms, np.int32).reshape(-1, 4)
        out = np.empty((n_out, self.N), self.dtype)
        if addend is not None:
            addend = np.ascontiguousarray(addend).view(self.dtype).reshape(n_out, self.N)
        _check(lib().thfhe_pm_mac(self.h, _p32(small), small.shape[0], torus.ctypes.data_as(_vp), torus.shape[0], _p32(terms), terms.shape[0],
                                  addend.ctypes.data_as(_vp) if addend is not None else None, out.ctypes.data_as(_vp), n_out))
        return out


class CCSCloudKey(_Handle):
    """MKCloudKey of the CCS scheme (mk_api.jl:392-408): MKBootstrapKey (uni-encrypted key bits, public keys, shared key) and the
    parties' KeyswitchKeys on one MI355X.  bk int32[P][n][3][l][N] (d1, f0, f1), pk int32[P][l][N], crs int32[l][N], ksk as MKCloudKey."""

    def __init__(self, params, bk, pk, crs, ksk, device=0):
        self.params = p = params
        arrs = [np.ascontiguousarray(a, np.int32) for a in (bk, pk, crs, ksk)]
        sizes = (p.parties * p.n * 3 * p.l * p.N, p.parties * p.l * p.N, p.l * p.N, p.parties * p.N * p.ks_t * ((1 << p.ks_basebit) - 1) * (p.n + 1))
        if any(a.size != s for a, s in zip(arrs, sizes)):
            raise ValueError("key table has the wrong size for these parameters")
        h = _vp()
        _check(lib().thfhe_ccs_ctx_create(C.byref(p), *[_p32(a) for a in arrs], device, C.byref(h)))
        self._own(h, lib().thfhe_ccs_ctx_destroy)
        self.words = p.parties * p.n + 1

    def gates(self, op, x, y):
        x, y = _rec(x, self.words), _rec(y, self.words)
        _same_count(x, y)
        out = np.empty_like(x)
        _check(lib().thfhe_ccs_gates(self.h, op, _p32(x), _p32(y), _p32(out), x.shape[0]))
        return out

    def bootstrap(self, x, mu=MU8):
        x = _rec(x, self.words)
        out = np.empty_like(x)
        _check(lib().thfhe_ccs_bootstrap(self.h, mu, _p32(x), _p32(out), x.shape[0]))
        return out

    def rotation_kernel_name(self):
        """The blind-rotation kernel of this context (thfhe_ccs_ctx_create: more than 8 parties or 8 levels take the wide kernel)."""
        return self._kernel_name(lib().thfhe_ccs_rotation_kernel_name)


def mk_gate_nand(ck, x, y): return ck.gates(NAND, x, y)          # mk_gates.jl:7-13 (CCS scheme)
def mk_bootstrap(ck, mu, x): return ck.bootstrap(x, mu)         # mk_internals.jl:855-858


# the reference's 3-gen gate API (3gen_mk_gates.jl:8-150); `bk` is the MKCloudKey (it holds bk and ks together)
def mk_gate_nand_3gen(bk, x, y): return bk.gates(NAND, x, y)
def mk_gate_or_3gen(bk, x, y): return bk.gates(OR, x, y)
def mk_gate_and_3gen(bk, x, y): return bk.gates(AND, x, y)
def mk_gate_xor_3gen(bk, x, y): return bk.gates(XOR, x, y)
def mk_gate_3and_3gen(bk, x, y, z): return bk.gates(AND3, x, y, z)
def mk_gate_mux_3gen(bk, x, y, z): return bk.gates(MUX, x, y, z)
def mk_gate_not_3gen(bk, x): return bk.gates(NOT, x)
def mk_bootstrap_3gen(bk, mu, x): return bk.bootstrap(x, mu)   # 3gen_mk_internals.jl:112-116
