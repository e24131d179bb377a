"""The named-set cases of the leveled DAG nodes, shared by tests/test_gpu_dag_lhe.py and the model-only noise test of
tests/test_dag_lhe_host.py -- TEST INFRASTRUCTURE ONLY.  Keys, inputs, TGSW samples and the model's wires are made once per process and per case on
fixed seeds, so the CPU test measures the noise of exactly the wires the GPU test compares word for word."""
import numpy as np

import dag_lhe_reference as DL
from support import N, pmap

NAND, XOR, AND, OR = 0, 3, 2, 1
SIGMA_GATHER = 4.0e-3      # sqrt(2) sigma_ks of SK-128: what a gathered wire carries, as a SELECT output does
_made = {}


class Keys:
    """key material of a named set on the seeds of tests/test_gpu_lhe.py, its CPU oracle and a packing key at the ring's noise"""
    def __init__(self, O, name):
        import thfhe
        from thfhe import keygen
        self.name, self.sig = name, thfhe.SIGMAS[name]
        self.tp = thfhe.make_params(name)
        self.K = keygen.SecretKeySet(self.tp, seed=0x5EED0100 + self.tp.n, sigma_lwe=self.sig["lwe"], sigma_bk=self.sig["bk"], sigma_ks=self.sig["ks"])
        self.p = O.make_params(name)
        self.orc = O.Oracle(self.p, self.K.bk, self.K.ksk)
        self.pk = keygen.gen_pack_key(np.random.default_rng(0x7EE0100 + self.tp.n), self.K.lwe_key, self.K.rlwe_key, self.p.ks_t, self.p.ks_basebit, self.sig["bk"])

    def tgsw(self, bits, seed):
        b = np.asarray(bits)
        return self.K.tgsw_encrypt(b.reshape(-1), seed=seed).reshape(b.shape[0], b.shape[1], 2 * self.p.l, 2, N)

    def model(self, cir, x, sets):
        return np.stack(pmap(lambda q: DL.evaluate(self.orc, cir, x[q], [C[q] for C in sets], self.pk, self.p.ks_t, self.p.ks_basebit), range(x.shape[0])))


def keys(O, name):
    if name not in _made:
        _made[name] = Keys(O, name)
    return _made[name]


def array_read(O, name="SK-128", count=8):
    """16 gate outputs over 8 input bits; lhe_array_read of the first 8 at (d_tree, d_rot) = (1, 2) at address q of instance q, and of all 16 at (1, 3)
    at address 2 q + 1.  Returns dict(S, cir, x, bits, sets, read8, read16, a8, a16, want (the plain gate outputs), ref (the model's wires))."""
    key = ("array_read", name, count)
    if key not in _made:
        from thfhe import circuits as CI
        import lhe_reference as LR
        S = keys(O, name)
        rng = np.random.default_rng(9100)
        cir = CI.Circuit()
        x = cir.inputs(8)
        g = [cir.gate((NAND, XOR, AND, OR)[i % 4], x[i % 8], x[(3 * i + 1) % 8]) for i in range(16)]
        read8 = CI.lhe_array_read(cir, g[:8], 0, 1, 2)
        read16 = CI.lhe_array_read(cir, g, 1, 1, 3)
        bits = rng.integers(0, 2, (count, 8))
        recs = np.stack([S.K.encrypt(bits[q], seed=9200 + q) for q in range(count)])
        a8, a16 = np.arange(count) % 8, (2 * np.arange(count) + 1) % 16
        sets = [S.tgsw(LR.address_bits(a8, 3), 9300), S.tgsw(LR.address_bits(a16, 4), 9301)]
        want = np.stack([CI.simulate(_gates_only(cir, 16), bits[q].astype(bool))[8:24] for q in range(count)])
        _made[key] = dict(S=S, cir=cir, x=recs, sets=sets, read8=read8, read16=read16, a8=a8, a16=a16, want=want, ref=S.model(cir, recs, sets))
    return _made[key]


def _gates_only(cir, n):
    from thfhe import circuits as CI
    c = CI.Circuit()
    c.n_inputs, c.gates = cir.n_inputs, cir.gates[:n]
    return c


def noise_std(S, recs, bits):
    """std of phase - encode(+-1/8) of gate-bit records, in torus units"""
    err = (S.K.phase(recs).astype(np.int64) - np.where(np.asarray(bits, bool), 1 << 29, -(1 << 29)) + 2**31) % 2**32 - 2**31
    return float(err.std()) / 2.0**32


def mux_max(O, name="SK-128", count=8, width=8):
    """wfa_mux_max at `width` bits on `count` pairs: the numbers as gate bits (MSB first) and as TGSW bits.  Returns dict(S, cir, x, sets, out, A, B, ref)."""
    key = ("mux_max", name, count, width)
    if key not in _made:
        from thfhe import circuits as CI
        S = keys(O, name)
        rng = np.random.default_rng(9400)
        A, B = rng.integers(0, 1 << width, count), rng.integers(0, 1 << width, count)
        A[0], B[0] = B[1], B[1]                       # an equal pair: a < b is false
        cir = CI.Circuit()
        a, b = cir.inputs(width), cir.inputs(width)
        out = CI.wfa_mux_max(cir, a, b, [0, 1], width)
        msb = lambda v: [(int(v) >> (width - 1 - i)) & 1 for i in range(width)]
        recs = np.stack([S.K.encrypt(msb(A[q]) + msb(B[q]), seed=9500 + q) for q in range(count)])
        sets = [S.tgsw(b_, 9600 + i) for i, b_ in enumerate(CI.wfa_pair_bits(A, B, width))]
        _made[key] = dict(S=S, cir=cir, x=recs, sets=sets, out=out, A=A, B=B, ref=S.model(cir, recs, sets))
    return _made[key]


def smallest(O, name):
    """one GATHER at (0, 1) over two gate outputs, 2 instances: the smallest shape, for the other named sets"""
    key = ("smallest", name)
    if key not in _made:
        from thfhe import circuits as CI
        import lhe_reference as LR
        S = keys(O, name)
        cir = CI.Circuit()
        x = cir.inputs(3)
        g = [cir.gate(NAND, x[0], x[1]), cir.gate(XOR, x[1], x[2])]
        out = cir.lhe_gather(0, g[0], 0, 1)
        bits = np.array([[1, 1, 0], [0, 1, 1]])
        recs = np.stack([S.K.encrypt(bits[q], seed=9700 + q) for q in range(2)])
        addr = np.array([1, 0])
        sets = [S.tgsw(LR.address_bits(addr, 1), 9800)]
        want = np.array([[not (b[0] and b[1]), b[1] != b[2]] for b in bits])[np.arange(2), addr]
        _made[key] = dict(S=S, cir=cir, x=recs, sets=sets, out=out, want=want, ref=S.model(cir, recs, sets))
    return _made[key]
