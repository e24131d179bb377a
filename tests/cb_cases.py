"""The real-key cases of circuit bootstrapping that tests/test_cb_host.py runs on the CPU model and tests/test_gpu_cb.py on the device (DESIGN.md
section 4.21): SK-128 and SK-80 with n reduced to 16, the level-2 set (CB-128 / CB-80, n = 16) at its full ring degree 2048 sharing the LWE key,
the private key at full D = 2048 with (t, basebit) = (7, 4) and sigma_pks = 2^-31.  Address bits are NAND outputs: 8 samples x 3 bits for the
lookup (every address once) and 4 samples x 6 bits for the comparison (two operands of 3 bits, two pairs equal).  Keys, inputs and model outputs
are built once per process and shared; `device` only chooses where the key generators multiply (both give the same words)."""
import numpy as np

import cb_reference as CB
import lhe_reference as LR
import wfa_reference as WR
from support import N, pmap

T, BASEBIT, SIGMA_PKS = 7, 4, 2.0**-31
N_RED, D2 = 16, 2048
P_OUT = 8
ADDR = np.array([6, 1, 7, 0, 3, 5, 2, 4])            # lookup: every address of the 8-entry table
OP_A, OP_B = np.array([5, 3, 0, 7]), np.array([5, 4, 0, 6])   # comparison: pairs 0 and 2 are equal
LEVEL2 = {"SK-128": "CB-128", "SK-80": "CB-80"}


class Keys:
    def __init__(self, O, name, device=None):
        import thfhe
        from thfhe import keygen
        self.name, self.sig, self.sig2 = name, thfhe.SIGMAS[name], thfhe.CB_SIGMAS[LEVEL2[name]]
        self.tp = thfhe.make_params(name, n=N_RED)
        self.K = keygen.SecretKeySet(self.tp, seed=0x5EED0C00 + self.tp.l, sigma_lwe=self.sig["lwe"], sigma_bk=self.sig["bk"], sigma_ks=self.sig["ks"])
        self.tp2 = thfhe.make_params(**dict(thfhe.CB_PARAM_SETS[LEVEL2[name]], n=N_RED))
        self.K2 = keygen.MKSecretKeySet(self.tp2, seed=0x5EED0C10 + self.tp.l, sigma_lwe=self.sig2["lwe"], sigma_bk=self.sig2["bk"], sigma_ks=self.sig2["ks"],
                                        device=device, lwe_keys=self.K.lwe_key[None, :])
        self.z2 = self.K2.rlwe_keys[0]
        self.pks = keygen.gen_cb_key(np.random.default_rng(0x5EED0C20 + self.tp.l), self.z2, self.K.rlwe_key, T, BASEBIT, SIGMA_PKS, device=device)
        self.p = O.make_params(name, n=N_RED)
        self.orc = O.Oracle(self.p, self.K.bk, self.K.ksk)
        self.p2 = O.make_params(**self.tp2.as_dict())
        self.orc2 = O.MKOracle(self.p2, self.K2.bk, self.K2.ksk)

    def sigma_row(self):
        z2n = float((self.z2.astype(np.float64) ** 2).sum())
        sa = CB.sigma_a(N_RED, self.tp2.l, self.tp2.Bgbit, D2, z2n, self.sig2["bk"])
        return CB.sigma_row(D2, T, BASEBIT, SIGMA_PKS, z2n, sa)


_made = {}


def keys(O, name, device=None):
    if ("keys", name) not in _made:
        _made["keys", name] = Keys(O, name, device)
    return _made["keys", name]


def _nand_records(S, O, want_bits, seed):
    """gate-encoded records of `want_bits` as outputs of a NAND layer on fresh encryptions (x random, y chosen so that NAND(x, y) is the bit)"""
    want = np.asarray(want_bits).astype(bool).reshape(-1)
    x = np.random.default_rng(seed).integers(0, 2, want.shape[0]).astype(bool)
    x |= ~want                                  # NAND = 0 needs x = y = 1
    y = np.where(want, ~x, True)
    assert np.array_equal(~(x & y), want)
    recs = S.orc.gates(O.NAND, S.K.encrypt(x, seed + 1), S.K.encrypt(y, seed + 2))
    assert np.array_equal(S.K.decrypt(recs), want)
    return recs


def case(O, name, device=None):
    """dict: recs (the 48 NAND outputs; SK-80: the 24 of the lookup), bits, rows (the model's TGSW rows), and for the lookup and the comparison the
    tables, the plain results and the model's key-switched records -- the model has decoded every one of them by the time this returns"""
    if ("case", name) in _made:
        return _made["case", name]
    from thfhe import circuits, lut
    S = keys(O, name, device)
    l, Bgbit = S.tp.l, S.tp.Bgbit
    bits_lk = lut.lhe_address_bits(ADDR, 3)
    ops = np.concatenate([(OP_A[:, None] >> np.arange(3)) & 1, (OP_B[:, None] >> np.arange(3)) & 1], axis=1).reshape(-1)   # sample-major: a0 a1 a2 b0 b1 b2
    bits = np.concatenate([bits_lk, ops]) if name == "SK-128" else bits_lk
    recs = _nand_records(S, O, bits, 0xCB00 + l)
    rows = CB.circuit_bootstrap(S.orc2, S.pks, recs, l, Bgbit, T, BASEBIT)
    c = dict(recs=recs, bits=bits, rows=rows)
    # lookup: d_tree = 1, d_rot = 2 in an 8-entry public table at modulus 8
    table = np.random.default_rng(0xCB10).integers(0, P_OUT, 8)
    tab = lut.lhe_table(table, 1, 2, 1, encode=lambda v: lut.encode(v, P_OUT))
    Cs = rows[:24].reshape(8, 3, 2 * l, 2, N)
    ref = np.stack(pmap(lambda s: LR.lookup(S.orc, Cs[s], None, tab, 1, 2, 1), range(8)))
    assert np.array_equal(lut.decode(S.K.phase(ref).reshape(8), P_OUT), table[ADDR]), "the model itself must decode every lookup"
    c.update(table=table, tab=tab, lookup=ref)
    if name == "SK-128":
        # comparison: wfa_equal(3) on one set of d = 6 holding a (bits 0 .. 2) and b (bits 3 .. 5) of every sample
        trans, _, fin, start = circuits.wfa_equal(3)
        step_bit = np.array([3 * (j & 1) + (j >> 1) for j in range(6)], np.int32)
        fin_b = lut.wfa_finals(fin, 1, encode=lambda v: lut.encode(v, P_OUT))
        Cw = rows[24:].reshape(4, 6, 2 * l, 2, N)
        wfa = np.stack(pmap(lambda s: WR.wfa(S.orc, [Cw[s]], trans, step_bit, None, fin_b, 1, start), range(4)))   # [4][n_out = 1][theta = 1][n+1]
        want = (OP_A == OP_B).astype(np.int64)
        assert np.array_equal(lut.decode(S.K.phase(wfa).reshape(4), P_OUT), want), "the model itself must decode every comparison"
        c.update(aut=(trans, step_bit, fin_b, start), wfa=wfa, equal=want)
    _made["case", name] = c
    return c


def drawn(case, bits, seed, pool=None):
    """(recs, idx): a batch of `bits` records drawn from the first `pool` records of the case (default: all of them), idx = rng.integers(0, pool,
    bits) on a fixed seed.  Every stage is a deterministic function of one record, so the model of the batch is case["rows"][idx].  The draw is
    random, not periodic: an offset wrong by a multiple of the pool size cannot hide."""
    pool = len(case["recs"]) if pool is None else int(pool)
    assert 1 <= pool <= len(case["recs"])
    idx = np.random.default_rng(seed).integers(0, pool, int(bits))
    return np.ascontiguousarray(case["recs"][idx]), idx


# The batch boundaries that tests/test_gpu_cb_slices.py is sized by: name -> (value, file under torus-fhe_amd/csrc, the defining line as a regular
# expression whose one group is the value).  tests/test_cb_host.py reads the files and asserts the values, so that a changed constant fails there
# and does not silently move the GPU cases off the boundaries.
BOUNDARIES = {
    "bit slice": (2048, "thfhe_cb_host.h", r"constexpr size_t kCbSliceBits = (\d+);"),                    # bits per slice of cb_fill
    "inputs per launch": (4096, "thfhe_cb.h", r"constexpr long kCbMaxLaunchInputs = (\d+);"),             # cb_enqueue: launches of 4096 // l * l inputs
    "stage-B host slice": (2048, "thfhe_cb_host.h", r"S_max = std::min<size_t>\(count, std::max\(1, (\d+) / l\)\);"),   # cb_private_keyswitch: 2048 // l samples
    "input tile": (256, "thfhe_cb.h", r"\(int\)\(\(G \+ 255\) / (\d+)\), 1\};"),                          # CbmArgs.gtiles: inputs per workgroup of the matrix-core kernel
    "pair threshold": (256, "thfhe_mk.hip", r"long pair_threshold = (\d+);"),                             # level-2 rotations per launch above which two jobs share a workgroup
}
SLICE_BITS, LAUNCH_INPUTS, HOST_SLICE_INPUTS, TILE_INPUTS, PAIR_THRESHOLD = (BOUNDARIES[k][0] for k in (
    "bit slice", "inputs per launch", "stage-B host slice", "input tile", "pair threshold"))


def row_noise(S, rows, bits):
    """std of phase - message over all coefficients of all rows (torus units)"""
    return float(CB.row_errors(S.K, rows, bits, S.tp.l, S.tp.Bgbit).std()) / 2.0**32
