"""Leveled table lookup under real keys (pytest -m gpu): SK-128, SK-80 and SK-lib at full size.  The address bits are TGSW
samples of SecretKeySet.tgsw_encrypt at the set's bootstrapping-key noise; every output word is compared with the model composed from the CPU
oracle's exact pieces (lhe_reference.py), and every sample must decrypt to its table entry: at 64 levels (padding bit) on the ring-key records
of the _wo_keyswitch entry, at p_out = 8 after the key switch.  The model alone, run on the CPU on these seeds, decrypts every case at those
encodings (the figures are in DESIGN 4.15), so nothing was narrowed.

Noise.  One CMux adds sigma_1 = sqrt(2 l N Bg^2 / 12) sigma_bk per coefficient (SK-128: 8.6e-5), d of them sqrt(d) sigma_1.  The test prints the
measured standard deviation of phase - encode over the _wo_keyswitch outputs and asserts it inside [0.5, 2] x the prediction (few samples, small
d); failure rates are not measured."""
import math

import numpy as np
import pytest

import lhe_reference as LR
from support import N, pmap

pytestmark = pytest.mark.gpu


class Keys:
    def __init__(self, O, name):
        import thfhe
        from thfhe import keygen
        self.name, self.sig = name, thfhe.SIGMAS[name]
        self.tp = thfhe.make_params(name)
        self.K = keygen.SecretKeySet(self.tp, seed=0x5EED0100 + self.tp.n, sigma_lwe=self.sig["lwe"], sigma_bk=self.sig["bk"], sigma_ks=self.sig["ks"])
        self.p = O.make_params(name)
        self.orc = O.Oracle(self.p, self.K.bk, self.K.ksk)
        self.ck = thfhe.CloudKey(self.tp, self.K.bk, self.K.ksk, device=0)

    def sigma_cmux(self):
        return math.sqrt(2 * self.p.l * N * 4.0 ** self.p.Bgbit / 12) * self.sig["bk"]

    def case(self, seed, count, d_tree, d_rot, theta, p_out, n_tables=1):
        """addresses, integer tables, their TGSW samples, the table at modulus p_out as a public and as an encrypted table"""
        from thfhe import lut
        rng = np.random.default_rng(seed)
        d = d_tree + d_rot
        addr = rng.integers(0, 1 << d, count)
        f = rng.integers(0, p_out, (n_tables, theta, 1 << d))
        tab = np.stack([lut.lhe_table(ft, d_tree, d_rot, theta, encode=lambda v: lut.encode(v, p_out)) for ft in f])
        Cs = self.K.tgsw_encrypt(lut.lhe_address_bits(addr, d), seed=seed + 1).reshape(count, d, 2 * self.p.l, 2, N)
        enc = lut.encrypt_table(self.K.rlwe_key, tab, self.sig["bk"], rng)
        return addr, f, tab, Cs, enc

    def check(self, count, d_tree, d_rot, theta, seed, label):
        """one lookup, encrypted table: word for word against the model, decrypt-exact; returns the measured noise std (torus units)"""
        from thfhe import lut
        kw = dict(d_tree=d_tree, d_rot=d_rot, theta=theta)
        addr, f, tab64, Cs, enc64 = self.case(seed, count, d_tree, d_rot, theta, 64)
        _, f8, tab8, _, enc8 = self.case(seed, count, d_tree, d_rot, theta, 8)
        want = f[0][:, addr].T
        ref = np.stack(pmap(lambda s: LR.lookup_wo_keyswitch(self.p, Cs[s], enc64[0][0], enc64[1][0], d_tree, d_rot, theta), range(count)))
        ph = self.K.ring_phase(ref).reshape(count, theta)
        assert np.array_equal(lut.decode(ph, 64), want), "the model itself must decrypt every case"
        ref8 = np.stack(pmap(lambda s: LR.lookup(self.orc, Cs[s], enc8[0][0], enc8[1][0], d_tree, d_rot, theta), range(count)))
        assert np.array_equal(lut.decode(self.K.phase(ref8).reshape(count, theta), 8), f8[0][:, addr].T), "the model itself must decrypt every case"
        with self.ck.tgsw_set(Cs, d_tree + d_rot) as ts:
            u = self.ck.lhe_lookup_wo_keyswitch(ts, enc64[1], tab_a=enc64[0], **kw)
            got8 = self.ck.lhe_lookup(ts, enc8[1], tab_a=enc8[0], **kw)
            pub = self.ck.lhe_lookup_wo_keyswitch(ts, tab64, **kw)
            triv = self.ck.lhe_lookup_wo_keyswitch(ts, tab64, tab_a=np.zeros_like(tab64), **kw)
        assert np.array_equal(u, ref), np.argwhere(u != ref)[:6].tolist()
        assert np.array_equal(got8, ref8), np.argwhere(got8 != ref8)[:6].tolist()
        assert np.array_equal(lut.decode(self.K.ring_phase(u).reshape(count, theta), 64), want)
        assert np.array_equal(lut.decode(self.K.phase(got8).reshape(count, theta), 8), f8[0][:, addr].T)
        assert np.array_equal(pub, triv), "a public table equals the encrypted table (0, tab_b) word for word"
        assert np.array_equal(lut.decode(self.K.ring_phase(pub).reshape(count, theta), 64), want)
        err = (self.K.ring_phase(u).reshape(count, theta).astype(np.int64) - lut.encode(want, 64).astype(np.int64) + 2**31) % 2**32 - 2**31
        std = float(err.std()) / 2.0**32
        pred = math.sqrt(d_tree + d_rot) * self.sigma_cmux()
        print(f"\nlhe noise {self.name} {label}: measured std {std:.3e} over {err.size} outputs (GPU == CPU model word for word), "
              f"predicted sqrt({d_tree + d_rot}) x {self.sigma_cmux():.3e} = {pred:.3e}, ratio {std / pred:.2f}")
        assert 0.5 * pred <= std <= 2 * pred
        return std


@pytest.fixture(scope="module")
def sk128(O):
    s = Keys(O, "SK-128")
    yield s
    s.ck.close()


def test_sk128_32_samples_16_bit_address(sk128):
    sk128.check(32, 6, 10, 1, 4100, "(6, 10, 1)")


def test_sk128_16_samples_four_functions(sk128):
    sk128.check(16, 2, 8, 4, 4200, "(2, 8, 4)")


def test_sk128_lookup_feeds_gates_and_lut_bootstrap(sk128):
    import thfhe
    from thfhe import lut
    S = sk128
    rng = np.random.default_rng(4300)
    d_tree, d_rot, count = 2, 8, 12
    addr = rng.integers(0, 1 << 10, (2, count))
    bits = rng.integers(0, 2, 1 << 10)
    digits = rng.integers(0, 4, 1 << 10)
    tab_bool = lut.lhe_table(np.where(bits == 1, lut.MU8, -lut.MU8), d_tree, d_rot)           # the gates' encoding
    tab_int = lut.lhe_table(digits, d_tree, d_rot, encode=lambda v: lut.encode(v, 4))
    outs = []
    for q in range(2):
        Cs = S.K.tgsw_encrypt(lut.lhe_address_bits(addr[q], 10), seed=4301 + q)
        with S.ck.tgsw_set(Cs, 10) as ts:
            outs.append((S.ck.lhe_lookup(ts, tab_bool, d_tree=d_tree, d_rot=d_rot)[:, 0], S.ck.lhe_lookup(ts, tab_int, d_tree=d_tree, d_rot=d_rot)[:, 0]))
    x, y = outs[0][0], outs[1][0]
    assert np.array_equal(S.K.decrypt(x), bits[addr[0]] == 1) and np.array_equal(S.K.decrypt(y), bits[addr[1]] == 1)
    nand = thfhe.gate_nand(S.ck, x, y)
    assert np.array_equal(S.K.decrypt(nand), ~((bits[addr[0]] == 1) & (bits[addr[1]] == 1)))
    g = lambda m: (3 * m + 1) % 4
    tv = lut.test_vector(lut.int_outputs(g, 4), 4)
    r = S.ck.lut_bootstrap(tv, outs[0][1])[:, 0]
    assert np.array_equal(lut.decode(S.K.phase(r), 4), g(digits[addr[0]]))


def test_sk128_sbox_16_bit_to_4_bit(sk128):
    from thfhe import circuits, lut
    S = sk128
    rng = np.random.default_rng(4500)
    table = rng.integers(0, 16, 1 << 16)
    addr = np.concatenate([[0, 65535, 1024, 1023], rng.integers(0, 1 << 16, 4)])
    with S.ck.tgsw_set(S.K.tgsw_encrypt(lut.lhe_address_bits(addr, 16), seed=4501), 16) as ts:
        out = circuits.lhe_sbox(S.ck, ts, table)
    assert out.shape == (8, 4, S.p.n + 1)
    got = lut.decode(S.K.phase(out).reshape(8, 4), 8)
    assert np.array_equal(got, (table[addr][:, None] >> np.arange(4)) & 1)


@pytest.mark.parametrize("name", ["SK-80", "SK-lib"])
def test_named_sets_at_full_size(O, name):
    s = Keys(O, name)
    try:
        s.check(8, 6, 10, 1, 4400 + s.p.n, "(6, 10, 1)")
    finally:
        s.ck.close()
