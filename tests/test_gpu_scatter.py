"""Leveled scatter under real keys (pytest -m gpu): SK-128, SK-80 and SK-lib at full size.  The address bits are TGSW samples
of SecretKeySet.tgsw_encrypt at the set's bootstrapping-key noise; every table word is compared with the model composed from the CPU oracle's exact
pieces (scatter_reference.py), and every slot must decrypt.  The model alone, run on the CPU on these seeds, decrypts every case (the figures are in
DESIGN 4.17), so nothing was narrowed.

Noise.  Every leaf of a sample carries the d products of its path, so a slot summed over S samples predicts sqrt(S d) sigma_1, sigma_1 = sqrt(2 l N
Bg^2 / 12) sigma_bk (SK-128: 8.6e-5).  The truncating decomposition's bias puts the measured figure above that and may add coherently
over S, so no band is asserted against the formula: the tests assert word equality with the model -- the std is then the model's by construction --
and that every slot decrypts, and print the std next to the figure recorded from the model: histogram of 16 samples at (2, 4), std over all 4 096
coefficients of the 4 polynomials 1.10e-3 (prediction 8.5e-4).  Failure rates are not measured."""
import math

import numpy as np
import pytest

import lhe_reference as LR
import scatter_reference as SR
from support import N, pmap

pytestmark = pytest.mark.gpu

HIST_S, HIST_CFG, P_OUT = 16, (2, 4), 8
HIST_STD_MODEL = 1.10e-3      # std of phase - encode over the table, measured on the CPU model on the seeds below


class Keys:
    def __init__(self, O, name, device=True):
        import thfhe
        from thfhe import keygen
        self.name, self.sig = name, thfhe.SIGMAS[name]
        self.tp = thfhe.make_params(name)
        self.K = keygen.SecretKeySet(self.tp, seed=0x5EED0100 + self.tp.n, sigma_lwe=self.sig["lwe"], sigma_bk=self.sig["bk"], sigma_ks=self.sig["ks"])
        self.p = O.make_params(name)
        self.ck = thfhe.CloudKey(self.tp, self.K.bk, self.K.ksk, device=0) if device else None

    def sigma_cmux(self):
        return math.sqrt(2 * self.p.l * N * 4.0 ** self.p.Bgbit / 12) * self.sig["bk"]

    def tgsw(self, addr, d, seed):
        from thfhe import lut
        return self.K.tgsw_encrypt(lut.lhe_address_bits(addr, d), seed=seed).reshape(len(addr), d, 2 * self.p.l, 2, N)

    def histogram_case(self, S, seed):
        """addresses, their TGSW samples, the model's table int32[1][2^d_tree][2N], the plain table"""
        from thfhe import circuits, lut
        d_tree, d_rot = HIST_CFG
        addr = np.random.default_rng(seed).integers(0, 1 << (d_tree + d_rot), S)
        Cs = self.tgsw(addr, d_tree + d_rot, seed + 1)
        one = lut.lhe_value([1], encode=lambda v: lut.encode(v, P_OUT))
        leaves = np.stack(pmap(lambda s: SR.scatter_wo_reduce(self.p, Cs[s], SR.trivial(one), d_tree, d_rot), range(S)))
        ref = leaves.astype(np.int64).sum(axis=0).astype(np.uint32).view(np.int32)[None]
        return addr, Cs, ref, circuits.lhe_scatter_plain(addr, one, d_tree, d_rot)

    def table_error(self, tab, plain):
        """phase - plain of a table int32[..., 2N] (mask | body) against its plain polynomials, as signed integers"""
        ph = self.K.tlwe_phase(tab[..., :N], tab[..., N:]).astype(np.int64)
        return (ph - plain + 2**31) % 2**32 - 2**31

    def check_histogram(self, S, seed):
        """one histogram: word for word against the model, every count decrypts; returns the std of phase - encode over the table (torus units)"""
        from thfhe import circuits, lut
        d_tree, d_rot = HIST_CFG
        addr, Cs, ref, plain = self.histogram_case(S, seed)
        counts = np.bincount(addr, minlength=1 << (d_tree + d_rot))
        assert counts.max() < P_OUT
        dec = lambda tab: lut.decode(lut.lhe_table_entries(self.K.tlwe_phase(tab[0, :, :N], tab[0, :, N:]), d_tree, d_rot)[0], P_OUT)
        assert np.array_equal(dec(ref), counts), "the model itself must decrypt every slot"
        with self.ck.tgsw_set(Cs, d_tree + d_rot) as ts:
            tab_a, tab_b = circuits.lhe_histogram(self.ck, ts, P_OUT, d_tree, d_rot)
        got = np.concatenate([tab_a, tab_b], axis=2)
        assert np.array_equal(got, ref), np.argwhere(got != ref)[:6].tolist()
        assert np.array_equal(dec(got), counts)
        std = float(self.table_error(got, plain).std()) / 2.0**32
        pred = math.sqrt(S * (d_tree + d_rot)) * self.sigma_cmux()
        print(f"\nscatter noise {self.name} histogram S = {S} at {HIST_CFG}: std {std:.3e} over {got.size // 2} coefficients (GPU == CPU model word for word), "
              f"sqrt({S} x {d_tree + d_rot}) x {self.sigma_cmux():.3e} = {pred:.3e}, ratio {std / pred:.2f}")
        return std


@pytest.fixture(scope="module")
def sk128(O):
    s = Keys(O, "SK-128")
    yield s
    s.ck.close()


def test_sk128_histogram_of_16_samples(sk128):
    std = sk128.check_histogram(HIST_S, 5100)
    print(f"recorded from the CPU model: {HIST_STD_MODEL:.3e}")
    assert 1 / 32 >= 6 * std      # the half-step of p_out = 8 against the measured noise: the rule DESIGN 4.17 derives the supported S from


def scatter_then_lookup_case(S):
    """4 writers of encrypted theta = 2 values at distinct addresses of (3, 5), 8 readers: (writer addresses, values, reader addresses, writer and
    reader TGSW samples, encrypted values (mask, body))"""
    from thfhe import lut
    rng = np.random.default_rng(5200)
    w_addr = np.array([5, 77, 200, 255])
    f = rng.integers(1, P_OUT, (4, 2))
    r_addr = np.concatenate([w_addr, [4, 109, 72, 0]])      # one bit off in the rotation part, in the tree part, in both, and far away
    vals = lut.lhe_value(f, encode=lambda v: lut.encode(v, P_OUT))
    enc = lut.encrypt_table(S.K.rlwe_key, vals, S.sig["bk"], rng)
    return w_addr, f, r_addr, S.tgsw(w_addr, 8, 5201), S.tgsw(r_addr, 8, 5202), enc


def scatter_then_lookup_model(S, case):
    from thfhe import lut
    w_addr, f, r_addr, Cw, Cr, (va, vb) = case
    tab = SR.scatter(S.p, Cw, np.concatenate([va, vb], axis=1), 3, 5)[0]
    u = np.stack(pmap(lambda s: LR.lookup_wo_keyswitch(S.p, Cr[s], tab[:, :N], tab[:, N:], 3, 5, 2), range(8)))
    want = np.zeros((8, 2), np.int64)
    for s, a in enumerate(r_addr):
        hit = np.flatnonzero(w_addr == a)
        if hit.size:
            want[s] = f[hit[0]]
    return tab, u, want


def test_sk128_scatter_then_lookup_on_the_returned_table(sk128):
    from thfhe import lut
    S = sk128
    case = scatter_then_lookup_case(S)
    w_addr, f, r_addr, Cw, Cr, (va, vb) = case
    tab, u_ref, want = scatter_then_lookup_model(S, case)
    assert (want[:4] == f).all() and not want[4:].any()
    dec = lambda u: lut.decode(S.K.ring_phase(u).reshape(8, 2), P_OUT)
    assert np.array_equal(dec(u_ref), want), "the model itself must decrypt every case"
    with S.ck.tgsw_set(Cw, 8) as tw, S.ck.tgsw_set(Cr, 8) as tr:
        tab_a, tab_b = S.ck.lhe_scatter(tw, vb, val_a=va, d_tree=3, d_rot=5)
        got = np.concatenate([tab_a[0], tab_b[0]], axis=1)
        assert np.array_equal(got, tab), np.argwhere(got != tab)[:6].tolist()
        u = S.ck.lhe_lookup_wo_keyswitch(tr, tab_b, tab_a=tab_a, d_tree=3, d_rot=5, theta=2)
    assert np.array_equal(u, u_ref), np.argwhere(u != u_ref)[:6].tolist()
    assert np.array_equal(dec(u), want)
    err = (S.K.ring_phase(u).reshape(8, 2).astype(np.int64) - lut.encode(want, P_OUT).astype(np.int64) + 2**31) % 2**32 - 2**31
    print(f"\nscatter + lookup noise SK-128 (3, 5): std {float(err.std()) / 2.0**32:.3e} over 16 outputs; one write and one read predict "
          f"sqrt(4 x 8 + 8) x {S.sigma_cmux():.3e} = {math.sqrt(40) * S.sigma_cmux():.3e}")


@pytest.mark.parametrize("name", ["SK-80", "SK-lib"])
def test_named_sets_at_full_size(O, name):
    s = Keys(O, name)
    try:
        s.check_histogram(4, 5300 + s.p.n)
    finally:
        s.ck.close()


def test_error_paths_that_need_a_live_context(sk128):
    import thfhe
    S = sk128
    Cs = LR.trivial_tgsw(S.p, LR.address_bits([1, 2, 3], 2))
    v = np.zeros((1, N), np.int32)
    other = thfhe.CloudKey(S.tp, S.K.bk, S.K.ksk, device=0)
    try:
        with S.ck.tgsw_set(Cs, 2) as ts:
            for kw in (dict(first=1, count=3), dict(first=4, count=0), dict(first=0, count=4)):
                with pytest.raises(thfhe.ThfheError, match="not all in the set"):
                    S.ck.lhe_scatter(ts, v, d_tree=1, d_rot=1, **kw)
            with pytest.raises(thfhe.ThfheError, match="must equal the set's d"):
                S.ck.lhe_scatter(ts, v, d_tree=1, d_rot=2)
            with pytest.raises(thfhe.ThfheError, match="another context"):
                other.lhe_scatter(ts, v, d_tree=1, d_rot=1)
            with pytest.raises(thfhe.ThfheError, match="another context"):
                other.lhe_demux(ts, 0, np.zeros((3, N), np.int32))
            with pytest.raises(thfhe.ThfheError, match="not all in the set"):
                S.ck.lhe_demux(ts, 0, np.zeros((4, N), np.int32))
            with pytest.raises(thfhe.ThfheError, match="bit must be"):
                S.ck.lhe_demux(ts, 2, np.zeros((3, N), np.int32))
            # count 0 passes the checks and returns zeroed tables
            tab_a, tab_b = S.ck.lhe_scatter(ts, v, d_tree=1, d_rot=1, first=3, count=0)
            assert tab_a.shape == (1, 2, N) and not tab_a.any() and not tab_b.any()
    finally:
        other.close()
