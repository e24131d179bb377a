"""Multi-value bootstrapping on the named parameter sets (pytest -m gpu): thfhe_mv_lut_bootstrap(_wo_keyswitch) word
for word against the model composed from the CPU oracle (mv_lut_reference.py) and decrypt-exact, on SK-128 and, at full size, on SK-80
(l = 2, Bgbit = 10, n = 500) and SK-lib (n = 1024).  Key material as conftest.sk128 builds it.

The rotation's noise reaches output j times the 2-norm |c|_2 of its factor, and one rotation's noise is 2.5e-3 on SK-128: the
cases stay inside the supported set of that section -- digit outputs (p_out = 4) with |c|_2 <= 4 on SK-128, bit outputs (p_out = 2) at
p = 8 and on SK-80 / SK-lib.  Every case is built from seeds, and the model alone was first run on the CPU on the same seeds.  With random
tables of values in [0, p) at p_out = p it decrypted all of p = 4 (|c|_2 up to 6.2, largest error 2.1e-2 of the half-step 6.3e-2) but
missed 16 of 64 outputs at p = q = 8 and 6 of 24 in the weighted case (|c|_2 up to 16.7, std 2.9e-2 against the half-step 3.1e-2), so those
tables were narrowed as below; the assertion is unchanged, and the model decrypts every output of every case kept.  The tests print the
measured std of phase - encode next to the prediction |c|_2 sigma_br (+) sigma_ks."""
import numpy as np
import pytest

import lut_reference as R
import mv_lut_reference as MV
from support import N, pmap

pytestmark = pytest.mark.gpu

SIGMA_BR = {"SK-128": 2.5e-3, "SK-80": 4.3e-3, "SK-lib": 3.2e-3}   # one rotation's noise, measured on the CPU model
SIGMA_KS = {"SK-128": 2.8e-3, "SK-80": 2.2e-3, "SK-lib": 2.8e-3}


class KeySet:
    def __init__(self, O, name, keys=None):
        self.name, self.sig = name, O.SIGMAS[name]
        self.p = O.make_params(name)
        self.K = keys or O.SKKeys(self.p, 0x5EED0000 + self.p.n, self.sig["bk"], self.sig["ks"])
        self.orc = O.Oracle(self.p, self.K.bk, self.K.ksk)
        self.ck = None

    def open(self):
        import thfhe
        self.ck = thfhe.CloudKey(thfhe.make_params(self.name), self.K.bk, self.K.ksk, device=0)
        return self

    def enc_int(self, m, p_msg, seed):
        from thfhe import lut
        return R.encrypt_words(self.K, lut.encode(np.asarray(m), p_msg), self.sig["lwe"], seed)

    def dec_int(self, recs, p_msg):
        from thfhe import lut
        return lut.decode(self.K.phases(recs), p_msg)


@pytest.fixture(scope="module")
def S128(O, sk128):
    s = KeySet(O, "SK-128", sk128[1]).open()
    yield s
    s.ck.close()


@pytest.fixture(scope="module", params=["SK-80", "SK-lib"])
def Snamed(O, request):
    s = KeySet(O, request.param).open()
    yield s
    s.ck.close()


def model(S, recs, weights, bias, tv0, factors, idx, picks):
    """(int32[picks][q][N+1], int32[picks][q][n+1]) of the samples `picks`"""
    wo = np.stack(pmap(lambda g: MV.mv_lut(S.orc, [r[g] for r in recs], weights, bias, tv0, factors[idx[g]], keyswitch=False), picks))
    ks = np.stack(pmap(S.orc.keyswitch, wo.reshape(-1, N + 1))).reshape(wo.shape[0], wo.shape[1], -1)
    return wo, ks


def report(S, got, want, p_out, factors, idx, what):
    """print the std of phase - encode over all outputs and the prediction from the factors' 2-norms"""
    from thfhe import lut
    err = (S.K.phases(got.reshape(-1, S.p.n + 1)).astype(np.int64) - lut.encode(want.reshape(-1), p_out).astype(np.int64) + 2**31) % 2**32 - 2**31
    norm = np.sqrt((np.asarray(factors, np.float64)[idx] ** 2).sum(axis=-1))                # [count][q]
    pred = np.sqrt(np.mean((norm * SIGMA_BR[S.name]) ** 2) + SIGMA_KS[S.name] ** 2)
    print(f"\n{S.name} {what}: std of phase - encode {np.std(err / 2.0**32):.3e} (largest {np.abs(err).max() / 2.0**32:.3e}, half-step {1 / (4 * p_out):.3e}); "
          f"predicted {pred:.3e} at |c|_2 up to {norm.max():.1f}")


# ---- the cases: inputs by seed, so that the CPU-only check of the model (the module docstring) can rebuild them ------------------------------

DIGIT_TABLES = np.array([[0, 1, 2, 3], [3, 2, 1, 0], [1, 1, 2, 2], [0, 1, 1, 0]])   # p = 4 -> p_out = 4 with |c|_2 = 3.5, 3.5, 3.2, 1.4


def message_case(S, p_msg):
    """every message of p_msg (twice at p = 4) and q = p_msg functions of it: the four digit tables above at p = 4 (p_out = 4), eight random
    bit-valued tables at p = 8 (p_out = 2, |c|_2 <= 3.4).  Returns (tv0, factors, records, table index, expected messages, p_out)."""
    from thfhe import lut
    rng = np.random.default_rng(300 + p_msg)
    F, p_out = (DIGIT_TABLES, 4) if p_msg == 4 else (rng.integers(0, 2, (8, 8)), 2)
    m = np.tile(np.arange(p_msg), 8 // p_msg)
    step = (1 << 32) // (2 * p_out)
    return lut.mv_base(step), lut.mv_factors(F, p_msg)[None], [S.enc_int(m, p_msg, 3000 + p_msg)], np.zeros(len(m), np.int32), F[:, m].T, p_out


def weighted_case(S):
    """three fresh bits at p = 8, x = 2a + b + c + 1 through weights (2, 1, 1) and the bias encode(1, 8): q = 3 bit-valued functions (p_out = 2) of
    the sum 1 .. 5, two tables with a per-sample index"""
    from thfhe import lut
    rng = np.random.default_rng(330)
    a, b, c = (np.arange(8) >> 2) & 1, (np.arange(8) >> 1) & 1, np.arange(8) & 1
    F = rng.integers(0, 2, (2, 3, 8))
    idx = rng.integers(0, 2, 8).astype(np.int32)
    recs = [S.enc_int(v, 8, 3300 + k) for k, v in enumerate((a, b, c))]
    m = 2 * a + b + c + 1
    return lut.mv_base(1 << 30), np.stack([lut.mv_factors(f, 8) for f in F]), recs, idx, F[idx, :, m], int(lut.encode([1], 8)[0])


def named_case(S):
    """8 samples at p = 4, two tables of q = 4 bit-valued functions each (p_out = 2, |c|_2 <= 2.6) with a per-sample index"""
    from thfhe import lut
    rng = np.random.default_rng(340 + S.p.n)
    F = rng.integers(0, 2, (2, 4, 4))
    idx = rng.integers(0, 2, 8).astype(np.int32)
    m = np.tile(np.arange(4), 2)
    return lut.mv_base(1 << 30), np.stack([lut.mv_factors(f, 4) for f in F]), [S.enc_int(m, 4, 3400)], idx, F[idx, :, m]


# ---- the tests -------------------------------------------------------------------------------------------------------------------------------

def check_all(S, tv0, w, recs, idx, want, p_out, what, weights=(1,), bias=0):
    count, q = want.shape
    kw = dict(tv0=tv0, weights=weights, bias=bias, table_index=idx)
    u = S.ck.mv_lut_bootstrap_wo_keyswitch(w, *recs, **kw)
    got = S.ck.mv_lut_bootstrap(w, *recs, **kw)
    assert u.shape == (count, q, N + 1) and got.shape == (count, q, S.p.n + 1)
    wo, ks = model(S, recs, weights, bias, tv0, w, idx, range(count))
    assert np.array_equal(u, wo)
    assert np.array_equal(got, ks)
    report(S, got, want, p_out, w, idx, what)
    assert np.array_equal(S.dec_int(got.reshape(-1, S.p.n + 1), p_out).reshape(count, q), want)


@pytest.mark.parametrize("p_msg", [4, 8])
def test_every_message(S128, p_msg):
    tv0, w, recs, idx, want, p_out = message_case(S128, p_msg)
    check_all(S128, tv0, w, recs, idx, want, p_out, f"p = q = {p_msg}, p_out = {p_out}")


def test_three_weighted_inputs_with_a_bias(S128):
    tv0, w, recs, idx, want, bias = weighted_case(S128)
    check_all(S128, tv0, w, recs, idx, want, 2, "p = 8, q = 3, p_out = 2, x = 2a + b + c + 1", weights=(2, 1, 1), bias=bias)


def test_inputs_built_from_gate_outputs(S128):
    # a p = 4 digit d + 2 g from a bootstrapped digit d in {0, 1} (a LUT output) and a NAND output g (+-1/8): x = d + g + 1/8, two weighted inputs
    # with a bias; both inputs carry a key switch's noise
    import thfhe
    from thfhe import lut
    S = S128
    rng = np.random.default_rng(350)
    a, b, d = rng.integers(0, 2, 8), rng.integers(0, 2, 8), np.arange(8) & 1
    xa, xb = S.K.encrypt_bits(a, S.sig["lwe"], 3500), S.K.encrypt_bits(b, S.sig["lwe"], 3501)
    g = thfhe.gate_nand(S.ck, xa, xb)
    xd = S.ck.lut_bootstrap(lut.test_vector(lut.int_outputs(lambda m: m & 1, 4), 4), S.enc_int(d, 4, 3502))[:, 0]
    m = d + 2 * (1 - (a & b))
    F = DIGIT_TABLES[[0, 2, 3]]
    tv0, w = lut.mv_base(1 << 29), lut.mv_factors(F, 4)
    kw = dict(tv0=tv0, weights=(1, 1), bias=1 << 29)
    got = S.ck.mv_lut_bootstrap(w, xd, g, **kw)
    picks = [0, 3, 6]
    wo, ks = model(S, [xd, g], (1, 1), 1 << 29, tv0, w[None], np.zeros(8, np.int32), picks)
    assert np.array_equal(S.ck.mv_lut_bootstrap_wo_keyswitch(w, xd, g, **kw)[picks], wo)
    assert np.array_equal(got[picks], ks)
    report(S, got, F[:, m].T, 4, w[None], np.zeros(8, np.int32), "p = 4, q = 3 on gate outputs")
    assert np.array_equal(S.dec_int(got.reshape(-1, S.p.n + 1), 4).reshape(8, 3), F[:, m].T)


def test_named_sets(Snamed):
    tv0, w, recs, idx, want = named_case(Snamed)
    check_all(Snamed, tv0, w, recs, idx, want, 2, "p = q = 4, p_out = 2, two tables")


def test_invalid_calls_are_refused_and_the_context_stays_usable(S128):
    import thfhe
    S = S128
    tv0, w, recs, idx, want, p_out = message_case(S, 4)
    with pytest.raises(thfhe.ThfheError, match="error -1.*out of range"):
        S.ck.mv_lut_bootstrap(w, *recs, tv0=tv0, table_index=np.ones(8, np.int32))
    with pytest.raises(thfhe.ThfheError, match="error -1.*p must be"):
        S.ck.mv_lut_bootstrap(np.zeros((1, 4, 3), np.int32), *recs, tv0=tv0)
    with pytest.raises(thfhe.ThfheError, match="error -1.*q must be"):
        S.ck.mv_lut_bootstrap(np.zeros((1, 65, 4), np.int32), *recs, tv0=tv0)
    got = S.ck.mv_lut_bootstrap(w, *recs, tv0=tv0)
    assert np.array_equal(S.dec_int(got.reshape(-1, S.p.n + 1), 4).reshape(8, 4), want)
