"""Plain tables, encrypted tables and the two-digit tree on SK-80 (l = 2, Bgbit = 10, n = 500) and SK-lib (n = 1024, 1 152-word key-switch
rows) at full size (pytest -m gpu).  tests/test_gpu_lut.py and tests/test_gpu_tree_lut.py run SK-128 only; the
tree's workspace sizes and strides follow p.n and the packing key's n.  Key material as conftest.sk128 builds it (oracle keygen,
O.SIGMAS[set]); the packing key maps the set's LWE key to its bootstrapping ring key, with the ring's noise.

Word equality against the model composed from the CPU oracle on every sample of every call (an SK-lib rotation is 1 024 oracle CMuxes, about
0.1 s: the whole model takes seconds per set); decrypt-exactness on all samples at message moduli for which the model alone, run on these
seeds on the CPU, decrypts every case."""
import numpy as np
import pytest

import lut_reference as R
import tree_lut_reference as TR
from support import N, pmap

pytestmark = pytest.mark.gpu

SETS = ["SK-80", "SK-lib"]


class NamedSet:
    def __init__(self, O, name):
        import thfhe
        from thfhe import keygen
        from thfhe import threshold as T
        self.name, self.sig = name, O.SIGMAS[name]
        self.p = O.make_params(name)
        self.K = O.SKKeys(self.p, 0x5EED0000 + self.p.n, self.sig["bk"], self.sig["ks"])
        self.orc = O.Oracle(self.p, self.K.bk, self.K.ksk)
        self.pk = keygen.gen_pack_key(np.random.default_rng(0x7EE0000 + self.p.n), self.K.lwe_key, self.K.rlwe_key[0], self.p.ks_t,
                                      self.p.ks_basebit, self.sig["bk"])
        self.ck = thfhe.CloudKey(thfhe.make_params(name), self.K.bk, self.K.ksk, device=0)
        self.pc = T.PolyContext(0)
        self.pc.set_pack_key(self.pk, self.p.ks_t, self.p.ks_basebit)

    def close(self):
        self.ck.close()
        self.pc.close()

    def enc_int(self, m, p_msg, seed):
        from thfhe import lut
        return R.encrypt_words(self.K, lut.encode(np.asarray(m), p_msg), self.sig["lwe"], seed)

    def dec_int(self, recs, p_msg):
        from thfhe import lut
        return lut.decode(self.K.phases(recs), p_msg)


@pytest.fixture(scope="module", params=SETS)
def S(O, request):
    s = NamedSet(O, request.param)
    yield s
    s.close()


# ---- the cases: inputs by seed, so that the CPU-only check of the model (the module docstring) can rebuild them ------------------------------

def plain_case(S):
    """16 samples at p = 4, three tables of theta = 2 functions each, random per-sample index"""
    from thfhe import lut
    rng = np.random.default_rng(210 + S.p.n)
    F = rng.integers(0, 4, (3, 2, 4))
    tvs = np.stack([lut.test_vector([lut.int_outputs(lambda m, f=f: f[m], 4) for f in Ft], 4, theta=2) for Ft in F])
    m = np.tile(np.arange(4), 4)
    idx = rng.integers(0, 3, 16).astype(np.int32)
    return tvs, S.enc_int(m, 4, 2100), idx, F[idx, :, m]


def enc_case(S):
    """16 samples at p = 2, three fresh encrypted tables of theta = 4 functions each, random per-sample index"""
    from thfhe import lut
    rng = np.random.default_rng(220 + S.p.n)
    F = rng.integers(0, 2, (3, 4, 2))
    tvs = np.stack([lut.test_vector([lut.int_outputs(lambda m, f=f: f[m], 2) for f in Ft], 2, theta=4) for Ft in F])
    tv_a, tv_b = lut.encrypt_table(S.K.rlwe_key[0], tvs, S.sig["bk"], rng)
    m = np.tile(np.arange(2), 8)
    idx = rng.integers(0, 3, 16).astype(np.int32)
    return tv_a, tv_b, S.enc_int(m, 2, 2200), idx, F[idx, :, m]


P_TREE = 4   # p_hi = p_lo = p_out of the tree case: the model decrypts all of its samples at this modulus on both sets


def tree_case(S):
    """13 samples, two tables, f_table(hi, lo) at p = 4 with theta1 = 2 (2 + 1 rotations per sample), per-sample table index"""
    from thfhe import lut
    rng = np.random.default_rng(230 + S.p.n)
    count = 13
    F = rng.integers(0, P_TREE, (2, P_TREE, P_TREE))
    tv1 = np.stack([lut.tree_test_vectors(lambda h, l, f=f: f[h, l], P_TREE, P_TREE, P_TREE, theta=2) for f in F])
    tab = rng.integers(0, 2, count).astype(np.int32)
    hi, lo = rng.integers(0, P_TREE, count), rng.integers(0, P_TREE, count)
    return tv1, tab, S.enc_int(hi, P_TREE, 2300), S.enc_int(lo, P_TREE, 2301), F[tab, hi, lo]


def tree_model(S, tv1, tab, xh, xl, picks):
    """tree_lut_reference.tree on the samples `picks`, the three stages batched: the rotations of both levels run per sample on threads, the
    packing model once for all picks (it turns the whole packing key into 16-bit limbs on every call)"""
    p, theta, R1 = S.p, 2, P_TREE // 2
    cands = pmap(lambda gr: R.lut_bootstrap(S.orc, [xl[gr[0]]], (1,), 0, tv1[tab[gr[0]]][gr[1]], theta), [(g, r) for g in picks for r in range(R1)])
    cands = np.concatenate(cands).reshape(len(picks) * P_TREE, p.n + 1)
    a, b = TR.pack_boxes(cands, S.pk, p.ks_t, p.ks_basebit, P_TREE)
    return np.stack(pmap(lambda i: TR.lut_enc(S.orc, [xh[picks[i]]], (1,), 0, a[i], b[i], 1)[0], range(len(picks))))


# ---- the tests -------------------------------------------------------------------------------------------------------------------------------

def test_plain_tables(S):
    tvs, x, idx, want = plain_case(S)
    u = S.ck.lut_bootstrap_wo_keyswitch(tvs, x, theta=2, lut_index=idx)
    got = S.ck.lut_bootstrap(tvs, x, theta=2, lut_index=idx)
    assert u.shape == (16, 2, N + 1) and got.shape == (16, 2, S.p.n + 1)
    wo = np.stack(pmap(lambda g: R.lut_bootstrap(S.orc, [x[g]], (1,), 0, tvs[idx[g]], 2, keyswitch=False), range(16)))
    assert np.array_equal(u, wo)
    assert np.array_equal(got, np.stack([np.stack([S.orc.keyswitch(r) for r in s]) for s in wo]))
    # decrypt-exact on all 16: the model alone, run on these seeds, decrypts all 16 x 2 outputs at p = 4 on both sets
    assert np.array_equal(S.dec_int(got.reshape(-1, S.p.n + 1), 4).reshape(16, 2), want)


def test_encrypted_tables(S):
    tv_a, tv_b, x, idx, want = enc_case(S)
    u = S.ck.lut_bootstrap_enc_wo_keyswitch(tv_a, tv_b, x, theta=4, lut_index=idx)
    got = S.ck.lut_bootstrap_enc(tv_a, tv_b, x, theta=4, lut_index=idx)
    assert u.shape == (16, 4, N + 1) and got.shape == (16, 4, S.p.n + 1)
    wo = np.stack(pmap(lambda g: TR.lut_enc(S.orc, [x[g]], (1,), 0, tv_a[idx[g]], tv_b[idx[g]], 4, keyswitch=False), range(16)))
    assert np.array_equal(u, wo)
    assert np.array_equal(got, np.stack([np.stack([S.orc.keyswitch(r) for r in s]) for s in wo]))
    # decrypt-exact on all 16: the model alone, run on these seeds, decrypts all 16 x 4 outputs at p = 2 on both sets
    assert np.array_equal(S.dec_int(got.reshape(-1, S.p.n + 1), 2).reshape(16, 4), want)


def test_tree_whole_and_in_slices(S):
    tv1, tab, xh, xl, want = tree_case(S)
    kw = dict(p_hi=P_TREE, theta=2, table_index=tab)
    whole = S.ck.tree_lut_bootstrap(S.pc, tv1, xl, xh, **kw)
    assert whole.shape == (13, S.p.n + 1)
    try:
        S.ck.set_tree_slice(3 * P_TREE)      # 13 samples in slices of 3: five slices, the last one holds one sample
        sliced = S.ck.tree_lut_bootstrap(S.pc, tv1, xl, xh, **kw)
    finally:
        S.ck.set_tree_slice(65536)
    assert np.array_equal(sliced, whole)
    assert np.array_equal(whole, tree_model(S, tv1, tab, xh, xl, list(range(13))))
    # decrypt-exact on all 13: the model alone, run on these seeds, decrypts all 13 at p = 4 on both sets
    assert np.array_equal(S.dec_int(whole, P_TREE), want)
