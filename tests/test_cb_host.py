"""Circuit bootstrapping, host side (no GPU): the argument checks of the C ABI that run before any device work, the digit
rule, the private key switch of the model (tests/cb_reference.py) on noiseless keys, its rows against SecretKeySet.tgsw_encrypt's on real keys, the
key generators, and the real-key cases of tests/test_gpu_cb.py on the CPU model: the model decodes every lookup and comparison before the device
is asked to (cb_cases.case asserts it), and its row noise lies inside the band the device test asserts."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import cb_cases as CC
import cb_reference as CB
import lhe_reference as LR
from support import N, words

SHAPES = [(1, 1), (7, 4), (8, 4), (10, 3), (4, 8)]


# ---- ABI ---------------------------------------------------------------------------------------------------------------------------------

def test_abi_symbols_refuse_bad_arguments_before_the_context_is_looked_at():
    import thfhe
    L = thfhe.lib()
    buf = np.zeros(64, np.int32)
    p, h = thfhe._p32(buf), C.c_void_p()
    for fn in ("thfhe_cb_key_set", "thfhe_cb_private_keyswitch", "thfhe_circuit_bootstrap", "thfhe_cb_set_batch_threshold", "thfhe_mk_ctx_info"):
        assert hasattr(L, fn)
    bad = thfhe.lib().thfhe_cb_key_set
    for D, t, basebit, what in ((64, 9, 4, "t basebit > 32"), (64, 33, 1, "t basebit > 32"), (0, 7, 4, "D = 0"), (2049, 7, 4, "D > 2048"), (64, 0, 4, "t = 0"),
                                (64, 3, 9, "a digit wider than a byte"), (64, 7, 0, "basebit = 0")):
        assert bad(None, p, D, t, basebit) != 0, what
        assert ("D must be" if "D" in what else "basebit") in L.thfhe_last_error().decode(), what
    assert bad(None, None, 64, 7, 4) != 0 and "null argument" in L.thfhe_last_error().decode()
    assert bad(None, p, 64, 7, 4) != 0 and "null ctx" in L.thfhe_last_error().decode()      # valid arguments reach the context check
    ks = L.thfhe_cb_private_keyswitch
    assert ks(None, None, 1, p) != 0 and "null argument" in L.thfhe_last_error().decode()
    assert ks(None, p, 1, None) != 0 and "null argument" in L.thfhe_last_error().decode()
    assert ks(None, p, 1, p) != 0 and "null ctx" in L.thfhe_last_error().decode()
    cb = L.thfhe_circuit_bootstrap
    assert cb(None, None, None, 1, 3, None, C.byref(h)) != 0 and "null argument" in L.thfhe_last_error().decode()
    assert cb(None, None, p, 1, 3, None, None) != 0 and "null argument" in L.thfhe_last_error().decode()
    for d in (0, -1, 17):
        assert cb(None, None, p, 1, d, None, C.byref(h)) != 0 and "d must be" in L.thfhe_last_error().decode()
    assert cb(None, None, p, 0, 3, None, C.byref(h)) != 0 and "count must be" in L.thfhe_last_error().decode()
    assert cb(None, None, p, 1, 3, None, C.byref(h)) != 0 and "null ctx" in L.thfhe_last_error().decode()
    assert not h.value
    assert L.thfhe_cb_set_batch_threshold(None, 8) != 0
    dev = C.c_int()
    assert L.thfhe_mk_ctx_info(None, C.byref(thfhe.Params()), C.byref(dev)) != 0


# ---- digit rule --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("t,basebit", SHAPES)
def test_digit_rule(t, basebit):
    B, bt = 1 << basebit, t * basebit
    rng = np.random.default_rng(100 * t + basebit)
    # every word whose rounding carries through all digits: the kept bits all ones and the rounding bit set (they round to zero)
    carry_all = [] if bt >= 32 else [(((1 << bt) - 1) << (32 - bt)) | (1 << (31 - bt)) | int(v) for v in rng.integers(0, 1 << (31 - bt), 64)] + \
        [(((1 << bt) - 1) << (32 - bt)) | (1 << (31 - bt)), 0xFFFFFFFF]
    # ... and the words whose balancing carries through all digits: every raw digit >= B/2
    half = sum((B // 2) << (32 - (p + 1) * basebit) for p in range(t))
    w = np.array([0, 0x7FFFFFFF, 0x80000000, half, (-half) & 0xFFFFFFFF] + carry_all + [int(v) for v in rng.integers(0, 1 << 32, 10000)], np.int64)
    d = CB.digits(w.astype(np.uint32).view(np.int32), t, basebit)
    assert d.shape == (w.shape[0], t) and d.min() >= -(B // 2) and d.max() < B // 2
    total = sum(d[:, p] << (32 - (p + 1) * basebit) for p in range(t))
    want = CB.rounded(w, t, basebit)
    assert np.array_equal(total & 0xFFFFFFFF, want & 0xFFFFFFFF)
    assert np.all(np.abs(CB.centred(want - w)) <= (1 << (31 - bt) if bt < 32 else 0))          # rounding to the nearest
    if carry_all:
        assert not d[5:5 + len(carry_all)].any()                                                # a whole turn: all digits zero
    assert np.all(d[4] == -(B // 2)) or basebit == 1                                            # the all-carry word: every digit -B/2
    # the kernel's closed form: ((w + offset) >> shift & (B - 1)) - B/2 with B/2 added at every digit position
    off = (0 if bt >= 32 else 1 << (31 - bt)) + sum(1 << (31 - p * basebit) for p in range(t))
    v = (w + off) & 0xFFFFFFFF
    closed = np.stack([((v >> (32 - (p + 1) * basebit)) & (B - 1)) - B // 2 for p in range(t)], axis=1)
    assert np.array_equal(closed, d)


def test_balanced_bytes():
    w = np.array([0, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF, 0x80808080, 0x7F7F7F7F, 0x12345678], np.int64)
    b = CB.balanced_bytes(w)
    assert b.min() >= -128 and b.max() <= 127
    assert np.array_equal(sum(b[:, p] << (8 * p) for p in range(4)) & 0xFFFFFFFF, w)
    assert b[1].tolist() == [-1, 0, 0, -128] and b[2].tolist() == [0, 0, 0, -128]


# ---- noiseless phases --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("t,basebit", [(7, 4), (8, 4), (10, 3)])
def test_noiseless_phases(t, basebit):
    import thfhe
    from thfhe import keygen
    D, l, Bgbit = 64, 3, 7
    rng = np.random.default_rng(7000 + t)
    K = keygen.SecretKeySet(thfhe.make_params("SK-128", n=4), seed=71)
    z2 = keygen.rand_ternary(rng, D)
    z2[:2] = (1, -1)
    key = keygen.gen_cb_key(rng, z2, K.rlwe_key, t, basebit, 0.0)
    assert key.shape == (2, D, t, 2, N) and key.dtype == np.int32
    bits = rng.integers(0, 2, 6)
    a = rng.integers(-2**31, 2**31, (6, l, D), dtype=np.int64)
    g = np.array([1 << (32 - (j + 1) * Bgbit) for j in range(l)], np.int64)
    b = (a * z2).sum(axis=2) + bits[:, None] * g[None, :]                         # noiseless LWE samples of m g_j under z2
    lwe2 = np.concatenate([a, b[:, :, None]], axis=2).astype(np.uint32).view(np.int32)
    rows = CB.private_keyswitch(key, lwe2, l, t, basebit)
    assert rows.shape == (6, 2 * l, 2, N)
    err = CB.row_errors(K, rows, bits, l, Bgbit)
    bound = int(np.abs(z2).sum()) * (1 << (31 - t * basebit) if t * basebit < 32 else 0)   # sum |z2_i| |a_i - round(a_i)|
    assert np.abs(err).max() <= bound, (int(np.abs(err).max()), bound)
    assert np.abs(err[:, l:, 1:]).max() == 0                                      # T_1: only coefficient 0 carries anything
    if bound:
        assert np.abs(err).max() > 0


# ---- real keys ---------------------------------------------------------------------------------------------------------------------------

def test_rows_are_tgsw_samples_up_to_noise(O):
    """the model's rows and SecretKeySet.tgsw_encrypt's rows of the same bits: same messages, noise inside 6.5 sigma of each; as the control bit of
    the model CMux (lhe_reference.cmux) both select the same operand"""
    from thfhe import lut
    S, c = CC.keys(O, "SK-128"), CC.case(O, "SK-128")
    l, Bgbit = S.tp.l, S.tp.Bgbit
    err = CB.row_errors(S.K, c["rows"], c["bits"], l, Bgbit)
    assert np.abs(err).max() <= 6.5 * S.sigma_row() * 2.0**32
    fresh = S.K.tgsw_encrypt(c["bits"], seed=0xCB30)
    assert fresh.shape == c["rows"].shape
    assert np.abs(CB.row_errors(S.K, fresh, c["bits"], l, Bgbit)).max() <= 6.5 * S.sig["bk"] * 2.0**32
    rng = np.random.default_rng(0xCB31)
    m1, m0 = 5, 2
    sigma_cmux = np.sqrt(2 * l * N * 4.0 ** Bgbit / 12) * S.sigma_row()
    for r in (0, 1, 2, 30):                                                        # bits of both values
        d1, d0 = (np.concatenate([words(rng, N), np.zeros(N, np.int32)]) for _ in range(2))
        for d, m in ((d1, m1), (d0, m0)):                                          # TLWE samples of constant polynomials under z
            d[N:] = (S.K.tlwe_phase(d[:N], np.zeros(N, np.int32)).astype(np.int64) * -1 + int(lut.encode(m, 8))).astype(np.uint32).view(np.int32)
        got, ref = LR.cmux(S.p, c["rows"][r], d1, d0), LR.cmux(S.p, fresh[r], d1, d0)
        want = lut.encode(m1 if c["bits"][r] else m0, 8)
        for out, tol in ((got, 6.5 * sigma_cmux), (ref, 6.5 * np.sqrt(2 * l * N * 4.0 ** Bgbit / 12) * S.sig["bk"])):
            e = CB.centred(S.K.tlwe_phase(out[:N], out[N:]).astype(np.int64) - int(want))
            assert np.abs(e).max() <= tol * 2.0**32 + 2.0 ** (32 - l * Bgbit), (r, float(np.abs(e).max()) / 2.0**32)
    assert {int(c["bits"][r]) for r in (0, 1, 2, 30)} == {0, 1}


@pytest.mark.parametrize("name", ["SK-128", "SK-80"])
def test_model_decodes_the_gpu_cases_and_its_row_noise_is_inside_the_band(O, name):
    S, c = CC.keys(O, name), CC.case(O, name)       # case() asserts that the model decodes every lookup and comparison
    assert c["rows"].shape == (len(c["bits"]), 2 * S.tp.l, 2, N)
    std, pred = CC.row_noise(S, c["rows"], c["bits"]), S.sigma_row()
    print(f"\ncb row noise {name} (CPU model): measured std {std:.3e} over {c['rows'].size // 2} coefficients, predicted {pred:.3e}, ratio {std / pred:.2f}")
    assert 0.5 * pred <= std <= 2 * pred


# ---- key generators ----------------------------------------------------------------------------------------------------------------------

def _mk_hash(K):
    h = hashlib.sha256()
    for a in (K.lwe_keys, K.rlwe_keys, K.bk, K.ksk):
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


@pytest.mark.parametrize("name,over,digest", [
    ("MK2", dict(n=12), "f42c3af89b3befced213a65103fc0ef1d4bf0adb1bcc7e55478f55db88dd8dd0"),
    ("MK4-N2048", dict(n=6, parties=1), "5252c33144cf0bbc9689b36b72ebf1e808ca6f11e68ae7af6f49a795ea53bcfd"),
    ("MK256", dict(n=5, parties=1), "0a64bab5169dd771ce8f4db987f0644aa1b1f48c2f8757d262ac959d99c8a5f6"),
])
def test_mk_key_set_without_lwe_keys_is_unchanged(name, over, digest):
    # sha256 of the key material recorded before the lwe_keys argument existed
    import thfhe
    from thfhe import keygen
    p = thfhe.make_params(name, **over)
    K = keygen.MKSecretKeySet(p, seed=0x5EED0C0B, sigma_bk=thfhe.SIGMAS[name]["bk"])
    assert _mk_hash(K) == digest
    # a given key replaces the drawn one and nothing else of the stream: the ring keys stay, the key-dependent tables change
    given = 1 - K.lwe_keys
    K2 = keygen.MKSecretKeySet(p, seed=0x5EED0C0B, sigma_bk=thfhe.SIGMAS[name]["bk"], lwe_keys=given)
    assert np.array_equal(K2.lwe_keys, given) and np.array_equal(K2.rlwe_keys, K.rlwe_keys)
    assert K2.bk.shape == K.bk.shape and not np.array_equal(K2.bk, K.bk)
    x = K2.encrypt([0, 1, 1, 0])
    assert np.array_equal(K2.decrypt(x), [False, True, True, False])


# ---- the boundaries of tests/test_gpu_cb_slices.py ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(CC.BOUNDARIES))
def test_batch_boundaries_are_what_the_sources_say(name):
    """the slice, launch, tile and threshold constants the GPU slice tests are sized by, read from the text of the sources: a changed constant fails
    here instead of moving those cases off their boundaries unnoticed"""
    import os
    import re
    value, fname, pattern = CC.BOUNDARIES[name]
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "torus-fhe_amd", "csrc", fname)) as f:
        found = re.findall(pattern, f.read())
    assert len(found) == 1, (name, fname, "the defining line was expected exactly once", found)
    assert int(found[0]) == value, (name, fname, int(found[0]), value)


def test_boundary_table_names_every_boundary_once():
    assert sorted(CC.BOUNDARIES) == ["bit slice", "input tile", "inputs per launch", "pair threshold", "stage-B host slice"]
    assert (CC.SLICE_BITS, CC.LAUNCH_INPUTS, CC.HOST_SLICE_INPUTS, CC.TILE_INPUTS, CC.PAIR_THRESHOLD) == (2048, 4096, 2048, 256, 256)


@pytest.mark.parametrize("name", ["SK-128", "SK-80"])
def test_pool_rows_are_pairwise_distinct(O, name):
    # a draw from the pool can only show a misplaced bit if no two records of the pool have the same rows
    rows = CC.case(O, name)["rows"]
    flat = rows.reshape(rows.shape[0], -1)
    assert len({r.tobytes() for r in flat}) == rows.shape[0] == (48 if name == "SK-128" else 24)


def test_drawn_batch_has_the_drawn_rows_as_its_model(O):
    S, c = CC.keys(O, "SK-128"), CC.case(O, "SK-128")
    recs, idx = CC.drawn(c, 100, 0xD7A3)
    assert recs.shape == (100, S.tp.n + 1) and idx.shape == (100,) and idx.min() >= 0 and idx.max() < 48
    assert np.array_equal(recs, c["recs"][idx])
    assert len(set(idx.tolist())) > 24 and not np.array_equal(idx, np.arange(100) % 48)       # a random draw, not a period of the pool
    again = CC.drawn(c, 100, 0xD7A3)
    assert np.array_equal(again[0], recs) and np.array_equal(again[1], idx)                      # a fixed seed
    assert not np.array_equal(CC.drawn(c, 100, 0xD7A4)[1], idx)
    assert CC.drawn(c, 100, 0xD7A3, pool=24)[1].max() < 24
    rows = CB.circuit_bootstrap(S.orc2, S.pks, recs, S.tp.l, S.tp.Bgbit, CC.T, CC.BASEBIT)
    assert np.array_equal(rows, c["rows"][idx])


def test_cb_param_sets_stay_out_of_the_named_sets():
    import thfhe
    assert not set(thfhe.CB_PARAM_SETS) & set(thfhe.PARAM_SETS)
    for name, sk in (("CB-128", "SK-128"), ("CB-80", "SK-80")):
        p = thfhe.make_params(**thfhe.CB_PARAM_SETS[name])
        assert (p.n, p.N, p.l, p.Bgbit, p.parties, p.torus_bits) == (thfhe.PARAM_SETS[sk]["n"], 2048, 2, 18, 1, 64)
        assert thfhe.CB_SIGMAS[name]["bk"] == 2.0**-62
