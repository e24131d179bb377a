"""CPU checks behind the key-switch module's GPU tests (tests/test_gpu_ks_*.py): ks_reference, the NumPy restatement of the key switch,
equals the C oracle word for word in every layout, crafted rows included; and the case table of ks_cases covers the code: the constants of
the restated launch rule are the ones in the sources' text, and every compiled kernel instance is the predicted route of some (case, count)."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import ks_cases as KC
import ks_reference as R

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "torus-fhe_amd", "csrc")


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _case(engine, n, t, bb, N=1024, parties=1):
    return KC._c("host", "host", engine, n, t, bb, {}, N=N, parties=parties)


def _data(c, count, seed):
    K = KC.make_key(c, seed)
    return K, KC.make_inputs(c, count, seed)


# ---- the reference against the oracle --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,t,bb", [(37, 5, 3), (12, 15, 2), (130, 8, 2), (9, 31, 1), (5, 1, 1), (6, 6, 5), (3, 3, 8), (127, 2, 4)])
def test_single_key_equals_oracle(O, n, t, bb):
    c = _case("sk", n, t, bb)
    K, u = _data(c, 12, 1)
    p = O.make_params(n=n, N=1024, k=1, l=1, Bgbit=8, ks_t=t, ks_basebit=bb, torus_bits=32, parties=1)
    orc = O.Oracle(p, np.zeros(O.bk_shape(p), np.int32), K[0])
    ref = R.keyswitch(u, K, t, bb)
    assert ref.shape == (12, n + 1)
    assert np.array_equal(ref, np.stack([orc.keyswitch(r) for r in u]))
    # the MUX combine: two records per gate, (0, 2^29) + u1 + u2
    both = (u.view(np.uint32)[0::2] + u.view(np.uint32)[1::2]).view(np.int32).copy()
    both[:, -1] = (both[:, -1].view(np.uint32) + np.uint32(1 << 29)).view(np.int32)
    assert np.array_equal(R.keyswitch(u, K, t, bb, rot_per_gate=2), np.stack([orc.keyswitch(r) for r in both]))
    assert np.array_equal(R.keyswitch(u, K, t, bb, rows=[3, 11]), ref[[3, 11]])


@pytest.mark.parametrize("name,n,parties,t,bb", [("MK3", 11, 3, 3, 3), ("MK3", 130, 2, 5, 2), ("MK16", 7, 4, 2, 4)])
def test_3gen_equals_oracle(O, name, n, parties, t, bb):
    p = O.make_params(name, n=n, parties=parties, ks_t=t, ks_basebit=bb)
    c = _case("mk", n, t, bb, N=p.N, parties=parties)
    K, u = _data(c, 10, 2)
    orc = O.MKOracle(p, np.zeros(O.mk_bk_shape(p), np.int64), K)
    assert np.array_equal(R.keyswitch(u, K, t, bb), np.stack([orc.keyswitch(r) for r in u]))


def test_kms_equals_oracle(O):
    n, parties, t, bb = 7, 3, 8, 2
    p = O.KmsParams(n=n, N=2048, parties=parties, l_gsw=1, bg_gsw=8, l_lev=1, bg_lev=8, l_uni=1, bg_uni=8, ks_t=t, ks_basebit=bb)
    c = _case("kms", n, t, bb, N=2048, parties=parties)
    K, u = _data(c, 9, 3)
    z = lambda *s: np.zeros(s, np.int64)
    orc = O.KMSOracle(p, z(parties, n, 2, 2, 2048), z(parties, 3, 1, 2048), z(parties, 1, 2048), z(1, 2048), K)
    assert u.shape[1] == parties * 2048 + 1
    assert np.array_equal(R.keyswitch(u, K, t, bb, u_pstride=2048), np.stack([orc.keyswitch(r) for r in u]))


def test_ccs_equals_oracle(O):
    n, parties, t, bb = 6, 2, 5, 3
    p = O.make_params("CCS2", n=n, ks_t=t, ks_basebit=bb)
    c = _case("kms", n, t, bb, N=1024, parties=parties)   # the CCS layout is the KMS one at N = 1024
    K, u = _data(c, 9, 4)
    keys = SimpleNamespace(bk=np.zeros(O.ccs_bk_shape(p), np.int32), pk=np.zeros((parties, p.l, p.N), np.int32), crs=np.zeros((p.l, p.N), np.int32), ksk=K)
    orc = O.CCSOracle(p, keys)
    assert np.array_equal(R.keyswitch(u, K, t, bb, u_pstride=1024), np.stack([orc.keyswitch(r) for r in u]))


@pytest.mark.parametrize("n,t,bb", [(5, 5, 3), (9, 8, 2), (3, 16, 2)])
def test_packing_layout_equals_pack_reference(n, t, bb):
    import pack_reference as PR
    c = _case("pack", n, t, bb)
    K, x = _data(c, 9, 5)
    assert K.shape == (n, t, (1 << bb) - 1, 2, 1024)
    assert np.array_equal(R.pack_keyswitch(x, K, t, bb), PR.per_sample(x, K, t, bb))


def test_crafted_records_do_what_they_claim():
    for t, bb in ((8, 2), (5, 3), (31, 1), (2, 4)):
        c = _case("sk", 4, t, bb)
        u = KC.make_inputs(c, 8, 0).view(np.uint32)
        assert not R.digits(u[4, :-1], t, bb).any()                      # -offset: the carry runs through every digit and wraps
        assert (R.digits(u[5, :-1], t, bb) == (1 << bb) - 1).all()       # -offset - 1: every digit maximal
        d = R.digits(u[6, :-1], t, bb)
        assert not d[0::2].any() and (d[1::2] == (1 << bb) - 1).all()
        K = KC.make_key(c).view(np.uint32)
        for q, w in enumerate(KC.KEY_WORDS):
            assert (K[:, 5 + 2 * q:7 + 2 * q] == w).all() and (K[:, 1024 - 12 + 2 * q:1024 - 10 + 2 * q] == w).all()


# ---- the table covers the code ---------------------------------------------------------------------------------------------------------------
def test_restated_constants_are_the_sources():
    h = _src("thfhe_keyswitch.h")
    assert int(re.search(r"kKsMfmaMinSamples = (\d+);", h).group(1)) == KC.KS_MFMA_MIN
    assert int(re.search(r"kKsStagedMinSamples = (\d+);", h).group(1)) == KC.KS_STAGED_MIN
    assert int(re.search(r"kPackMfmaMinSamples = (\d+);", _src("thfhe_threshold.hip")).group(1)) == KC.PACK_MFMA_MIN
    widths = [(int(w), int(x4), int(x2)) for w, x4, x2 in re.findall(r"THFHE_KS_CASE\((\d+), (\d+), (\d+)\)", h)]
    assert sorted(64 * w for w, _, _ in widths) == sorted(KC.PLAIN_WIDTHS) and len(widths) == 12
    assert all(w == 4 * x4 + 2 * x2 for w, x4, x2 in widths)             # ROW = 64 (4 NX4 + 2 NX2) is the case's row
    staged = {tuple(map(int, m)) for m in re.findall(r"hipLaunchKernelGGL\(\(ks_staged_kernel<(\d+), (\d+), (\d+)>\)", h)}
    assert staged == set(KC.STAGED.values()) and len(staged) == 7
    for (row, bb), (W, rows, SJ) in KC.STAGED.items():
        assert row == 64 * W and rows == (1 << bb) - 1
    mfma = {tuple(map(int, m)) for m in re.findall(r"hipLaunchKernelGGL\(\(sk_keyswitch_mfma_kernel<(\d+), (\d+)>\)", h)}
    assert mfma == KC.MFMA_INSTANCES
    assert "samples < %d) ? 64 : 128" % KC.SPAN128_MIN in h and "a.t * a.basebit <= %d" % KC.STAGED_MAX_BITS in h
    assert "while (k.nsplit < 8 && (long)k.gtiles * k.wtiles * k.nsplit < 1024) k.nsplit *= 2;" in h   # mfma_nsplit
    assert "sA[%d]" % KC.MAX_SLICE in h and "a.N / nsplit_plain > %d" % KC.MAX_SLICE in h
    # the engines' nsplit rules, as text
    assert "gates <= 32 ? 16 : (gates <= 128 ? 8 : (gates <= 512 ? 2 : 1))" in _src("thfhe_sk.hip")
    assert "s <= 64 ? 16 : (s <= 256 ? 4 : (c->p.N > 2048 ? 2 : 1))" in _src("thfhe_mk.hip")
    assert "count <= 64 ? 8 : 2" in _src("thfhe_kms.hip")
    assert "n_pad / 64, stream, kPackMfmaMinSamples" in _src("thfhe_threshold.hip")


def _routes():
    return {(c.id, count): KC.case_route(c, count) for c in KC.CASES for count in c.counts}


def test_every_kernel_instance_is_some_cases_route():
    routes = set(_routes().values())
    plain = {r[1] for r in routes if r[0] == "plain"}
    staged = {r[1:4] for r in routes if r[0] == "staged"}
    spans = {r[4] for r in routes if r[0] == "staged"}
    mfma = {r[1:] for r in routes if r[0] == "mfma"}
    assert plain == set(KC.PLAIN_WIDTHS), sorted(set(KC.PLAIN_WIDTHS) - plain)
    assert staged == set(KC.STAGED.values()), sorted(set(KC.STAGED.values()) - staged)
    assert spans == {64, 128}
    assert mfma == KC.MFMA_INSTANCES, sorted(KC.MFMA_INSTANCES - mfma)
    # the single key's span-128 branch, which no named set reaches (a 2-bit staged shape without planes from 2 048 samples on)
    assert any(r[0] == "staged" and r[4] == 128 and KC.BY_ID[i].engine == "sk" for (i, _), r in _routes().items())
    # every nsplit tier of every engine, and both full slices of sA: N = 2048 with nsplit = 1, N = 4096 with nsplit = 2
    tiers = {(KC.BY_ID[i].engine, r[2]) for (i, _), r in _routes().items() if r[0] == "plain"}
    assert tiers >= {("sk", 16), ("sk", 8), ("sk", 2), ("sk", 1), ("mk", 16), ("mk", 4), ("mk", 2), ("mk", 1), ("kms", 8), ("kms", 2), ("pack", 2), ("pack", 4)}
    # the matrix-core kernel's chunk ranges (1 stores, the others accumulate), and a grid that the XCD renumbering leaves alone
    grids = {(k, (-(-count // 256) * (KC.row_words(KC.BY_ID[i].n) // 32) * k) % 8 == 0) for (i, count), r in _routes().items()
             if r[0] == "mfma" and KC.BY_ID[i].engine == "sk" for k in [KC.mfma_nsplit(KC.row_words(KC.BY_ID[i].n), count)]}
    assert {k for k, _ in grids} == {1, 2, 4, 8} and (1, False) in grids and (1, True) in grids
    slices = {(KC.BY_ID[i].N, r[2]) for (i, _), r in _routes().items() if r[0] == "plain" and KC.BY_ID[i].engine == "mk"}
    assert (2048, 1) in slices and (4096, 2) in slices
    print("covered: %d plain widths, %d staged instances, spans %s, %d matrix-core instances" % (len(plain), len(staged), sorted(spans), len(mfma)))


def test_cases_keep_their_claims():
    for (cid, count), rt in _routes().items():
        c = KC.BY_ID[cid]
        assert rt[0] == c.counts[count], (cid, count, rt)                # the count sits on the side of its threshold the case claims
        if rt[0] == "plain":
            N = 128 * ((c.n + 127) // 128) if c.engine == "pack" else c.N
            assert N % rt[2] == 0 and N // rt[2] <= KC.MAX_SLICE, (cid, count, rt)
        rows = KC.check_rows(c, count, rt)
        assert set(KC.crafted_positions(count)) <= set(rows) and len(rows) >= min(count, KC.N_CRAFTED + 4), (cid, count)
        assert c.n > 128 or len(rows) == count
    for c in KC.CASES:
        assert KC.key_bytes(c) <= KC.KEY_CAP, (c.id, KC.key_bytes(c))
        assert c.t * c.basebit <= 31 and c.n <= (1407 if c.engine in ("sk", "mux") else 2048 if c.engine == "pack" else 767), c.id
    # the thresholds' two sides are both present
    sk = [count for c in KC.CASES if c.engine == "sk" for count in c.counts]
    for edge in (32, 128, 512, KC.KS_STAGED_MIN - 1, KC.KS_MFMA_MIN - 1, KC.SPAN128_MIN - 1):
        assert edge in sk and edge + 1 in sk, edge
