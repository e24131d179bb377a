"""One call of 66 636 jobs (blind rotations: one per gate, two per MUX gate) on the MI355X (pytest -m gpu): 32 rounds of 2 048 on the eight-wave
ring kernel plus 1 100 = 1 024 on the four-wave ring and 76 on the cooperative kernel.  So one call runs every single-key kernel shape, the gate
prologues launch more than 65 535 grid rows (grid.y = jobs), and the LUT prologues, which clamp grid.y to 65 535, take a second pass of their
stride loop.  Job 65 536 is the first past that line and the first of the remainder.  Every output word must equal the same engine on the same
records cut into calls of 4 096 gates (the size the rest of the suite compares with the oracle), and the rows around each boundary must equal
the CPU oracle word for word.  Inputs are random records: the oracle evaluates any record, and so does the engine.  The key switches
(thfhe_keyswitch.h) run sk_keyswitch_mfma_kernel on the single key and ks_staged_kernel on the multi key, in the one call and in the chunks."""
import numpy as np
import pytest

import lut_reference as R
import mk_lut_reference as MR

pytestmark = pytest.mark.gpu

JOBS = 32 * 2048 + 1100
CHUNK = 4096   # gates (samples) per call of the chunked run: a MUX chunk is 8 192 jobs
# first / last job of the first eight-wave round, the last two jobs under 2^16, the first past it (and of the four-wave ring), the last
# four-wave job, the first cooperative job, the last job
EDGE_JOBS = [0, 2047, 2048, 65534, 65535, 65536, 66559, 66560, JOBS - 1]
EDGE_MUX_GATES = sorted({j // 2 for j in EDGE_JOBS})   # the MUX gates holding those jobs: 32 767 and 32 768 among them


def records(rng, count, words):
    return rng.integers(-2**31, 2**31, (count, words), dtype=np.int32)


def chunked(call, *arrays):
    """call() on slices of CHUNK rows of every array, outputs concatenated"""
    count = arrays[0].shape[0]
    return np.concatenate([call(*(a[s:s + CHUNK] for a in arrays)) for s in range(0, count, CHUNK)])


def assert_rows_equal(got, want, what):
    assert got.shape == want.shape, what
    bad = np.flatnonzero((got != want).reshape(got.shape[0], -1).any(axis=1))
    assert bad.size == 0, f"{what}: {bad.size} of {got.shape[0]} rows differ, first at {bad[:8].tolist()}"


# ---- single key (SK-128) ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sk(sk128):
    import thfhe
    p, K, orc = sk128
    ck = thfhe.CloudKey(thfhe.make_params("SK-128"), K.bk, K.ksk, device=0)
    assert ck.rotation_kernel_name(JOBS) == "sk_blind_rotate_ring_kernel<3>"
    assert ck.rotation_kernel_name(JOBS % 2048) == "sk_blind_rotate_ring_kernel<3, 4 waves>"   # 1 100 = 1 024 four-wave + 76 cooperative
    yield p, orc, ck
    ck.close()


def test_sk_nand(O, sk):
    import thfhe
    p, orc, ck = sk
    rng = np.random.default_rng(1)
    x, y = records(rng, JOBS, p.n + 1), records(rng, JOBS, p.n + 1)
    got = ck.gates(thfhe.NAND, x, y)
    assert_rows_equal(got, chunked(lambda a, b: ck.gates(thfhe.NAND, a, b), x, y), "NAND vs chunked")
    assert_rows_equal(got[EDGE_JOBS], orc.gates(O.NAND, x[EDGE_JOBS], y[EDGE_JOBS]), "NAND vs oracle")


def test_sk_mux(O, sk):
    import thfhe
    p, orc, ck = sk
    rng = np.random.default_rng(2)
    x, y, z = (records(rng, JOBS // 2, p.n + 1) for _ in range(3))
    got = ck.gates(thfhe.MUX, x, y, z)
    assert_rows_equal(got, chunked(lambda a, b, c: ck.gates(thfhe.MUX, a, b, c), x, y, z), "MUX vs chunked")
    g = EDGE_MUX_GATES
    assert_rows_equal(got[g], orc.gates(O.MUX, x[g], y[g], z[g]), "MUX vs oracle")


def test_sk_gates_mixed(O, sk):
    import thfhe
    p, orc, ck = sk
    rng = np.random.default_rng(3)
    x, y = records(rng, JOBS, p.n + 1), records(rng, JOBS, p.n + 1)
    ops = rng.integers(thfhe.NAND, thfhe.ORYN + 1, JOBS).astype(np.int32)
    got = ck.gates_mixed(ops, x, y)
    assert_rows_equal(got, chunked(lambda o, a, b: ck.gates_mixed(o, a, b), ops, x, y), "gates_mixed vs chunked")
    ref = np.concatenate([orc.gates(int(ops[j]), x[j:j + 1], y[j:j + 1]) for j in EDGE_JOBS])
    assert_rows_equal(got[EDGE_JOBS], ref, "gates_mixed vs oracle")


def test_sk_bootstrap_wo_keyswitch(sk):
    p, orc, ck = sk
    rng = np.random.default_rng(4)
    x = records(rng, JOBS, p.n + 1)
    got = ck.bootstrap_wo_keyswitch(x)
    assert_rows_equal(got, chunked(ck.bootstrap_wo_keyswitch, x), "bootstrap_wo_keyswitch vs chunked")
    assert_rows_equal(got[EDGE_JOBS], np.stack([orc.bootstrap_wo_keyswitch(x[j]) for j in EDGE_JOBS]), "bootstrap_wo_keyswitch vs oracle")


def test_sk_lut_theta2(sk):
    # two inputs, non-trivial weights and bias, three tables picked per sample; key-switched outputs (int32[count][2][n+1])
    p, orc, ck = sk
    rng = np.random.default_rng(5)
    x, y = records(rng, JOBS, p.n + 1), records(rng, JOBS, p.n + 1)
    tvs = rng.integers(-2**31, 2**31, (3, p.N), dtype=np.int32)
    idx = rng.integers(0, 3, JOBS).astype(np.int32)
    weights, bias = (3, -7), int(rng.integers(-2**31, 2**31))

    def call(i, a, b):
        return ck.lut_bootstrap(tvs, a, b, weights=weights, bias=bias, theta=2, lut_index=i)
    got = call(idx, x, y)
    assert got.shape == (JOBS, 2, p.n + 1)
    assert_rows_equal(got, chunked(call, idx, x, y), "lut_bootstrap vs chunked")
    ref = np.stack([R.lut_bootstrap(orc, [x[j], y[j]], weights, bias, tvs[idx[j]], 2) for j in EDGE_JOBS])
    assert_rows_equal(got[EDGE_JOBS], ref, "lut_bootstrap vs composed oracle")


# ---- 3-gen multi-key (MK2) ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mk2(O):
    import thfhe
    p = O.make_params("MK2")
    s = O.SIGMAS["MK2"]
    K = O.MKKeys(p, 0x5EED0003, s["bk"], s["ks"])
    ck = thfhe.MKCloudKey(thfhe.make_params("MK2"), K.bk, K.ksk, device=0)
    yield p, O.MKOracle(p, K.bk, K.ksk), ck
    ck.close()


def test_mk2_nand(O, mk2):
    import thfhe
    p, orc, ck = mk2
    rng = np.random.default_rng(11)
    x, y = records(rng, JOBS, ck.words), records(rng, JOBS, ck.words)
    got = ck.gates(thfhe.NAND, x, y)
    assert_rows_equal(got, chunked(lambda a, b: ck.gates(thfhe.NAND, a, b), x, y), "MK2 NAND vs chunked")
    assert_rows_equal(got[EDGE_JOBS], orc.gates(O.NAND, x[EDGE_JOBS], y[EDGE_JOBS]), "MK2 NAND vs oracle")


def test_mk2_mux(O, mk2):
    import thfhe
    p, orc, ck = mk2
    rng = np.random.default_rng(12)
    x, y, z = (records(rng, JOBS // 2, ck.words) for _ in range(3))
    got = ck.gates(thfhe.MUX, x, y, z)
    assert_rows_equal(got, chunked(lambda a, b, c: ck.gates(thfhe.MUX, a, b, c), x, y, z), "MK2 MUX vs chunked")
    g = EDGE_MUX_GATES
    assert_rows_equal(got[g], orc.gates(O.MUX, x[g], y[g], z[g]), "MK2 MUX vs oracle")


def test_mk2_lut_theta1(mk2):
    p, orc, ck = mk2
    rng = np.random.default_rng(13)
    x, y = records(rng, JOBS, ck.words), records(rng, JOBS, ck.words)
    tvs = rng.integers(-2**63, 2**63, (3, p.N), dtype=np.int64)
    idx = rng.integers(0, 3, JOBS).astype(np.int32)
    weights, bias = (-2, 5), int(rng.integers(-2**31, 2**31))

    def call(i, a, b):
        return ck.lut_bootstrap(tvs, a, b, weights=weights, bias=bias, theta=1, lut_index=i)
    got = call(idx, x, y)
    assert got.shape == (JOBS, 1, ck.words)
    assert_rows_equal(got, chunked(call, idx, x, y), "MK2 lut_bootstrap vs chunked")
    ref = np.stack([MR.lut_bootstrap(orc, [x[j], y[j]], weights, bias, tvs[idx[j]], 1) for j in EDGE_JOBS])
    assert_rows_equal(got[EDGE_JOBS], ref, "MK2 lut_bootstrap vs composed oracle")


# ---- CCS (CCS2) ----------------------------------------------------------------------------------------------------------------------
def test_ccs2_nand(O):
    import thfhe
    p = O.make_params("CCS2")
    s = O.SIGMAS["CCS2"]
    K = O.CCSKeys(p, 0x5EED0001, s["bk"], s["ks"])
    ck = thfhe.CCSCloudKey(thfhe.make_params(**p.as_dict()), K.bk, K.pk, K.crs, K.ksk, device=0)
    try:
        rng = np.random.default_rng(21)
        x, y = records(rng, JOBS, ck.words), records(rng, JOBS, ck.words)
        got = ck.gates(thfhe.NAND, x, y)
        assert_rows_equal(got, chunked(lambda a, b: ck.gates(thfhe.NAND, a, b), x, y), "CCS2 NAND vs chunked")
        assert_rows_equal(got[EDGE_JOBS], O.CCSOracle(p, K).gates(O.NAND, x[EDGE_JOBS], y[EDGE_JOBS]), "CCS2 NAND vs oracle")
    finally:
        ck.close()
