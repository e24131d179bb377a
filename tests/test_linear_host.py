"""Encrypted dense layers on the CPU (no GPU): the numpy reference against Python's big integers on the edge values, every
refusal of the entries with no device present, the ctypes signatures, the plaintext helpers of thfhe.circuits, and the slice planner
(torus-fhe_amd/csrc/thfhe_linear_plan.h) as a stand-alone program under AddressSanitizer + UBSan (tests/cpp/linear_plan_test.cpp).
GPU twins: tests/test_gpu_linear.py, tests/test_gpu_mk_linear.py."""
import ctypes as C
import itertools
import json
import os
import subprocess

import numpy as np
import pytest

import linear_reference as LR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NAMES = ["lwe_linear", "linear_lut_bootstrap", "linear_lut_bootstrap_wo_keyswitch", "set_linear_slice"]


def test_reference_against_big_integers_on_the_edge_values():
    # every (weight, word) pair of the edge sets as a K = 1 product, then sums of K = 5 of them in every rotation, with and without an edge bias
    W1 = np.array(LR.EDGE_WEIGHTS, np.int64).reshape(-1, 1).astype(np.int32)
    x1 = np.array(LR.EDGE_WORDS, np.int64).reshape(1, 1, -1).astype(np.int32)
    assert np.array_equal(LR.linear(W1, x1), LR.linear_bigint(W1, x1))
    ew, ed = LR.EDGE_WEIGHTS, LR.EDGE_WORDS
    W = np.array([ew[r:] + ew[:r] for r in range(5)] + [[2**31 - 1] * 5, [-2**31] * 5], np.int64).astype(np.int32)   # [7][5]
    cols = list(itertools.product(ed, repeat=2))                                                                       # 16 (first, second) pairs
    x = np.array([[[cols[i][k % 2] if k < 2 else ed[(i + k) % 4] for i in range(16)] for k in range(5)]], np.int64).astype(np.int32)   # [1][5][16]
    for bias in (None, np.array([0, -1, 2**31 - 1, -2**31, 1, 5, -7], np.int64).astype(np.int32)):
        got, want = LR.linear(W, x, bias), LR.linear_bigint(W, x, bias)
        assert got.dtype == np.int32 and np.array_equal(got, want)
    rng = np.random.default_rng(5)
    W = rng.integers(-2**31, 2**31, (4, 9)).astype(np.int32)
    x = rng.integers(-2**31, 2**31, (2, 9, 6)).astype(np.int32)
    b = rng.integers(-2**31, 2**31, 4).astype(np.int32)
    assert np.array_equal(LR.linear(W, x, b), LR.linear_bigint(W, x, b))
    # the bias lands on the body word only
    assert np.array_equal(LR.linear(W, np.zeros_like(x), b)[:, :, :-1], np.zeros((2, 4, 5), np.int32))
    assert np.array_equal(LR.linear(W, np.zeros_like(x), b)[0, :, -1], b)


def test_new_symbols_are_in_signatures():
    import thfhe
    for prefix in ("thfhe_", "thfhe_mk_"):
        for n in NAMES + ["linear_last_timings"]:
            assert prefix + n in thfhe.SIGNATURES, prefix + n
    assert "thfhe_linear_tile" in thfhe.SIGNATURES
    tm, tk = thfhe.CloudKey.linear_tile()
    assert tm >= 1 and tk >= 1
    assert thfhe.MKCloudKey.linear_tile() == (tm, tk)


def test_every_refusal_without_a_device():
    import thfhe
    L = thfhe.lib()
    z = np.zeros(64, np.int32)
    t64 = np.zeros(64, np.int64)
    p = z.ctypes.data_as(C.POINTER(C.c_int32))
    fake = C.c_void_p(8)   # never dereferenced: every check below comes before the context is looked at

    def refused(rc, text):
        assert rc == -1 and text in L.thfhe_last_error(), (rc, L.thfhe_last_error())

    for mk in (False, True):
        pre = "thfhe_mk_" if mk else "thfhe_"
        lin, fus, fwo = (getattr(L, pre + n) for n in NAMES[:3])
        tv = t64.ctypes.data_as(C.POINTER(C.c_int64)) if mk else p
        # thfhe_lwe_linear(ctx, W, bias, M, K, in, out, count)
        for W, i, o in ((None, p, p), (p, None, p), (p, p, None)):
            refused(lin(fake, W, None, 1, 1, i, o, 1), b"null argument")
        for M, K in ((0, 1), (1, 0), (-1, 1), (65537, 1), (1, 65537)):
            refused(lin(fake, p, None, M, K, p, p, 1), b"M and K must be 1 .. 65536")
        refused(lin(None, p, None, 1, 1, p, p, 1), b"null ctx")
        assert lin(fake, p, None, 1, 1, p, p, 0) == 0 and lin(fake, p, p, 65536, 65536, p, p, 0) == 0   # count 0 is OK, the limits themselves too
        # thfhe_linear_lut_bootstrap(ctx, W, bias, M, K, theta, tv, n_luts, lut_index, in, out, count), and _wo_keyswitch
        for f in (fus, fwo):
            for W, t, i, o in ((None, tv, p, p), (p, None, p, p), (p, tv, None, p), (p, tv, p, None)):
                refused(f(fake, W, None, 1, 1, 1, t, 1, None, i, o, 1), b"null argument")
            for M, K in ((0, 1), (1, 0), (65537, 1), (1, 65537)):
                refused(f(fake, p, None, M, K, 1, tv, 1, None, p, p, 1), b"M and K must be 1 .. 65536")
            for theta in (0, 3, 5, 8, -1):
                refused(f(fake, p, None, 1, 1, theta, tv, 1, None, p, p, 1), b"theta must be 1, 2 or 4")
            for n_luts in (0, -1, 1025):
                refused(f(fake, p, None, 1, 1, 1, tv, n_luts, None, p, p, 1), b"n_luts must be 1 .. 1024")
            for bad in (-1, 3):
                idx = np.array([0, 2, bad], np.int32)
                refused(f(fake, p, None, 3, 1, 1, tv, 3, idx.ctypes.data_as(C.POINTER(C.c_int32)), p, p, 1), b"lut_index out of range")
            refused(f(None, p, None, 1, 1, 1, tv, 1, None, p, p, 1), b"null ctx")
            for theta in (1, 2, 4):
                assert f(fake, p, p, 3, 2, theta, tv, 1024, p, p, p, 0) == 0
        slc = getattr(L, pre + NAMES[3])
        refused(slc(None, 16), b"slice must be")
        refused(slc(fake, 0), b"slice must be")
        refused(slc(fake, (1 << 20) + 1), b"slice must be")
        tim = getattr(L, pre + "linear_last_timings")
        refused(tim(None, (C.c_float * 3)()), b"null argument")
        refused(tim(fake, None), b"null argument")
    refused(L.thfhe_linear_tile(None, None), b"null argument")


def test_python_wrappers_refuse_mismatched_shapes():
    import thfhe
    ck = thfhe.CloudKey.__new__(thfhe.CloudKey)   # no context: the shape checks come before the library is called
    ck.words = 5
    W = np.ones((2, 3), np.int32)
    with pytest.raises(ValueError):
        ck.lwe_linear(W, np.zeros((1, 4, 5), np.int32))          # K differs
    with pytest.raises(ValueError):
        ck.lwe_linear(W, np.zeros((1, 3, 6), np.int32))          # record width differs
    with pytest.raises(ValueError):
        ck.lwe_linear(W, np.zeros((1, 3, 5), np.int32), [1])     # one bias per output
    with pytest.raises(ValueError):
        ck.lwe_linear(np.ones(3, np.int32), np.zeros((1, 3, 5), np.int32))


def direct_conv(img, k, stride):
    kh, kw = k.shape
    oh, ow = (img.shape[0] - kh) // stride + 1, (img.shape[1] - kw) // stride + 1
    return np.array([[int((img[y * stride:y * stride + kh, x * stride:x * stride + kw] * k).sum()) for x in range(ow)] for y in range(oh)])


def test_conv2d_weights_against_a_direct_convolution():
    from thfhe import circuits
    rng = np.random.default_rng(9)
    for (H, Wd), (kh, kw), stride in (((5, 5), (3, 3), 1), ((6, 7), (2, 3), 1), ((7, 6), (3, 2), 2), ((4, 4), (4, 4), 1), ((5, 8), (1, 1), 3)):
        img = rng.integers(-5, 6, (H, Wd))
        k = rng.integers(-3, 4, (kh, kw))
        Wm = circuits.conv2d_weights(k, (H, Wd), stride)
        want = direct_conv(img, k, stride)
        assert Wm.dtype == np.int32 and Wm.shape == (want.size, H * Wd)
        assert np.array_equal(Wm.astype(np.int64) @ img.reshape(-1), want.reshape(-1))
    ks = rng.integers(-3, 4, (2, 2, 2))   # two filters: their rows one after the other
    img = rng.integers(-5, 6, (4, 5))
    Wm = circuits.conv2d_weights(ks, (4, 5))
    want = np.concatenate([direct_conv(img, ks[f], 1).reshape(-1) for f in range(2)])
    assert np.array_equal(Wm.astype(np.int64) @ img.reshape(-1), want)
    with pytest.raises(ValueError):
        circuits.conv2d_weights(np.ones((3, 3)), (2, 5))


def test_dense_bias_keeps_every_reachable_sum_in_range():
    from thfhe import circuits, lut
    # every input vector of a small layer, enumerated: with the bias the sums are messages in [lo, p), and the smallest one is lo exactly
    p = 16
    W = np.array([[1, -1, 2], [-1, -1, -1], [0, 3, 0], [2, 1, -2]])
    for lo, m_max in ((0, 3), (1, 2), (0, 1), (3, 2)):
        off = circuits.dense_bias_messages(W, p, lo, m_max)
        bias = circuits.dense_bias(W, p, lo, m_max)
        assert bias.dtype == np.int32 and np.array_equal(lut.decode(bias, p), off % (2 * p))
        msgs = np.array(list(itertools.product(range(m_max + 1), repeat=3)))
        sums = circuits.dense_plain(W, off, msgs, p)
        assert sums.min() >= lo and sums.max() < p
        assert np.array_equal(sums.min(axis=0), np.full(4, lo))
        # the torus side: W applied to the encoded messages plus the bias words decodes to the same sums
        enc = lut.encode(msgs, p).astype(np.int64)
        words = LR.to_i32(enc @ W.T + bias.astype(np.int64))
        assert np.array_equal(lut.decode(words, p), sums)
    assert np.array_equal(circuits.dense_plain(W, None, [1, 2, 3], p), (W @ np.array([1, 2, 3])) % (2 * p))
    with pytest.raises(ValueError):
        circuits.dense_bias(W, 8, 0, 3)          # row 0 spans 3 * 4 + 1 = 13 messages
    with pytest.raises(ValueError):
        circuits.dense_bias(np.ones((1, 9), int), 8, 0, 1)   # sums 0 .. 9


def test_slice_planner_under_asan(tmp_path):
    exe = str(tmp_path / "linear_plan_test")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                    "-o", exe, os.path.join(ROOT, "tests", "cpp", "linear_plan_test.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["errors"] == 0 and res["plans"] == 11 * 8 * 3 * 11 * 2
