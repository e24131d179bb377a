"""The conditions tests/test_gpu_mk_rotation_ends.py relies on, checked once on the CPU (no GPU): the edge words of
tests/conv_edges.py tell the Torus64 -> Torus32 conversion from an exact-integer truncation in every binade where uniform random words never do;
the numpy model of the conversion is the oracle's and the host build's of thfhe_lane.h; the vectorised start and extraction are
mk_lut_reference's; the body words of amount_words() reach every rotation amount of every ring degree."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import conv_edges as E
import mk_lut_reference as R
import mk_mv_lut_reference as MV

HERE = os.path.dirname(os.path.abspath(__file__))
i32p, i64p = C.POINTER(C.c_int32), C.POINTER(C.c_int64)


@pytest.fixture(scope="module")
def lane():
    subprocess.run(["make", "-s", "-C", os.path.join(HERE, "emu")], check=True)
    return C.CDLL(os.path.join(HERE, "emu", "liblane_emu.so"))


@pytest.fixture(scope="module")
def mv_emu(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("conv_edges") / "libmk_mv_emu.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, os.path.join(HERE, "emu", "mk_mv_emu.cpp")], check=True)
    L = C.CDLL(so)
    L.mk_mv_emu_extract.argtypes = [C.c_int, i64p, i32p, C.c_int, C.c_int, C.c_int64, i32p]
    L.mk_mv_emu_extract.restype = C.c_int
    return L


def test_the_list_bites_in_every_binade_with_both_signs():
    w = E.edge_words()
    assert len(set(w.tolist())) == len(w)
    differ = E.t64tot32(w) != E.trunc_shift(w)
    b = E.binade(w)
    for e in E.BINADES:
        assert np.any(differ & (b == e) & (w > 0)) and np.any(differ & (b == e) & (w < 0)), e
    print("edge words: %d, the two conversions differ on %d" % (len(w), differ.sum()))
    # the saturating end: Float64(d) = 2^63 gives the quotient 2^31, which wraps
    assert np.all(np.isin(E.SATURATING, w))
    assert E.t64tot32(E.SATURATING).tolist() == [-2**31, -2**31] and E.trunc_shift(E.SATURATING).tolist() == [2**31 - 1, 2**31 - 1]
    assert E.t64tot32(E.to_i64([-2**63, -2**63 + 512, -2**63 + 513, 2**63 - 513])).tolist() == [-2**31, -2**31, -2**31 + 1, 2**31 - 1]
    bw = E.biting_words()
    assert len(bw) == differ.sum() and set(bw.tolist()) == set(w[differ].tolist())
    assert set(zip(E.binade(bw[:20]).tolist(), (bw[:20] < 0).tolist())) == {(e, s) for e in E.BINADES for s in (False, True)}


def test_random_words_do_not_bite():
    # The reason this file and its list exist: on uniform random 64-bit words -- what every other GPU test feeds the extraction kernels -- the
    # exact-integer truncation and the Float64 conversion agree on every word (they differ on about one word in 10^7), so a t64tot32 rewritten
    # with shifts, or a device lowering that double-rounds, would pass all of them.
    r = np.random.default_rng(20260101).integers(-2**63, 2**63, 10**6, dtype=np.int64)
    assert np.count_nonzero(E.t64tot32(r) != E.trunc_shift(r)) == 0


def test_model_is_the_oracles_conversion(O):
    w = E.edge_words()
    assert np.array_equal(E.t64tot32(w), [O.lib().oracle_t64tot32(int(v)) for v in w])
    assert MV.t64tot32 is E.t64tot32   # one copy of the model


@pytest.mark.parametrize("N,fn", [(1024, "emu_mk_extract"), (2048, "emu_mk_extract_2k")])
def test_model_is_the_host_build_of_the_lane_code(lane, N, fn):
    # extract16_64 and its N = 2048 twin, compiled for the host from thfhe_lane.h, on accumulators whose every word is an edge word; three cyclic
    # offsets so that every edge word stands at a negated mask position, and at mask word 0 and the body word some of them
    w = E.edge_words()
    for off in (0, 307, 611):
        acc = np.stack([E.tiled(w, N, off), E.tiled(w, N, off + 450)])
        out = np.zeros(N + 1, np.int32)
        getattr(lane, fn)(acc.ctypes.data_as(i64p), out.ctypes.data_as(i32p))
        ref = E.extract_at64(acc, 0, N)
        assert np.array_equal(out, ref), (N, off, np.flatnonzero(out != ref)[:6].tolist())
        wrong = E.trunc_shift(np.concatenate([acc[0, :1], E.neg64(acc[0, :0:-1]), acc[1, :1]]))
        assert np.count_nonzero(wrong != ref) > 100


@pytest.mark.parametrize("N", [1024, 2048, 4096])
@pytest.mark.parametrize("out_bias", [0, int(E.edge_words()[5])])
def test_model_is_the_host_build_of_the_mv_epilogue(mv_emu, N, out_bias):
    rng = np.random.default_rng(N)
    bw = E.biting_words()

    def run(acc, taps):
        out = np.zeros((len(taps), N + 1), np.int32)
        assert mv_emu.mk_mv_emu_extract(N, acc.ctypes.data_as(i64p), taps.ctypes.data_as(i32p), 2, len(taps), out_bias, out.ctypes.data_as(i32p)) == 1
        return out

    def check(acc, taps):
        out = run(acc, taps)
        ref = MV.combine64(acc.reshape(-1), taps, 2, N, out_bias)
        assert np.array_equal(out, ref), np.argwhere(out != ref)[:6].tolist()
        wrong = MV.combine64(acc.reshape(-1), taps, 2, N, out_bias, convert=E.trunc_shift)
        sums = MV.combine64(acc.reshape(-1), taps, 2, N, out_bias, convert=lambda s: s)
        assert set(E.binade(sums[wrong != ref]).tolist()) >= set(E.BINADES)   # the comparison above could have failed in every binade
        return sums

    # one tap, +-1: the sums are the accumulator's own (edge) words
    acc = np.stack([E.tiled(bw, N, 3), E.tiled(bw, N, 101)])
    check(acc, E.MV_TAPS_ONE)
    # two taps: the Torus64 sum of two words N/2 apart is an edge word, neither summand is (nor does either tell the two conversions apart)
    # (out_bias meets the body word only: the body's targets are the edge words less the bias)
    mask_tgt, body_tgt = E.tiled(bw, N // 2, 7), E.tiled(bw, N // 2, 59)
    acc = np.stack([E.two_tap_base(mask_tgt, rng, N), E.two_tap_base(E.to_i64(v - out_bias for v in body_tgt.tolist()), rng, N)])
    assert not np.isin(acc, E.edge_words()).any() and np.array_equal(E.t64tot32(acc), E.trunc_shift(acc))
    sums = check(acc, E.MV_TAPS_TWO)
    assert np.isin(mask_tgt, sums[:, :N]).all() and body_tgt[N // 4] in sums[:, N]   # the taps meet body words N/4 and 3N/4


def test_vectorised_references_are_the_oracles(O):
    rng = np.random.default_rng(8)
    for N in (1024, 2048, 4096):
        tv = rng.integers(-2**63, 2**63, (2, N), dtype=np.int64)
        tv[0, :5] = [-2**63, 2**63 - 512, 0, -1, 2**63 - 1]
        bars = [0, 1, N - 1, N, N + 1, 2 * N - 1, -1, -N, int(rng.integers(-N, N))]
        got = E.start64(tv[0], bars, N)
        for g, bar in enumerate(bars):
            assert np.array_equal(got[g], R.monomial64(tv[0], -bar, N)), (N, bar)
        both = np.stack([E.start64(tv[0], bars, N), E.start64(tv[1], bars, N)], axis=1)   # [jobs][2][N]
        for j in (0, 1, 3, N - 1):
            ex = E.extract_at64(both, j, N)
            assert ex.shape == (len(bars), N + 1)
            for g in (0, 2, 3, 5, 8):
                assert np.array_equal(ex[g], R.extract_at(both[g].reshape(-1), j, N)), (N, bars[g], j)


@pytest.mark.parametrize("N", [1024, 2048, 4096])
@pytest.mark.parametrize("theta", [1, 2, 4])
def test_amounts_are_complete(O, N, theta):
    w = E.amount_words(N, theta, np.random.default_rng(N + theta))
    assert w.dtype == np.int32 and len(w) == 2 * N // theta + 28
    bar = np.array(R.bars(w, N, theta))
    assert set((bar % (2 * N)).tolist()) == set(range(0, 2 * N, theta))
    # the ends sit where the rounding changes: c + step/2 - 1 stays with c, c + step/2 goes to the next amount; the same below c
    ends = np.array(R.bars(E.interval_ends(N, theta), N, theta)).reshape(4, 7) % (2 * N)
    for row, c in zip(ends, (0, N, theta, 2 * N - theta)):
        assert row.tolist() == [c, c, c, (c - theta) % (2 * N), c, c, (c + theta) % (2 * N)], (N, theta, c)
