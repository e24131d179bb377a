"""The leveled-scatter kernels at the FP64 exactness bound (pytest -m gpu; DESIGN.md sections 3 and 4.17), in the discipline of
test_gpu_exactness_bound.py: crafted inputs of bound_inputs.py -- every TGSW word extreme_key_word (0x7FFF8000), and an operand whose digits are
all -Bg/2 in every row -- so the limb sums of the product reach 2l N 2^(Bgbit-1) 2^15 exactly (l rows: half of it), which random words stay more
than 5 bits below.  Each case asserts the sum it reached and every output word of 12 samples against the exact-NTT model.

  thfhe_lhe_demux          sk_lhe_demux_kernel<l, false> on x = (T, T) and <l, true> on the trivial x = (0, T), T = digit_word everywhere;
  thfhe_lhe_scatter (0, 1) one POSITIVE rotation step of sk_lhe_scatter_rotate_kernel<l> by N / 2 on the value (0 | -T) in both halves -- X^(N/2) v - v
                           is T at every coefficient -- encrypted (2l rows) and trivial (the l body rows); every sample into a table of its own."""
import numpy as np
import pytest

import bound_inputs as B
import lhe_reference as LR
import scatter_reference as SR

pytestmark = pytest.mark.gpu

LHE_SHAPES = [(1, 8), (2, 10), (3, 7), (3, 10), (4, 8)]
LHE_IDS = ["l1-Bg8", "SK-80", "SK-128", "l3-Bg10", "l4-Bg8-full"]
BATCH = 12      # identical samples: more than one workgroup per CU pair, every one compared


@pytest.fixture
def E(O, request):
    """(oracle parameters, CloudKey) of the shape at n = 4"""
    import thfhe
    l, Bgbit = request.param
    kw = dict(O.PARAM_SETS["SK-128"], n=4, l=l, Bgbit=Bgbit)
    p = O.make_params(**kw)
    K = O.SKKeys(p, 0xB0 + l, 2.0**-25, 2.0**-15)
    ck = thfhe.CloudKey(thfhe.make_params(**kw), K.bk, K.ksk, device=0)
    yield p, ck
    ck.close()


def _same_as(got, ref, what):
    for g in range(got.shape[0]):
        assert np.array_equal(got[g], ref), (what, g, np.argwhere(got[g] != ref)[:8].tolist())


@pytest.mark.parametrize("E", LHE_SHAPES, ids=LHE_IDS, indirect=True)
def test_demux_at_the_bound(E):
    p, ck = E
    N, l = p.N, p.l
    C, x, _ = B.lhe_cmux_case(p)
    with ck.tgsw_set(np.tile(C, (BATCH, 1, 1, 1)), 1) as ts:
        for kind, xs, rows in (("enc", x, 2 * l), ("pub", SR.trivial(x[N:]), l)):
            assert B.lhe_reached(p, C, xs) == B.bound(rows, N, p.Bgbit)
            ref0, ref1 = SR.demux(p, C, xs)
            t = np.tile(xs, (BATCH, 1))
            o0a, o0b, o1a, o1b = ck.lhe_demux(ts, 0, t[:, N:], x_a=t[:, :N] if kind == "enc" else None)
            _same_as(np.concatenate([o1a, o1b], axis=1), ref1, (kind, "child 1"))
            _same_as(np.concatenate([o0a, o0b], axis=1), ref0, (kind, "child 0"))


@pytest.mark.parametrize("E", LHE_SHAPES, ids=LHE_IDS, indirect=True)
def test_positive_rotation_step_at_the_bound(E):
    p, ck = E
    N, l = p.N, p.l
    C = np.full((1, 2 * l, 2, N), B.extreme_key_word(32), np.int32)
    T = B.digit_word(32, l, p.Bgbit)
    half = B._i32(np.concatenate([np.zeros(N // 2, np.int64), np.full(N // 2, -T, np.int64)]))     # X^(N/2) half - half = T everywhere
    with ck.tgsw_set(np.tile(C, (BATCH, 1, 1, 1, 1)), 1) as ts:
        for kind, v_a, rows in (("enc", half, 2 * l), ("pub", None, l)):
            diff = B.lhe_rot_diff(v_a, half, N // 2)
            assert np.all(diff[N:] == B._i32(T)) and B.lhe_reached(p, C[0], diff) == B.bound(rows, N, p.Bgbit)
            v = np.concatenate([np.zeros(N, np.int32) if v_a is None else v_a, half])
            ref = SR.scatter_wo_reduce(p, C, v, 0, 1)[0]
            tab_a, tab_b = ck.lhe_scatter(ts, half, val_a=v_a, d_tree=0, d_rot=1, n_tables=BATCH, table_index=np.arange(BATCH))
            assert tab_a.shape == (BATCH, 1, N)
            _same_as(np.concatenate([tab_a[:, 0], tab_b[:, 0]], axis=1), ref, kind)
            # ... and all twelve into one table: twelve times the leaf, mod 2^32
            one_a, one_b = ck.lhe_scatter(ts, half, val_a=v_a, d_tree=0, d_rot=1)
            assert np.array_equal(np.concatenate([one_a[0, 0], one_b[0, 0]]), B._i32(ref.astype(np.int64) * BATCH)), kind
