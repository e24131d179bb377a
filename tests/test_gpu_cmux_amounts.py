"""The opening of a CMux -- X^a acc - acc read from the LDS and cut into gadget digits (thfhe_lane.h: rotated_word, rotated_fields_keep,
rotated_digits_z) -- at EVERY rotation amount on the MI355X (pytest -m gpu), single key.  The index and sign of a rotated word depend on the amount,
the digits on the word, and that code runs on the device only (the host emulators take another branch of it), so the sweep goes through the public
calls: with n = 1 a job is exactly one CMux, and the encrypted-table bootstrap starts it from caller words in both polynomials
(tests/decomp_edges.py: every digit edge at every amount; its conditions are asserted on the CPU by test_decomp_edges_host.py).

  (a) every amount on the crafted accumulators and a random one, barb = 0;   (b) every amount behind a non-zero start rotation;
  (c) the other instantiations of the kernels -- the gate, the plaintext table (an all-zero mask polynomial: rows of -Bg/2 throughout) at theta = 1, 2
      and 4, the multi-value epilogue;   (d) two steps, the second on what the first wrote, on the structured amounts.

Every test runs the gadget depths l = 1 .. 4 on the eight-wave ring, the four-wave ring and the cooperative kernel, in calls of an odd job count that
stay on their shape; every output word against the CPU oracle, the first call of each shape twice with byte-equal outputs.  The CCS and KMS engines'
own CMux kernels are out of reach of this recipe -- no call sets their accumulator, so a job there runs many steps -- and remain covered by random
words only."""
import numpy as np
import pytest

import decomp_edges as D
import lut_reference as R
import mv_lut_reference as MV
import tree_lut_reference as TR
from support import KERNELS, pmap, thresholds, words
from test_gpu_mk_rotation_ends import odd_calls
from test_gpu_ring_exchange import MU, setup

pytestmark = pytest.mark.gpu

N = 1024
GADGETS = [(1, 8), (2, 10), (3, 7), (4, 8)]
gadgets = pytest.mark.parametrize("l, Bgbit", GADGETS, ids=["l%d" % g[0] for g in GADGETS])
SHAPES = [k for k in KERNELS if k[0] in ("ring8", "ring4", "coop")]
LIMIT = 1023          # jobs per call: odd, and within the four-wave ring's threshold
STARTS = (1, 63, 64, 1023, 1024, 1025, 2047)


@pytest.fixture(scope="module")
def ctx(O):
    """(n, l, Bgbit) -> (params, oracle, CloudKey): SK-128 at that length and gadget, random keys; built once, closed at the end"""
    made = {}

    def get(n, l, Bgbit):
        if (n, l, Bgbit) not in made:
            made[n, l, Bgbit] = setup(O, 0xCA00 + 64 * n + 16 * l + Bgbit, n=n, l=l, Bgbit=Bgbit)
        return made[n, l, Bgbit]
    yield get
    for v in made.values():
        v[2].close()


def records(O, amounts, barb, rng):
    """records (a_1 .. a_n, b) whose words mod-switch to the rows of `amounts` and to barb, each somewhere inside its rounding interval"""
    amounts = np.asarray(amounts, np.int64).reshape(len(amounts), -1)
    barb = np.broadcast_to(np.asarray(barb, np.int64), (len(amounts),))
    x = np.concatenate([D.amount_word(amounts, N, rng), D.amount_word(barb, N, rng)[:, None]], axis=1)
    for g in rng.integers(0, len(x), 64):
        assert [O.lib().oracle_modswitch(int(w), N) % (2 * N) for w in x[g]] == amounts[g].tolist() + [int(barb[g])]
    return x


def sweep(ck, l, amounts, launch, ref, expect):
    """launch(slice) on each shape, cut into odd calls that stay on it: every word equal to ref, the first call twice; the amounts the calls covered
    are `expect`"""
    ref = ref.reshape(ref.shape[0], -1, N + 1)
    for shape, coop, ring4, name in SHAPES:
        with thresholds(ck, coop, ring4):
            covered = set()
            for k, sl in enumerate(odd_calls(len(ref), LIMIT)):
                count = sl.stop - sl.start
                assert count % 2 == 1 and ck.rotation_kernel_name(count) == name.format(l=l)
                u = launch(sl)
                if k == 0:
                    again = launch(sl)
                    assert u.tobytes() == again.tobytes(), (shape, "two launches differ")
                u = u.reshape(count, -1, N + 1)
                assert u.shape == ref[sl].shape
                bad = np.argwhere(u != ref[sl])
                assert bad.size == 0, (shape, "amount, output, word of the first mismatches",
                                       [(amounts[sl.start + g].tolist(), int(j), int(q)) for g, j, q in bad[:6]])
                covered |= set(np.asarray(amounts[sl]).reshape(count, -1)[:, 0].tolist())
            assert covered == set(expect), shape


def tables_and_jobs(l, Bgbit, rng, amounts, random_table=True):
    """(tv_a, tv_b int32[tables][N], row of `amounts` and table of every job): every row on the edge table(s) its first amount takes
    (decomp_edges.tables_at) and on one uniform random table, the jobs permuted so that the waves of a workgroup hold unrelated amounts"""
    pairs = D.edge_tables(32, N, l, Bgbit) + ([tuple(words(rng, 2, N))] if random_table else [])
    tv_a, tv_b = np.stack([t[0] for t in pairs]), np.stack([t[1] for t in pairs])
    amounts = np.asarray(amounts)
    jobs = [(r, k) for r, a in enumerate(amounts.reshape(len(amounts), -1)[:, 0]) for k in D.tables_at(a, N) + (D.TABLES,) * random_table]
    jobs = np.array(jobs)[rng.permutation(len(jobs))]
    return tv_a, tv_b, amounts[jobs[:, 0]], jobs[:, 1].astype(np.int32)


def each(fn, items):
    """the reference models, one job after the other (they are numpy between two oracle calls: threads only contend for the interpreter)"""
    return np.stack([fn(g) for g in items])


@gadgets
def test_every_amount_on_crafted_accumulators(O, ctx, l, Bgbit):
    # (a): barb = 0, so the accumulator entering the one CMux is (tv_a, tv_b) word for word; a = 0 is the skipped CMux, beside working neighbours
    p, orc, ck = ctx(1, l, Bgbit)
    rng = np.random.default_rng([0xA, l, Bgbit])
    tv_a, tv_b, a, idx = tables_and_jobs(l, Bgbit, rng, np.arange(2 * N))
    xs = records(O, a, 0, rng)
    assert all(O.lib().oracle_modswitch(int(w), N) == 0 for w in xs[:, 1]) and len(tv_a) == D.TABLES + 1
    assert all({int(k) for k in idx[a == v]} == set(D.tables_at(v, N)) | {D.TABLES} for v in range(2 * N))    # the tables the host test counts on
    ref = each(lambda g: TR.lut_enc(orc, [xs[g]], (1,), 0, tv_a[idx[g]], tv_b[idx[g]], 1, keyswitch=False), range(len(xs)))
    sweep(ck, l, a, lambda sl: ck.lut_bootstrap_enc_wo_keyswitch(tv_a, tv_b, xs[sl], theta=1, lut_index=idx[sl]), ref, range(2 * N))


@gadgets
def test_every_amount_behind_a_start_rotation(O, ctx, l, Bgbit):
    # (b): the start X^(-barb) and the CMux X^a compose; barb walks through STARTS as a varies
    p, orc, ck = ctx(1, l, Bgbit)
    rng = np.random.default_rng([0xB, l, Bgbit])
    tv_a, tv_b = words(rng, 1, N), words(rng, 1, N)
    a = rng.permutation(2 * N)
    barb = np.array(STARTS)[a % len(STARTS)]
    assert {(int(u) % 64, int(v)) for u, v in zip(a, barb)} >= {(r, s) for r in range(64) for s in STARTS}   # every lane residue with every start
    xs = records(O, a, barb, rng)
    ref = each(lambda x: TR.lut_enc(orc, [x], (1,), 0, tv_a[0], tv_b[0], 1, keyswitch=False), xs)
    sweep(ck, l, a, lambda sl: ck.lut_bootstrap_enc_wo_keyswitch(tv_a, tv_b, xs[sl], theta=1), ref, range(2 * N))


@gadgets
def test_every_amount_through_the_gate(O, ctx, l, Bgbit):
    # (c) kGate: the accumulator is (0, X^(-barb) mu): any body word
    p, orc, ck = ctx(1, l, Bgbit)
    rng = np.random.default_rng([0xC0, l, Bgbit])
    a = rng.permutation(2 * N)
    xs = records(O, a, rng.integers(0, 2 * N, len(a)), rng)
    ref = np.stack(pmap(lambda x: orc.bootstrap_wo_keyswitch(x, MU), xs))
    sweep(ck, l, a, lambda sl: ck.bootstrap_wo_keyswitch(xs[sl], MU), ref, range(2 * N))


@pytest.mark.parametrize("theta", [1, 2, 4])
@gadgets
def test_every_amount_on_a_plaintext_table(O, ctx, l, Bgbit, theta):
    # (c) kLut on the edge BODY polynomials: the mask polynomial is all zero, its l rows are -Bg/2 at every coefficient, only the body row carries
    # digits.  theta > 1: the prologue rounds the mask amounts to multiples of theta -- every one of those
    p, orc, ck = ctx(1, l, Bgbit)
    rng = np.random.default_rng([0xC1, l, Bgbit, theta])
    _, tv, a, idx = tables_and_jobs(l, Bgbit, rng, np.arange(0, 2 * N, theta), random_table=False)
    xs = records(O, a, 0, rng)
    ref = each(lambda g: R.lut_bootstrap(orc, [xs[g]], (1,), 0, tv[idx[g]], theta, keyswitch=False), range(len(xs)))
    assert ref.shape == (len(xs), theta, N + 1)
    sweep(ck, l, a, lambda sl: ck.lut_bootstrap_wo_keyswitch(tv, xs[sl], theta=theta, lut_index=idx[sl]), ref, range(0, 2 * N, theta))


@gadgets
def test_every_amount_through_the_multi_value_epilogue(O, ctx, l, Bgbit):
    # (c) kLutMv, the factor shapes of test_gpu_ring_exchange.test_multi_value_instantiation_n3: two tables of q = 9 outputs, p = 16 taps
    p, orc, ck = ctx(1, l, Bgbit)
    rng = np.random.default_rng([0xC2, l, Bgbit])
    tv0, factors = words(rng, N), words(rng, 2, 9, 16)
    a = rng.permutation(2 * N)
    idx = (np.arange(len(a)) % 2).astype(np.int32)
    xs = records(O, a, rng.integers(0, 2 * N, len(a)), rng)
    ref = each(lambda g: MV.combine(MV.rotate(orc, R.prologue([xs[g]], (1,), 0), tv0), factors[idx[g]], N), range(len(xs)))
    sweep(ck, l, a, lambda sl: ck.mv_lut_bootstrap_wo_keyswitch(factors, xs[sl], tv0=tv0, table_index=idx[sl]), ref, range(2 * N))


@gadgets
def test_two_steps_on_the_structured_amounts(O, ctx, l, Bgbit):
    # (d) n = 2: the second CMux rotates the accumulator the first one wrote (the ring kernel's update, then a rotated re-read), by the amount that
    # undoes the first rotation and by the same amount again
    p, orc, ck = ctx(2, l, Bgbit)
    rng = np.random.default_rng([0xD, l, Bgbit])
    S = D.structured_amounts(N, rng)
    assert D.structured_members(N) <= set(S.tolist()) and {int(v) % 64 for v in S} == set(range(64)) and len(S) >= 150
    both = np.array([(v, (2 * N - v) % (2 * N)) for v in S] + [(v, v) for v in S])
    tv_a, tv_b, pairs, idx = tables_and_jobs(l, Bgbit, rng, both)
    xs = records(O, pairs, 0, rng)
    ref = each(lambda g: TR.lut_enc(orc, [xs[g]], (1,), 0, tv_a[idx[g]], tv_b[idx[g]], 1, keyswitch=False), range(len(xs)))
    sweep(ck, l, pairs, lambda sl: ck.lut_bootstrap_enc_wo_keyswitch(tv_a, tv_b, xs[sl], theta=1, lut_index=idx[sl]), ref, S.tolist())
