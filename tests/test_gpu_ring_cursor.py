"""The ring kernel's key-stream cursor on the MI355X (pytest -m gpu).  The cursor is wave-uniform: a 64-bit stream position
and a count of the chunks still ahead, both in scalar registers, advanced once per issue; a lane adds one constant byte offset; issues past the end
of the stream repeat its last chunk.  What such a cursor can get wrong is aimed at here: a stream shorter than the prologue and the first rows'
issues (n = 1, 2, 3) and one just past them (n = 5), every gadget depth (the stream is 8 l n chunks long), workgroups whose last waves have no
job and waves whose mask word is 0 (both still issue and must advance like their neighbours), the second slice of the four-wave shape, and the
lookup-table instantiations.  Every output word against the exact oracle, every launch twice on the same inputs with byte-equal outputs.

SK-128 with a short mask keeps an oracle rotation at milliseconds (the recipe of test_gpu_ring_handoff.py)."""
import numpy as np
import pytest

import lut_reference as R
import mv_lut_reference as MV
from support import KERNELS, differing, pmap, thresholds, words

pytestmark = pytest.mark.gpu

RING = {k[0]: k for k in KERNELS if k[0] in ("ring8", "ring4")}
JOBS = {"ring8": (1, 7, 8, 9, 17), "ring4": (1, 3, 4, 5)}   # partly filled, full, and a last workgroup holding one job, per shape
MU = 1 << 29


def setup(O, seed, **over):
    """(params, oracle, CloudKey) of SK-128 with the given fields replaced, random keys"""
    import thfhe
    kw = dict(O.PARAM_SETS["SK-128"], **over)
    p = O.make_params(**kw)
    K = O.SKKeys(p, seed, 2.0**-25, 2.0**-15)
    return p, O.Oracle(p, K.bk, K.ksk), thfhe.CloudKey(thfhe.make_params(**kw), K.bk, K.ksk, device=0)


def twice(ck, shape, l, jobs, launch, ref):
    """launch() on the forced shape, twice: byte-identical outputs, every word equal to ref"""
    _, coop, ring4, name = RING[shape]
    with thresholds(ck, coop, ring4):
        assert ck.rotation_kernel_name(jobs) == name.format(l=l)
        first, second = launch(), launch()
        assert first.tobytes() == second.tobytes(), (shape, jobs, "two launches differ at", differing(first, second))
        assert np.array_equal(first, ref), (shape, jobs, differing(first, ref))


# n = 1, 2, 3: the three prologue issues and the first rows' issues already run past the end of an 8 l n-chunk stream; n = 5: they do not
@pytest.mark.parametrize("n", [1, 2, 3, 5])
@pytest.mark.parametrize("l, Bgbit", [(1, 8), (2, 10), (3, 7), (4, 8)], ids=["l1", "l2", "l3", "l4"])
def test_stream_end_job_counts_and_depth(O, l, Bgbit, n):
    p, orc, ck = setup(O, 0x5A00 + 16 * l + n, n=n, l=l, Bgbit=Bgbit)
    try:
        xs = words(np.random.default_rng(0x5B00 + 16 * l + n), 17, p.n + 1)
        ref = np.stack(pmap(lambda x: orc.bootstrap_wo_keyswitch(x, MU), xs))
        for shape, counts in JOBS.items():
            for jobs in counts:
                twice(ck, shape, l, jobs, lambda: ck.bootstrap_wo_keyswitch(xs[:jobs], MU), ref[:jobs])
    finally:
        ck.close()


def test_idle_waves_keep_the_cursor_moving(O):
    # n = 5, 9 jobs: the second eight-wave workgroup has seven waves without a job, the third four-wave one three.  Job j skips CMux j mod 5
    # while its neighbours work there, job 2 also CMux 3 and 4 (the end of the stream), job 6 every CMux.
    p, orc, ck = setup(O, 0x5C0, n=5)
    try:
        xs = words(np.random.default_rng(0x5C1), 9, p.n + 1)
        zero = {j: {j % p.n} for j in range(9)}
        zero[2] |= {3, 4}
        zero[6] = set(range(p.n))
        for j in range(9):
            for i in range(p.n):
                bar = O.lib().oracle_modswitch(int(xs[j, i]), p.N) % (2 * p.N)
                if i in zero[j]:
                    xs[j, i] = 0
                elif bar == 0:
                    xs[j, i] = 1 << 21        # mod-switches to 1
                assert (O.lib().oracle_modswitch(int(xs[j, i]), p.N) % (2 * p.N) == 0) == (i in zero[j])
        ref = np.stack(pmap(lambda x: orc.bootstrap_wo_keyswitch(x, MU), xs))
        for shape in RING:
            twice(ck, shape, p.l, 9, lambda: ck.bootstrap_wo_keyswitch(xs, MU), ref)
    finally:
        ck.close()


@pytest.fixture(scope="module")
def lut_env(O):
    p, orc, ck = setup(O, 0x5E0, n=3)
    yield p, orc, ck, words(np.random.default_rng(0x5E1), 9, p.n + 1)
    ck.close()


def test_lut_instantiation_theta4_n3(lut_env):
    p, orc, ck, xs = lut_env
    tv = words(np.random.default_rng(0x5E2), p.N)
    ref = np.stack(pmap(lambda x: R.lut_bootstrap(orc, [x], (1,), 0, tv, 4, keyswitch=False), xs))
    for shape in RING:
        twice(ck, shape, p.l, len(xs), lambda: ck.lut_bootstrap_wo_keyswitch(tv, xs, theta=4), ref)


def test_multi_value_instantiation_n3(lut_env):
    p, orc, ck, xs = lut_env
    rng = np.random.default_rng(0x5E4)
    tv0 = words(rng, p.N)
    factors = words(rng, 2, 9, 16)            # two tables of q = 9 outputs, p = 16 taps
    idx = (np.arange(len(xs)) % 2).astype(np.int32)
    accs = pmap(lambda x: MV.rotate(orc, R.prologue([x], (1,), 0), tv0), xs)
    ref = np.stack([MV.combine(acc, factors[t], p.N) for acc, t in zip(accs, idx)])
    for shape in RING:
        twice(ck, shape, p.l, len(xs), lambda: ck.mv_lut_bootstrap_wo_keyswitch(factors, xs, tv0=tv0, table_index=idx), ref)
