"""thfhe_dag_last_group_ms: the device time of a run's last SELECT / TREE / MV / TREE_MV / leveled group from events of the
group's own.  A gate level that follows the group must not disturb it, profiling must not change a word, and the entry refuses to answer when no
profiled group was recorded."""
import ctypes as C

import numpy as np
import pytest

from support import SHAPES, shape_env, words


def test_null_arguments_are_refused_without_a_device():
    import thfhe
    L = thfhe.lib()
    ms = C.c_float()
    assert L.thfhe_dag_last_group_ms(None, C.byref(ms)) == -1 and L.thfhe_dag_last_group_ms(None, None) == -1


@pytest.fixture(scope="module")
def env(O):
    yield from shape_env(O, with_pack=True)


@pytest.mark.gpu
def test_group_time_survives_a_later_gate_level(env):
    import thfhe
    from thfhe import circuits as CI
    shape = SHAPES[0]
    p, K, orc, ck, pc, pk = env(shape)
    rng = np.random.default_rng(8180)
    cir = CI.Circuit()
    x = cir.inputs(3)
    g = cir.lhe_gather(0, x[0], 0, 1)
    cir.gate(0, g, x[2])                      # a gate level after the leveled group
    rec = words(rng, 2, 3, p.n + 1)
    ts = ck.tgsw_set(words(rng, 2, 1, 2 * p.l, 2, p.N), 1)
    try:
        plain = CI.evaluate_batch(ck, cir, rec, pack=pc, tgsw_sets=[ts])
        ck.set_profiling(True)
        with pytest.raises(thfhe.ThfheError):
            ck.dag_last_group_ms()            # no profiled run yet
        timed = CI.evaluate_batch(ck, cir, rec, pack=pc, tgsw_sets=[ts])
        ms = ck.dag_last_group_ms()
        print(f"\ngather group at (0, 1), 2 instances: {ms:.4f} ms")
        assert np.array_equal(timed, plain)
        assert 0.0 < ms < 1000.0
        ck.set_profiling(False)
        with pytest.raises(thfhe.ThfheError):
            ck.dag_last_group_ms()
    finally:
        ck.set_profiling(False)
        ts.close()
