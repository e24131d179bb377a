"""Long-lived contexts on the MI355X (pytest -m gpu): every call family of tests/ctx_sequence.py interleaved on ONE context, in
the orders defined there, every output word of every call against the op's CPU reference.  What this aims at is host code: a call that reads words
past what it wrote this time (after a larger call of another family they are not what a fresh allocation held), a workspace sized for fewer records
than the call writes (hidden whenever an earlier call grew the buffer further -- the cold order makes every family's large op the FIRST call on a
fresh context), a device pointer taken before the grow that replaces it, objects that must survive other calls (the TgswSets, the packing keys, a
replaced packing key), and settings or profiling state that leak from one family into the next.

One test case is one order on one freshly created context; the references are computed once per engine for the whole module."""
import numpy as np
import pytest

import ctx_sequence as CS
from support import DEFAULT_COOP, DEFAULT_RING4, KERNELS, thresholds

pytestmark = pytest.mark.gpu

ENGINES = ("sk", "MK2", "MK4-N2048", "MK64-fft")
N_FAMILIES = {"sk": 24, "MK2": 12, "MK4-N2048": 12, "MK64-fft": 12}
ORDERS = ("big-then-small", "small-big-small", "alternating", "shuffled-1", "shuffled-2")
RING = {k[0]: k for k in KERNELS if k[0] in ("ring8", "ring4")}


class World:
    """the environments and catalogues (references computed once per engine) and the one live context of the module"""

    def __init__(self, O):
        self.O, self.made, self.ck, self.dev = O, {}, None, None

    def engine(self, name):
        if name not in self.made:
            if name in ("CCS2", "KMS2"):
                env = CS.GateEnv(self.O, name)
                cat = CS.gate_sequence(env)
            else:
                env = CS.SkEnv(self.O) if name == "sk" else CS.MkEnv(self.O, name)
                cat = CS.sk_catalogue(env) if name == "sk" else CS.mk_catalogue(env)
                assert len(CS.families(cat)) == N_FAMILIES[name] and len(cat) == 2 * N_FAMILIES[name]
            extra = [CS.small_key_op(env)] if isinstance(env, CS.MkEnv) else []
            CS.references(env, cat + extra)
            self.made[name] = (env, cat, extra)
        return self.made[name]

    def close(self):
        if self.ck is not None:
            self.dev.close()
            self.ck.close()
        self.ck = self.dev = None

    def context(self, engine, **open_kw):
        """a fresh context and what lives on the device next to it, the one before closed first: never more than one alive"""
        self.close()
        env = self.engine(engine)[0]
        self.ck = env.cloud_key()
        self.dev = env.open(self.ck, **open_kw)
        return self.ck, self.dev


@pytest.fixture(scope="module")
def world(O):
    w = World(O)
    yield w
    w.close()


def run_ops(world, engine, ck, dev, seq, first, stop, between=None):
    """ops first .. stop-1 of seq on the context.  A multi-key sequence swaps the packing key at a third of its length: the D = P n key comes in, the
    tree call is refused (THFHE_E_INVALID), pack_boxes packs key-switched records on the new key, and the D = N key goes back before the first op
    that needs it, at two thirds at the latest."""
    import thfhe
    env, cat, extra = world.engine(engine)
    mk = isinstance(env, CS.MkEnv)
    for pos in range(first, stop):
        op = seq[pos]
        prev = seq[pos - 1].name if pos else "context creation"
        if mk:
            if pos == len(seq) // 3 and pos:
                dev.set_small_key()
                tree = CS.by(cat, "tree_lut_bootstrap", "small")
                with pytest.raises(thfhe.ThfheError, match="D = N"):
                    CS.tree_call(ck, dev, tree.inputs(dev))
                CS.check(extra[0].run(ck, dev), extra[0].reference(dev), extra[0], "the refused tree call", pos)
            if dev.small_key and (op.needs == "packN" or pos >= 2 * len(seq) // 3):
                dev.set_tree_key()
        if between is not None:
            between(pos, op)
        CS.check(op.run(ck, dev), op.reference(dev), op, prev, pos)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("engine", ENGINES)
def test_order_on_one_context(world, engine, order):
    seq = CS.orders(world.engine(engine)[1])[order]
    assert {op.name for op in seq} == {op.name for op in world.engine(engine)[1]}
    ck, dev = world.context(engine)
    run_ops(world, engine, ck, dev, seq, 0, len(seq))
    world.close()


@pytest.mark.parametrize("engine", ENGINES)
def test_cold_every_family_first_on_a_fresh_context(world, engine):
    # the family's large op is the first call the context ever sees, then its small one; one context alive at a time.  A multi-key context gets
    # the packing key only where the family needs it (a 256 MiB upload at N = 4096)
    env, cat, _ = world.engine(engine)
    for seq in CS.cold(cat):
        kw = dict(pack=seq[0].needs == "packN") if engine != "sk" else {}
        ck, dev = world.context(engine, **kw)
        run_ops(world, engine, ck, dev, seq, 0, 1)      # no key swap in a two-op sequence
        CS.check(seq[1].run(ck, dev), seq[1].reference(dev), seq[1], seq[0].name, 1)
    world.close()


@pytest.mark.parametrize("shape", list(RING))
def test_forced_ring_shapes_big_then_small(world, shape):
    # the single-key big-then-small order with every rotation on the eight-wave ring, and again on the four-wave ring
    seq = CS.orders(world.engine("sk")[1])["big-then-small"]
    ck, dev = world.context("sk")
    _, coop, ring4, name = RING[shape]
    with thresholds(ck, coop, ring4):
        assert ck.rotation_kernel_name(CS.LARGE) == name.format(l=dev.p.l) and ck.rotation_kernel_name(1) == name.format(l=dev.p.l)
        run_ops(world, "sk", ck, dev, seq, 0, len(seq))
    world.close()


SK_SETTINGS = [  # (setter, the non-default values it cycles through, default)
    ("set_coop_threshold", (0, 1 << 20, 6), DEFAULT_COOP), ("set_ring4_threshold", (0, 6), DEFAULT_RING4), ("set_dag_slice", (1,), 8192),
    ("set_tree_slice", (1,), 65536), ("set_wfa_chunk", (1, 3), 0),
]
MK_SETTINGS = [("set_pair_threshold", (0, 1), 256), ("set_dag_slice", (1,), 8192), ("set_tree_slice", (1,), 16384), ("set_mv_slice", (9,), 4096)]
TIMED = ("gates-nand", "gates-mux", "lut_bootstrap-theta4-index", "lut_bootstrap-theta1-noindex", "tree_lut_bootstrap")   # families whose flat call records the four events


@pytest.mark.parametrize("engine", ["sk", "MK2"])
def test_settings_and_profiling_change_no_word(world, engine):
    # before every op one more setting leaves its default (all go back to it once every one has left); profiling goes on half-way
    import thfhe
    seq = CS.orders(world.engine(engine)[1])["alternating"]
    settings = SK_SETTINGS if engine == "sk" else MK_SETTINGS
    ck, dev = world.context(engine)
    state = dict(profiling=False, timed=False, group=None, turn=0)

    def between(pos, op):
        k = pos % len(settings)
        if k == 0 and pos:
            for name, _, default in settings:
                getattr(ck, name)(default)
            state["turn"] += 1
        name, values, _ = settings[k]
        getattr(ck, name)(values[state["turn"] % len(values)])
        if pos == len(seq) // 2:
            ck.set_profiling(True)
            state.update(profiling=True, timed=False, group=False)
    try:
        for pos in range(len(seq)):
            run_ops(world, engine, ck, dev, seq, pos, pos + 1, between)
            op = seq[pos]
            if not state["profiling"]:
                continue
            if op.kind == "flat":
                state["timed"] |= op.family in TIMED
                if state["timed"]:
                    ms = ck.last_timings()
                    assert len(ms) == 4 and all(np.isfinite(v) and v >= 0 for v in ms.values()), (op.name, pos, ms)
            elif engine == "sk" and op.kind in ("dag", "dag-group") and op.family != "dag_run_batch":
                state["group"] = op.kind == "dag-group"     # the last run's last group; a run without one leaves none
            if engine == "sk":
                if state["group"]:                          # after a flat op or a gates-only dag_run_batch it is still that run's
                    ms = ck.dag_last_group_ms()
                    assert np.isfinite(ms) and ms >= 0, (op.name, pos, ms)
                else:
                    with pytest.raises(thfhe.ThfheError, match="no profiled group"):
                        ck.dag_last_group_ms()
    finally:
        ck.set_profiling(False)
        for name, _, default in settings:
            getattr(ck, name)(default)
    world.close()


@pytest.mark.parametrize("scheme", ["CCS2", "KMS2"])
def test_ccs_and_kms_nand_at_2_19_2(world, scheme):
    env, seq, _ = world.engine(scheme)
    ck, dev = world.context(scheme)
    run_ops(world, scheme, ck, dev, seq, 0, len(seq))
    world.close()
