"""The catalogue of calls and the orders of the long-lived-context tests (tests/test_gpu_ctx_sequence.py, tests/test_gpu_ctx_threads.py, and the
CPU conditions of tests/test_ctx_sequence_host.py) -- TEST INFRASTRUCTURE ONLY.  A plain module like support.py: nothing here
loads the HIP library at import time.

An Op is one call family at one size: run(ck, env) calls the engine, reference(env) the CPU models (oracle_lib and the *_reference modules, never the
engine), both return a tuple of arrays that must agree word for word.  Its inputs are uniform random words from a seed derived from the op's name, so
neither inputs nor reference depend on where the op sits in a sequence.  An environment (SkEnv, MkEnv, GateEnv) holds the keys and the oracle on
the CPU; open(ck) adds what lives on the device next to the context (the PolyContext with the packing key and the two TgswSets of the single-key
engine, the packing keys of the multi-key one, three arrays of resident device records for both), close() releases it.

Sizes: `small` is 2 samples, `large` 19 (odd, more than two eight-wave and four four-wave ring workgroups, a partial last one).  Families whose
unit is a group take the nearest admissible counts: trees count candidates (5 samples x p_hi = 4 at large, 1 sample at small), pack_boxes a multiple
of p (20 and 4 records), the DAG families 5 and 1 instances of their circuit."""
import zlib

import numpy as np

from support import N, SIGMA_BK, pmap, words

SMALL, LARGE = 2, 19
SMALL_TREE, LARGE_TREE = 1, 5
SMALL_DAG, LARGE_DAG = 1, 5
SET_COUNT, SET_D = 19, 3          # the two TgswSets every leveled family reads: 19 samples of 3 address bits
MU32, MU64 = 1 << 29, 1 << 61
SHUFFLE_SEEDS = (1, 2)            # the first two seeds tried


def rng_of(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def words64(rng, *shape):
    return rng.integers(-2**63, 2**63, size=shape, dtype=np.int64)


def index_of(rng, count, n_tables):
    """a per-sample index that spreads over the n_tables tables; a single sample takes the last table, so an index left at zero shows"""
    if count == 1:
        return np.array([n_tables - 1], np.int32)
    return rng.permutation((np.arange(count) + 1) % n_tables).astype(np.int32)


class Op:
    """family: the call family (and variant); size: 'small' / 'large'; make(rng, env) -> the inputs, a dict of arrays; call(ck, env, I) and
    model(env, I) -> tuples of arrays.  kind: 'flat', 'dag' (a dag_run_*_batch without launch groups of its own), 'dag-group' (one with a SELECT /
    TREE / MV / leveled group), 'dev' (device-buffer call, no profiling events).  needs: 'packN' for the calls that need the D = N packing key."""

    def __init__(self, family, size, make, call, model, kind="flat", needs=None):
        self.family, self.size, self.name = family, size, family + ":" + size
        self._make, self._call, self._model, self.kind, self.needs = make, call, model, kind, needs

    def inputs(self, env):
        if self.name not in env.inputs:
            env.inputs[self.name] = self._make(rng_of(env.name + "/" + self.name), env)
        return env.inputs[self.name]

    def run(self, ck, env):
        return tuple(np.asarray(a) for a in self._call(ck, env, self.inputs(env)))

    def reference(self, env):
        if self.name not in env.refs:
            env.refs[self.name] = tuple(np.asarray(a) for a in self._model(env, self.inputs(env)))
        return env.refs[self.name]

    def __repr__(self):
        return self.name


def both_sizes(family, small, large, make, call, model, **kw):
    """the two ops of a family: make(rng, env, count)"""
    return [Op(family, size, (lambda rng, env, c=c: make(rng, env, c)), call, model, **kw) for size, c in (("small", small), ("large", large))]


def stack(fn, count):
    """the per-sample model fn(s) over the samples, on threads"""
    return np.stack(pmap(fn, range(count)))


# ---- single key: SK-128 with n = 5 ---------------------------------------------------------------------------------------------------------------

class SkEnv:
    """SK-128 at n = 5: keys, oracle, packing key (the words support.make_pack makes on the same seed) and the TGSW words of the two sets"""
    name, PACK_SEED = "sk", 0x7EE0C5

    def __init__(self, O):
        from thfhe import keygen
        self.O = O
        self.kw = dict(O.PARAM_SETS["SK-128"], n=5)
        self.p = O.make_params(**self.kw)
        self.K = O.SKKeys(self.p, 0xC5E0, 2.0**-25, 2.0**-15)
        self.orc = O.Oracle(self.p, self.K.bk, self.K.ksk)
        self.pk = keygen.gen_pack_key(np.random.default_rng(self.PACK_SEED), self.K.lwe_key, self.K.rlwe_key[0], self.p.ks_t, self.p.ks_basebit, SIGMA_BK)
        self.Cs = [words(rng_of("sk/tgsw-%d" % i), SET_COUNT, SET_D, 2 * self.p.l, 2, N) for i in range(2)]
        self.inputs, self.refs = {}, {}
        self.words = self.p.n + 1
        self.resident = resident_words(self)

    def cloud_key(self):
        import thfhe
        return thfhe.CloudKey(thfhe.make_params(**self.kw), self.K.bk, self.K.ksk, device=0)

    def open(self, ck):
        """the PolyContext and the two TgswSets, created before the first op"""
        from support import make_pack
        pc, pk = make_pack(self.K, self.p, self.PACK_SEED)
        assert np.array_equal(pk, self.pk)
        return SkDevice(self, pc, [ck.tgsw_set(C, SET_D) for C in self.Cs], resident_records(ck, self))

    def pack_args(self):
        return self.pk, self.p.ks_t, self.p.ks_basebit


class SkDevice:
    """what one context's ops read on the device next to it; the CPU side is the SkEnv's"""
    def __init__(self, env, pc, sets, records):
        self.env, self.pc, self.sets, self.records = env, pc, sets, records

    def __getattr__(self, k):
        return getattr(self.env, k)

    def close(self):
        for b in self.records:
            b.free()
        for s in self.sets:
            s.close()
        self.pc.close()


def resident_words(env):
    """two operand arrays of LARGE records that live on the device for as long as the context (reserve'd device records must survive every call)"""
    r = rng_of(env.name + "/resident")
    return [words(r, LARGE, env.words) for _ in range(2)]


def resident_records(ck, env):
    """the two operand arrays uploaded ONCE, and an output array: three DeviceBuffers of LARGE records"""
    bufs = [ck.device_records(LARGE) for _ in range(3)]
    for b, a in zip(bufs, env.resident):
        b.upload(a)
    return bufs


def dev_gate_ops(env):
    """gates_dev on the first `count` resident records, after reserve(count): nothing is uploaded by the op itself"""
    O, orc = env.O, env.orc

    def call(ck, e, I):
        c = len(I["x"])
        ck.reserve(c)
        dx, dy, dout = e.records
        ck.gates_dev(O.NAND, dx, dy, None, dout, c)
        ck.sync()
        return (dout.download((c, e.words)),)
    return both_sizes("gates_dev-resident", SMALL, LARGE, lambda rng, e, c: dict(x=e.resident[0][:c], y=e.resident[1][:c]), call,
                      lambda e, I: (orc.gates(O.NAND, I["x"], I["y"]),), kind="dev")


def _recs(rng, env, count, k=1):
    return [words(rng, count, env.words) for _ in range(k)]


def sk_catalogue(env):
    import lhe_reference as LR
    import lut_reference as R
    import mv_lut_reference as MV
    import scatter_reference as SR
    import tree_lut_reference as TR
    import tree_mvk_reference as TK
    import wfa_reference as WR
    O, p, orc = env.O, env.p, env.orc
    W = env.words
    cat = []

    def xyz(k):
        return lambda rng, e, c: dict(zip("xyz", _recs(rng, e, c, k)))
    cat += both_sizes("gates-nand", SMALL, LARGE, xyz(2), lambda ck, e, I: (ck.gates(O.NAND, I["x"], I["y"]),), lambda e, I: (orc.gates(O.NAND, I["x"], I["y"]),))
    cat += both_sizes("gates-mux", SMALL, LARGE, xyz(3), lambda ck, e, I: (ck.gates(O.MUX, I["x"], I["y"], I["z"]),),
                      lambda e, I: (orc.gates(O.MUX, I["x"], I["y"], I["z"]),))

    def mk_mixed(rng, e, c):
        return dict(ops=np.array([(O.XOR, O.NAND, O.OR, O.AND)[g % 4] for g in range(c)], np.int32), x=words(rng, c, W), y=words(rng, c, W))
    cat += both_sizes("gates_mixed", SMALL, LARGE, mk_mixed, lambda ck, e, I: (ck.gates_mixed(I["ops"], I["x"], I["y"]),),
                      lambda e, I: (stack(lambda g: orc.gates(int(I["ops"][g]), I["x"][g:g + 1], I["y"][g:g + 1])[0], len(I["ops"])),))

    def call_bs(ck, e, I):
        u = ck.bootstrap_wo_keyswitch(I["x"], MU32)
        return u, ck.keyswitch(u)

    def ref_bs(e, I):
        u = stack(lambda s: orc.bootstrap_wo_keyswitch(I["x"][s], MU32), len(I["x"]))
        return u, stack(lambda s: orc.keyswitch(u[s]), len(u))
    cat += both_sizes("bootstrap_wo_keyswitch+keyswitch", SMALL, LARGE, xyz(1), call_bs, ref_bs)

    # programmable bootstraps: three tables; theta = 4 with a per-sample index, theta = 1 without one (table 0 whatever an earlier call left)
    def mk_lut(rng, e, c):
        return dict(tv=words(rng, 3, N), x=words(rng, c, W), y=words(rng, c, W), idx=index_of(rng, c, 3), bias=int(rng.integers(-2**31, 2**31)))
    cat += both_sizes("lut_bootstrap-theta4-index", SMALL, LARGE, mk_lut,
                      lambda ck, e, I: (ck.lut_bootstrap(I["tv"], I["x"], I["y"], weights=(3, -2), bias=I["bias"], theta=4, lut_index=I["idx"]),),
                      lambda e, I: (stack(lambda s: R.lut_bootstrap(orc, [I["x"][s], I["y"][s]], (3, -2), I["bias"], I["tv"][I["idx"][s]], 4), len(I["x"])),))
    cat += both_sizes("lut_bootstrap-theta1-noindex", SMALL, LARGE, mk_lut,
                      lambda ck, e, I: (ck.lut_bootstrap(I["tv"], I["x"], theta=1, lut_index=None),),
                      lambda e, I: (stack(lambda s: R.lut_bootstrap(orc, [I["x"][s]], (1,), 0, I["tv"][0], 1), len(I["x"])),))

    def mk_enc(rng, e, c):
        return dict(ta=words(rng, 3, N), tb=words(rng, 3, N), x=words(rng, c, W), idx=index_of(rng, c, 3))
    cat += both_sizes("lut_bootstrap_enc", SMALL, LARGE, mk_enc,
                      lambda ck, e, I: (ck.lut_bootstrap_enc(I["ta"], I["tb"], I["x"], weights=(-5,), theta=2, lut_index=I["idx"]),),
                      lambda e, I: (stack(lambda s: TR.lut_enc(orc, [I["x"][s]], (-5,), 0, I["ta"][I["idx"][s]], I["tb"][I["idx"][s]], 2), len(I["x"])),))

    def mk_tree(rng, e, c):
        return dict(tv1=words(rng, 2, 2, N), lo=words(rng, c, W), hi=words(rng, c, W), idx=index_of(rng, c, 2), blo=int(rng.integers(-2**31, 2**31)))
    cat += both_sizes("tree_lut_bootstrap", SMALL_TREE, LARGE_TREE, mk_tree,
                      lambda ck, e, I: (ck.tree_lut_bootstrap(e.pc, I["tv1"], I["lo"], I["hi"], p_hi=4, weights_lo=(3,), bias_lo=I["blo"], theta=2,
                                                              weights_hi=(-5,), table_index=I["idx"]),),
                      lambda e, I: (stack(lambda s: TR.tree(orc, *e.pack_args(), [I["lo"][s]], (3,), I["blo"], 2, [I["hi"][s]], (-5,), 0,
                                                            I["tv1"][I["idx"][s]], 4)[0], len(I["lo"])),))

    # multi-value: q = 9 outputs, p = 16 taps, two factor tables, with and without a table index
    def mk_mv(rng, e, c):
        return dict(tv0=words(rng, N), fac=words(rng, 2, 9, 16), x=words(rng, c, W), idx=index_of(rng, c, 2))
    for fam, with_idx in (("mv_lut_bootstrap-index", True), ("mv_lut_bootstrap-noindex", False)):
        cat += both_sizes(fam, SMALL, LARGE, mk_mv,
                          lambda ck, e, I, w=with_idx: (ck.mv_lut_bootstrap(I["fac"], I["x"], tv0=I["tv0"], table_index=I["idx"] if w else None),),
                          lambda e, I, w=with_idx: (stack(lambda s: MV.mv_lut(orc, [I["x"][s]], (1,), 0, I["tv0"], I["fac"][I["idx"][s] if w else 0]), len(I["x"])),))

    def mk_tmv(rng, e, c):
        return dict(tv0=words(rng, N), fac=words(rng, 2, 4, 8), fack=words(rng, 2, 2, 4, 8), lo=words(rng, c, W), hi=words(rng, c, W), idx=index_of(rng, c, 2))
    cat += both_sizes("tree_lut_bootstrap_mv", SMALL_TREE, LARGE_TREE, mk_tmv,
                      lambda ck, e, I: (ck.tree_lut_bootstrap_mv(e.pc, I["fac"], I["lo"], I["hi"], tv0=I["tv0"], weights_hi=(7,), table_index=I["idx"]),),
                      lambda e, I: (stack(lambda s: MV.tree_mv(orc, *e.pack_args(), [I["lo"][s]], (1,), 0, [I["hi"][s]], (7,), 0, I["tv0"],
                                                               I["fac"][I["idx"][s]])[0], len(I["lo"])),))
    cat += both_sizes("tree_lut_bootstrap_mvk", SMALL_TREE, LARGE_TREE, mk_tmv,
                      lambda ck, e, I: (ck.tree_lut_bootstrap_mvk(e.pc, I["fack"], I["lo"], I["hi"], tv0=I["tv0"], weights_hi=(7,), table_index=I["idx"]),),
                      lambda e, I: (stack(lambda s: TK.tree_mvk(orc, *e.pack_args(), [I["lo"][s]], (1,), 0, [I["hi"][s]], (7,), 0, I["tv0"],
                                                                I["fack"][I["idx"][s]])[0], len(I["lo"])),))

    # leveled calls on the two TgswSets: the large ops read every sample, the small ones a window (lookup, wfa, scatter) or the first two
    A, B = env.Cs
    first_of = lambda c: 0 if c == SET_COUNT else 7

    def mk_cmux(rng, e, c):
        return dict(d1=words(rng, c, 2 * N), d0=words(rng, c, 2 * N))
    cat += both_sizes("lhe_cmux", SMALL, LARGE, mk_cmux,
                      lambda ck, e, I: (np.concatenate(ck.lhe_cmux(e.sets[0], 1, I["d1"][:, :N], I["d1"][:, N:], I["d0"][:, :N], I["d0"][:, N:]), axis=1),),
                      lambda e, I: (stack(lambda s: LR.cmux(p, A[s][1], I["d1"][s], I["d0"][s]), len(I["d1"])),))

    def mk_lookup(rng, e, c):
        return dict(ta=words(rng, 3, 4, N), tb=words(rng, 3, 4, N), idx=index_of(rng, c, 3))
    for fam, enc in (("lhe_lookup-encrypted", True), ("lhe_lookup-public", False)):
        cat += both_sizes(fam, SMALL, LARGE, mk_lookup,
                          lambda ck, e, I, enc=enc: (ck.lhe_lookup(e.sets[0], I["tb"], d_tree=2, d_rot=1, theta=2, tab_a=I["ta"] if enc else None, table_index=I["idx"],
                                                                   first=first_of(len(I["idx"])), count=len(I["idx"])),),
                          lambda e, I, enc=enc: (stack(lambda s: LR.lookup(orc, A[first_of(len(I["idx"])) + s], I["ta"][I["idx"][s]] if enc else None, I["tb"][I["idx"][s]],
                                                                           2, 1, 2), len(I["idx"])),))

    trans = np.array([[[1, 2], [2, 2], [3, 0], [4, 1], [0, 4]], [[2, 3], [0, 0], [4, 1], [1, 3], [3, 2]], [[4, 0], [3, 1], [2, 2], [0, 4], [1, 3]]], np.int32)
    step_bit = np.array([0, 16 + 1, 2], np.int32)      # bit 0 of set 0, bit 1 of set 1, bit 2 of set 0
    start = np.array([0, 3], np.int32)

    def mk_wfa(rng, e, c):
        return dict(fa=words(rng, 2, 5, N), fb=words(rng, 2, 5, N), idx=index_of(rng, c, 2))
    cat += both_sizes("lhe_wfa", SMALL, LARGE, mk_wfa,
                      lambda ck, e, I: (ck.lhe_wfa(e.sets, trans, step_bit, I["fb"], start, theta=2, fin_a=I["fa"], table_index=I["idx"], first=first_of(len(I["idx"])),
                                                   count=len(I["idx"])),),
                      lambda e, I: (stack(lambda s: WR.wfa(orc, [A[first_of(len(I["idx"])) + s], B[first_of(len(I["idx"])) + s]], trans, step_bit, I["fa"][I["idx"][s]],
                                                           I["fb"][I["idx"][s]], 2, start).reshape(2, 2, -1), len(I["idx"])),))

    def mk_demux(rng, e, c):
        return dict(x=words(rng, c, 2 * N))

    def ref_demux(e, I):
        r = pmap(lambda s: SR.demux(p, B[s][2], I["x"][s]), range(len(I["x"])))
        return np.stack([a for a, _ in r]), np.stack([b for _, b in r])

    def call_demux(ck, e, I):
        a0, b0, a1, b1 = ck.lhe_demux(e.sets[1], 2, I["x"][:, N:], I["x"][:, :N])
        return np.concatenate([a0, b0], axis=1), np.concatenate([a1, b1], axis=1)
    cat += both_sizes("lhe_demux", SMALL, LARGE, mk_demux, call_demux, ref_demux)

    def mk_scatter(rng, e, c):
        return dict(v=words(rng, c, 2 * N), idx=index_of(rng, c, 2))

    def call_scatter(ck, e, I):
        c = len(I["idx"])
        ta, tb = ck.lhe_scatter(e.sets[1], I["v"][:, N:], d_tree=2, d_rot=1, val_a=I["v"][:, :N], n_tables=2, table_index=I["idx"], first=first_of(c), count=c)
        return (np.concatenate([ta, tb], axis=-1),)

    def ref_scatter(e, I):
        c, f = len(I["idx"]), first_of(len(I["idx"]))
        leaves = pmap(lambda s: SR.scatter_wo_reduce(p, B[f + s], I["v"][s], 2, 1), range(c))
        tab = np.zeros((2, 4, 2 * N), np.int64)
        for s in range(c):
            tab[I["idx"][s]] += leaves[s]
        return (tab.astype(np.uint32).view(np.int32),)
    cat += both_sizes("lhe_scatter", SMALL, LARGE, mk_scatter, call_scatter, ref_scatter)

    cat += sk_dag_ops(env, trans, step_bit, start)
    cat += dev_gate_ops(env)
    return cat


def sk_dag_ops(env, trans, step_bit, start):
    """the five gate-DAG entries, each on the smallest circuit that holds its node kinds, at 1 and 5 instances"""
    import dag_lhe_reference as DL
    import dag_lut_reference as DLUT
    import dag_mv_reference as DM
    import dag_tree_reference as DT
    from thfhe import circuits as CI
    O, orc = env.O, env.orc
    W = env.words
    r = rng_of("sk/dag-circuits")

    gates = CI.Circuit()
    x = gates.inputs(3)
    g0, g1 = gates.gate(O.NAND, x[0], x[1]), gates.gate(O.XOR, x[1], x[2])
    gates.gate(O.AND, gates.gate(O.MUX, g0, g1, x[0]), g0)

    lut = CI.Circuit()
    x = lut.inputs(2)
    l = lut.lut(lut.table(words(r, N)), [lut.gate(O.NAND, x[0], x[1]), x[0]], weights=(2, 1), bias=77, theta=2)
    lut.gate(O.XOR, l[0], l[1])

    tree = CI.Circuit()
    x = tree.inputs(2)
    tree.lut_enc(tree.enc_table(words(r, N), words(r, N)), [x[0]], weights=(3,), theta=2)
    tree.tree(tree.tree_rows(words(r, 2, N)), [x[0]], [x[1]], 4, lo_weights=(5,), theta1=2)
    tree.select([x[1]], 0, 2)

    mv = CI.Circuit()
    x = mv.inputs(2)
    m = mv.mv(mv.mv_base(words(r, N)), words(r, 3, 4), [x[0], x[1]], weights=(3, -2), bias=12345)
    mv.gate(O.NAND, m[0], m[1])
    mv.tree_mv(mv.mv_base(words(r, N)), words(r, 2, 2, 4), [m[2]], [x[0]])

    lhe = CI.Circuit()
    x = lhe.inputs(3)
    g = [lhe.gate((O.NAND, O.XOR, O.AND, O.OR)[i % 4], x[i % 3], x[(i + 1) % 3]) for i in range(8)]
    lhe.lhe_gather(0, g[0], 1, 2)
    lhe.lhe_lookup(1, lhe.lhe_table(words(r, 4, N), words(r, 4, N)), 2, 1, theta=2)
    lhe.lhe_wfa((trans, step_bit, None, start), [0, 1], lhe.lhe_finals(words(r, 5, N)), theta=2)

    def make(cir):
        return lambda rng, e, c: dict(x=words(rng, c, cir.n_inputs, W))

    def call(cir):
        return lambda ck, e, I: (CI.evaluate_batch(ck, cir, I["x"], pack=e.pc, tgsw_sets=e.sets),)
    ops = []
    for fam, cir, kind, model in (
            ("dag_run_batch", gates, "dag", lambda e, x: DLUT.evaluate(orc, gates, x)),
            ("dag_run_lut_batch", lut, "dag", lambda e, x: DLUT.evaluate(orc, lut, x)),
            ("dag_run_tree_batch", tree, "dag-group", lambda e, x: DT.evaluate(orc, tree, x, *e.pack_args())),
            ("dag_run_mv_batch", mv, "dag-group", lambda e, x: DM.evaluate(orc, mv, x, *e.pack_args())),
            ("dag_run_lhe_batch", lhe, "dag-group", None)):
        if model is None:
            ref = lambda e, I: (stack(lambda q: DL.evaluate(orc, lhe, I["x"][q], [C[q] for C in e.Cs], *e.pack_args()), len(I["x"])),)
        else:
            ref = lambda e, I, model=model: (stack(lambda q: model(e, I["x"][q]), len(I["x"])),)
        ops += both_sizes(fam, SMALL_DAG, LARGE_DAG, make(cir), call(cir), ref, kind=kind)
    return ops


# ---- the 3-gen multi-key engine ------------------------------------------------------------------------------------------------------------------

MK_SETS = {"MK2": dict(n=3, parties=2), "MK4-N2048": dict(n=2, parties=2), "MK64-fft": dict(n=2, parties=2)}


class MkEnv:
    """a 3-gen set at a short mask and two parties: keys, oracle, and two packing keys of random words -- the D = N key the tree needs (word
    equality is all that is asserted) and the D = P n key that replaces it mid-sequence"""

    def __init__(self, O, set_name):
        self.O, self.set_name, self.name = O, set_name, "mk/" + set_name
        self.p = O.make_params(set_name, **MK_SETS[set_name])
        s = O.SIGMAS[set_name]
        self.K = O.MKKeys(self.p, 0xC5E1, s["bk"], s["ks"])
        self.orc = O.MKOracle(self.p, self.K.bk, self.K.ksk)
        self.words = self.p.parties * self.p.n + 1
        self.t, self.basebit = (2, 1) if self.p.N == 1024 else (1, 1)      # the D = N key holds N t 2 N words: 32 MiB, 64 MiB, 256 MiB
        r = rng_of(self.name + "/pack-keys")
        self.pk = words64(r, self.p.N, self.t, 1, 2, self.p.N)
        self.pk_small = words64(r, self.words - 1, 2, 3, 2, self.p.N)      # D = P n, (t, basebit) = (2, 2)
        self.inputs, self.refs = {}, {}
        self.resident = resident_words(self)

    def cloud_key(self):
        import thfhe
        return thfhe.MKCloudKey(thfhe.make_params(**self.p.as_dict()), self.K.bk, self.K.ksk, device=0)

    def open(self, ck, pack=True):
        """pack: upload the D = N packing key now (it then has to survive every other call)"""
        if pack:
            ck.pack_key_set(self.pk, self.t, self.basebit)
        return MkDevice(self, ck)


class MkDevice:
    def __init__(self, env, ck):
        self.env, self.ck, self.small_key, self.records = env, ck, False, resident_records(ck, env)

    def __getattr__(self, k):
        return getattr(self.env, k)

    def set_small_key(self):
        self.ck.pack_key_set(self.pk_small, 2, 2)
        self.small_key = True

    def set_tree_key(self):
        self.ck.pack_key_set(self.pk, self.t, self.basebit)
        self.small_key = False

    def close(self):
        for b in self.records:
            b.free()


def mk_catalogue(env):
    import mk_lut_reference as R
    import mk_mv_lut_reference as MV
    import mk_pack_reference as MP
    from thfhe import circuits as CI
    O, p, orc, W = env.O, env.p, env.orc, env.words
    NN = p.N
    cat = []

    def xyz(k):
        return lambda rng, e, c: dict(zip("xyz", _recs(rng, e, c, k)))
    cat += both_sizes("gates-nand", SMALL, LARGE, xyz(2), lambda ck, e, I: (ck.gates(O.NAND, I["x"], I["y"]),), lambda e, I: (orc.gates(O.NAND, I["x"], I["y"]),))
    cat += both_sizes("gates-mux", SMALL, LARGE, xyz(3), lambda ck, e, I: (ck.gates(O.MUX, I["x"], I["y"], I["z"]),),
                      lambda e, I: (orc.gates(O.MUX, I["x"], I["y"], I["z"]),))
    cat += both_sizes("bootstrap", SMALL, LARGE, xyz(1), lambda ck, e, I: (ck.bootstrap(I["x"], MU64),),
                      lambda e, I: (stack(lambda s: orc.keyswitch(orc.bootstrap_wo_keyswitch(I["x"][s], MU64)), len(I["x"])),))

    def mk_lut(rng, e, c):
        return dict(tv=words64(rng, 3, NN), x=words(rng, c, W), y=words(rng, c, W), idx=index_of(rng, c, 3), bias=int(rng.integers(-2**31, 2**31)))
    cat += both_sizes("lut_bootstrap-theta4-index", SMALL, LARGE, mk_lut,
                      lambda ck, e, I: (ck.lut_bootstrap(I["tv"], I["x"], I["y"], weights=(3, -2), bias=I["bias"], theta=4, lut_index=I["idx"]),),
                      lambda e, I: (stack(lambda s: R.lut_bootstrap(orc, [I["x"][s], I["y"][s]], (3, -2), I["bias"], I["tv"][I["idx"][s]], 4), len(I["x"])),))
    cat += both_sizes("lut_bootstrap-theta1-noindex", SMALL, LARGE, mk_lut,
                      lambda ck, e, I: (ck.lut_bootstrap(I["tv"], I["x"], theta=1, lut_index=None),),
                      lambda e, I: (stack(lambda s: R.lut_bootstrap(orc, [I["x"][s]], (1,), 0, I["tv"][0], 1), len(I["x"])),))

    def mk_mv(rng, e, c):
        return dict(tv0=words64(rng, NN), fac=words(rng, 2, 9, 8), x=words(rng, c, W), idx=index_of(rng, c, 2), ob=int(words64(rng, 1)[0]))
    cat += both_sizes("mv_lut_bootstrap", SMALL, LARGE, mk_mv,
                      lambda ck, e, I: (ck.mv_lut_bootstrap(I["fac"], I["x"], tv0=I["tv0"], table_index=I["idx"], out_bias=I["ob"]),),
                      lambda e, I: (stack(lambda s: MV.mv_lut(orc, [I["x"][s]], (1,), 0, I["tv0"], I["fac"][I["idx"][s]], I["ob"]), len(I["x"])),))

    def ref_pack(e, I):
        r = pmap(lambda g: MP.pack(I["recs"][4 * g:4 * g + 4], e.pk, e.t, e.basebit, 4), range(len(I["recs"]) // 4))
        return np.concatenate([a for a, _ in r]), np.concatenate([b for _, b in r])
    cat += both_sizes("pack_boxes", 4, 20, lambda rng, e, c: dict(recs=words(rng, c, NN + 1)), lambda ck, e, I: ck.pack_boxes(I["recs"], 4), ref_pack, needs="packN")

    def mk_enc(rng, e, c):
        return dict(ta=words64(rng, 3, NN), tb=words64(rng, 3, NN), x=words(rng, c, W), idx=index_of(rng, c, 3))
    cat += both_sizes("lut_bootstrap_enc", SMALL, LARGE, mk_enc,
                      lambda ck, e, I: (ck.lut_bootstrap_enc(I["ta"], I["tb"], I["x"], weights=(-5,), theta=2, lut_index=I["idx"]),),
                      lambda e, I: (stack(lambda s: MP.lut_bootstrap_enc(orc, [I["x"][s]], (-5,), 0, I["ta"][I["idx"][s]], I["tb"][I["idx"][s]], 2), len(I["x"])),))

    def mk_tree(rng, e, c):
        return dict(tv1=words64(rng, 2, 2, NN), lo=words(rng, c, W), hi=words(rng, c, W), idx=index_of(rng, c, 2), blo=int(rng.integers(-2**31, 2**31)))
    cat += both_sizes("tree_lut_bootstrap", SMALL_TREE, LARGE_TREE, mk_tree, tree_call,
                      lambda e, I: (stack(lambda s: MP.tree(orc, e.pk, e.t, e.basebit, I["tv1"][I["idx"][s]], [I["lo"][s]], [I["hi"][s]], 4, (3,), I["blo"], 2, (-5,), 0),
                                          len(I["lo"])),), needs="packN")

    # the circuit of tests/test_gpu_mk_dag_mv.py: an MV node, a NAND of two of its outputs, a LUT node on the third
    r = rng_of(env.name + "/dag-circuit")
    tv0, fac, tv, ob = words64(r, NN), words(r, 3, 4), words64(r, NN), int(words64(r, 1)[0])
    cir = CI.Circuit()
    a, b = cir.inputs(2)
    m = cir.mv(cir.mv_base(tv0), fac, [a, b], weights=(3, -2), bias=12345, out_bias=ob)
    cir.gate(O.NAND, m[0], m[1])
    cir.lut(cir.table(tv), [m[2]])

    def ref_dag(e, I):
        def one(q):
            x = I["x"][q]
            r_mv = MV.mv_lut(orc, [x[0], x[1]], (3, -2), 12345, tv0, fac, ob)
            return np.concatenate([x, r_mv, orc.gates(O.NAND, r_mv[0:1], r_mv[1:2]), R.lut_bootstrap(orc, [r_mv[2]], (1,), 0, tv, 1)])
        return (stack(one, len(I["x"])),)
    cat += both_sizes("dag_run_mv_batch", SMALL_DAG, LARGE_DAG, lambda rng, e, c: dict(x=words(rng, c, 2, W)),
                      lambda ck, e, I: (CI.evaluate_batch(ck, cir, I["x"]),), ref_dag, kind="dag")

    def ref_partial(e, I):
        def one(s):
            x = I["x"][s].copy()
            x[-1] = 0
            return MV.rotate(orc, x, np.full(NN, MU64, np.int64)).reshape(2, NN)
        return (stack(one, len(I["x"])),)

    def call_partial(ck, e, I):
        from support import mk_rotate_dev
        return (mk_rotate_dev(ck, p, I["x"], MU64),)
    cat += both_sizes("rotate_partial_dev", SMALL, LARGE, xyz(1), call_partial, ref_partial, kind="dev")
    cat += dev_gate_ops(env)
    return cat


def tree_call(ck, e, I):
    """the multi-key tree op's call, also what must be refused under the D = P n key"""
    return (ck.tree_lut_bootstrap(I["tv1"], I["lo"], I["hi"], p_hi=4, weights_lo=(3,), bias_lo=I["blo"], theta=2, weights_hi=(-5,), table_index=I["idx"]),)


def small_key_op(env):
    """pack_boxes under the D = P n key: four key-switched records into one table, against the model on that key"""
    import mk_pack_reference as MP
    return Op("pack_boxes-small-key", "small", lambda rng, e: dict(recs=words(rng, 4, e.words)), lambda ck, e, I: ck.pack_boxes(I["recs"], 4),
              lambda e, I: MP.pack(I["recs"], e.pk_small, 2, 2, 4))


# ---- CCS and KMS: NAND at counts 2, 19, 2 on one context -------------------------------------------------------------------------------------------

class GateEnv:
    """CCS2 or KMS2 at n = 3: keys, oracle, and the three NAND ops (small, large, small again on other inputs)"""

    def __init__(self, O, scheme):
        self.O, self.scheme, self.name = O, scheme, scheme
        self.inputs, self.refs = {}, {}
        if scheme == "CCS2":
            self.p = O.make_params("CCS2", n=3)
            s = O.SIGMAS["CCS2"]
            self.K = O.CCSKeys(self.p, 0xC5E2, s["bk"], s["ks"])
            self.orc = O.CCSOracle(self.p, self.K)
        else:
            import thfhe
            from thfhe import keygen
            self.p = thfhe.make_kms_params("KMS2", n=3)
            self.K = K = keygen.KMSSecretKeySet(self.p, seed=0xC5E3)
            self.orc = O.KMSOracle(self.p, K.gsw, K.uni, K.pk, K.crs, K.ksk)
        self.words = self.p.parties * self.p.n + 1

    def cloud_key(self):
        import thfhe
        K = self.K
        if self.scheme == "CCS2":
            return thfhe.CCSCloudKey(thfhe.make_params(**self.p.as_dict()), K.bk, K.pk, K.crs, K.ksk, device=0)
        from thfhe import kms
        return kms.KMSCloudKey(self.p, K.gsw, K.uni, K.pk, K.crs, K.ksk, device=0)

    def open(self, ck):
        return self

    def close(self):
        pass


def gate_sequence(env):
    O, orc = env.O, env.orc
    mk = lambda rng, e, c: dict(x=words(rng, c, e.words), y=words(rng, c, e.words))
    ops = [Op("gates-nand-%d" % i, size, (lambda rng, e, c=c: mk(rng, e, c)), lambda ck, e, I: (ck.gates(O.NAND, I["x"], I["y"]),),
              lambda e, I: (orc.gates(O.NAND, I["x"], I["y"]),)) for i, (size, c) in enumerate((("small", SMALL), ("large", LARGE), ("small", SMALL)))]
    return ops


# ---- the orders ----------------------------------------------------------------------------------------------------------------------------------

def families(cat):
    return list(dict.fromkeys(op.family for op in cat))


def by(cat, family, size):
    return next(op for op in cat if op.family == family and op.size == size)


def cold(cat):
    """one sequence per family, each for a context of its own: the family's large op as the first call, then its small one"""
    return [[by(cat, f, "large"), by(cat, f, "small")] for f in families(cat)]


def big_then_small(cat):
    """every large op in catalogue order, then every small one: stale tails everywhere"""
    return [op for op in cat if op.size == "large"] + [op for op in cat if op.size == "small"]


def small_big_small(cat):
    """family by family small, large, small: buffers grow in mid-life"""
    return [by(cat, f, s) for f in families(cat) for s in ("small", "large", "small")]


def alternating(cat):
    """large of family k, then small of family k + 1: every family's small op runs directly after another family's large one"""
    fam = families(cat)
    return [op for k, f in enumerate(fam) for op in (by(cat, f, "large"), by(cat, fam[(k + 1) % len(fam)], "small"))]


def shuffled(cat, seed):
    return [cat[i] for i in np.random.default_rng(seed).permutation(len(cat))]


def orders(cat):
    """name -> sequence, every order that runs on ONE context"""
    o = {"big-then-small": big_then_small(cat), "small-big-small": small_big_small(cat), "alternating": alternating(cat)}
    for s in SHUFFLE_SEEDS:
        o["shuffled-%d" % s] = shuffled(cat, s)
    return o


def segments(seq, size):
    return [seq[i:i + size] for i in range(0, len(seq), size)]


def check(got, ref, op, prev, pos):
    """every output word of op against its reference; the message names the op, the one before it and the position"""
    from support import differing
    assert len(got) == len(ref), (op.name, "outputs", len(got), len(ref))
    for k, (g, r) in enumerate(zip(got, ref)):
        assert g.shape == r.shape and g.dtype == r.dtype, "%s (after %s, position %d): output %d is %s %s, the reference %s %s" % (
            op.name, prev, pos, k, g.dtype, g.shape, r.dtype, r.shape)
        assert np.array_equal(g, r), "%s (after %s, position %d): output %d differs at %s" % (op.name, prev, pos, k, differing(g, r))


def references(env, cat):
    """every reference of the catalogue, once, on threads"""
    for op in cat:
        op.inputs(env)
    pmap(lambda op: op.reference(env), [op for op in cat if op.name not in env.refs])
