"""LUT nodes in the gate-DAG executor, host side (no GPU): Circuit.lut wire numbering, spec / table dedup and the 6-column node rows;
levels() / census() of mixed circuits; the row checks of thfhe_dag_run_lut_batch / thfhe_mk_dag_run_lut_batch, which run before the context
is looked at; and the CPU yardstick (tests/dag_lut_reference.py) decrypting a LUT adder and a gate / LUT conversion chain on reduced keys."""
import ctypes as C

import numpy as np
import pytest

import dag_lut_reference as DR
import lut_reference as R

I32, I64 = C.POINTER(C.c_int32), C.POINTER(C.c_int64)


def test_lut_node_rows_wires_and_dedup():
    import thfhe
    from thfhe import circuits as Cc, lut
    c = Cc.Circuit()
    x = c.inputs(3)
    t_add = c.table(Cc.adder_table())
    t_id = c.table(lut.test_vector(lut.int_outputs(lambda m: m, 4), 4))
    assert c.table(Cc.adder_table()) == t_add and t_add != t_id and len(c.tables) == 2
    o1 = c.lut(t_add, [x[0], x[1]], weights=(1, 1), theta=2)
    g = c.gate(thfhe.NAND, o1[0], x[2])
    o2 = c.lut(t_id, [x[2]], theta=4)
    o3 = c.lut(t_add, [x[1], x[2]], weights=(1, 1), theta=2)   # same spec as o1: deduplicated
    o4 = c.lut(t_id, [x[0], x[1], g], weights=(1, -2, 3), bias=-5)
    assert o1 == [3, 4] and g == 5 and o2 == [6, 7, 8, 9] and o3 == [10, 11] and o4 == [12]
    assert c.specs == [(2, (1, 1, 0), 0, 2), (1, (1, 0, 0), 0, 4), (3, (1, -2, 3), -5, 1)]
    nodes = c.nodes()
    assert nodes.dtype == np.int32 and nodes.shape == (10, 6)
    assert nodes.tolist() == [
        [thfhe.LUT, 0, 1, -1, 0, t_add], [thfhe.LUT_OUT, 3, -1, -1, -1, -1],
        [thfhe.NAND, 3, 2, -1, -1, -1],
        [thfhe.LUT, 2, -1, -1, 1, t_id]] + [[thfhe.LUT_OUT, 6, -1, -1, -1, -1]] * 3 + [
        [thfhe.LUT, 1, 2, -1, 0, t_add], [thfhe.LUT_OUT, 10, -1, -1, -1, -1],
        [thfhe.LUT, 0, 1, 5, 2, t_id]]
    assert np.array_equal(nodes[:, :4], np.array(c.gates, np.int32))
    with pytest.raises(ValueError):
        c.lut(t_id, [x[0]], theta=3)
    with pytest.raises(ValueError):
        c.lut(t_id, [x[0], x[1]], weights=(1,))
    with pytest.raises(ValueError):
        c.lut(7, [x[0]])


def test_levels_and_census_of_mixed_circuits():
    import thfhe
    from thfhe import circuits as Cc
    c = Cc.Circuit()
    a, b = c.inputs(2)
    t = c.table(Cc.adder_table())
    s, cy = c.lut(t, [a, b], weights=(1, 1), theta=2)      # level 1
    n = c.gate(thfhe.NOT, cy)                                # free, on the LUT's level
    g = c.gate(thfhe.AND, s, n)                              # level 2
    s2, cy2 = c.lut(t, [s, cy, g], weights=(1, 1, 1), theta=2)   # level 3
    m = c.gate(thfhe.MUX, cy2, s2, a)                        # level 4
    gi = lambda w: w - c.n_inputs
    assert c.levels() == [[gi(s), gi(cy)], [gi(n)], [gi(g)], [gi(s2), gi(cy2)], [gi(m)]]
    assert c.census() == dict(gates=7, bootstrapped=4, mux=1, rotations=5, depth=4, luts=2)


def test_gate_only_circuits_are_unchanged():
    import thfhe
    from thfhe import circuits as Cc
    c = Cc.Circuit()
    a, b, cin = c.inputs(3), c.inputs(3), c.inputs(1)[0]
    s, carry = Cc.full_adder(c, a, b, cin)
    c.gate(thfhe.NOT, s[0])
    assert not c.has_luts() and c.tables == [] and c.specs == []
    assert c.census() == dict(gates=15, bootstrapped=14, mux=0, rotations=14, depth=6)
    assert sum(len(l) for l in c.levels()) == 15 and len(c.levels()) == 7
    nodes = c.nodes()
    assert np.array_equal(nodes[:, :4], np.array(c.gates, np.int32).reshape(-1, 4)) and np.all(nodes[:, 4:] == -1)


def _call(L, mk, nodes, n_inputs=3, specs=None, n_specs=None, tv=True, n_luts=2, out_wires=None):
    import thfhe
    specs = [(1, (1, 0, 0), 0, 1), (2, (1, 1, 0), 0, 2), (3, (1, 1, 1), 0, 4)] if specs is None else specs
    sp = (thfhe.LutSpec * max(len(specs), 1))(*[thfhe.LutSpec(n, (C.c_int32 * 3)(*w), b, t) for n, w, b, t in specs])
    nodes = np.ascontiguousarray(nodes, np.int32).reshape(-1, 6)
    words = 1041 if mk else 631
    x = np.zeros((1, n_inputs, words), np.int32)
    out = np.zeros((1, max(nodes.shape[0], 1), words), np.int32)
    tab = np.zeros((2, 1024), np.int64 if mk else np.int32)
    ptv = tab.ctypes.data_as(I64 if mk else I32) if tv else None
    sel = None if out_wires is None else np.ascontiguousarray(out_wires, np.int32)
    fn = L.thfhe_mk_dag_run_lut_batch if mk else L.thfhe_dag_run_lut_batch
    rc = fn(None, x.ctypes.data_as(I32), n_inputs, nodes.ctypes.data_as(I32), nodes.shape[0], sp if specs else None,
            len(specs) if n_specs is None else n_specs, ptv, n_luts, 1, None if sel is None else sel.ctypes.data_as(I32),
            0 if sel is None else len(sel), out.ctypes.data_as(I32), None)
    return rc, L.thfhe_last_error().decode()


LUT, LUT_OUT, NAND, NOT, AND3, XNOR = 14, 15, 0, 11, 13, 4
OK_ROWS = [[LUT, 0, 1, -1, 1, 0], [LUT_OUT, 3, -1, -1, -1, -1], [NAND, 3, 4, -1, -1, -1], [LUT, 2, -1, -1, 0, 1], [NOT, 6, -1, -1, -1, -1]]


@pytest.mark.parametrize("mk", [False, True])
def test_lut_dag_rejections_without_a_device(mk):
    import thfhe
    L = thfhe.lib()

    def bad(rule, nodes, **kw):
        rc, msg = _call(L, mk, nodes, **kw)
        assert rc == thfhe_e_invalid and rule in msg, (rule, msg)

    thfhe_e_invalid = -1
    bad("null", OK_ROWS, tv=False)
    bad("null", OK_ROWS, specs=[], n_specs=1)
    bad("n_specs", OK_ROWS, n_specs=0)
    bad("n_specs", OK_ROWS, n_specs=1025)
    for n_luts in (0, -1, 1025):
        bad("n_luts", OK_ROWS, n_luts=n_luts)
    bad("n_inputs", OK_ROWS, specs=[(1, (1, 0, 0), 0, 1), (4, (1, 1, 0), 0, 2)])
    bad("theta", OK_ROWS, specs=[(1, (1, 0, 0), 0, 3), (2, (1, 1, 0), 0, 2)])
    bad("output wire", OK_ROWS, out_wires=[0, 8])
    bad("output wire", OK_ROWS, out_wires=[-1])
    bad("spec index", [[LUT, 0, -1, -1, 3, 0]])
    bad("spec index", [[LUT, 0, -1, -1, -1, 0]])
    bad("table index", [[LUT, 0, -1, -1, 0, 2]])
    bad("table index", [[LUT, 0, -1, -1, 0, -1]])
    bad("operands do not match", [[LUT, 0, -1, -1, 1, 0], [LUT_OUT, 3, -1, -1, -1, -1]])     # spec 1 names two inputs
    bad("operands do not match", [[LUT, 0, 1, -1, 0, 0]])                                    # spec 0 names one
    bad("operands do not match", [[LUT, 0, -1, 2, 0, 0]])
    bad("missing LUT_OUT", [[LUT, 0, 1, -1, 1, 0]])                                          # theta 2 at the end
    bad("missing LUT_OUT", [[LUT, 0, 1, -1, 1, 0], [NAND, 0, 1, -1, -1, -1]])
    bad("missing LUT_OUT", [[LUT, 0, 1, 2, 2, 0], [LUT_OUT, 3, -1, -1, -1, -1], [LUT_OUT, 3, -1, -1, -1, -1]])
    bad("without a LUT node", [[LUT, 0, -1, -1, 0, 0], [LUT_OUT, 3, -1, -1, -1, -1]])         # extra (theta 1)
    bad("without a LUT node", [[LUT_OUT, 0, -1, -1, -1, -1]])                                # misplaced
    bad("without a LUT node", [[LUT, 0, 1, -1, 1, 0], [LUT_OUT, 3, -1, -1, -1, -1], [LUT_OUT, 3, -1, -1, -1, -1]])
    bad("wrong head", [[LUT, 0, 1, -1, 1, 0], [LUT_OUT, 2, -1, -1, -1, -1]])
    bad("wrong head", [[NAND, 0, 1, -1, -1, -1], [LUT, 0, 1, -1, 1, 0], [LUT_OUT, 3, -1, -1, -1, -1]])
    bad("fields after the head", [[LUT, 0, 1, -1, 1, 0], [LUT_OUT, 3, -1, -1, 0, -1]])
    bad("spec and lut must be -1", [[NAND, 0, 1, -1, 0, -1]])
    bad("spec and lut must be -1", [[NOT, 0, -1, -1, -1, 1]])
    bad("topological", [[LUT, 3, -1, -1, 0, 0]])
    bad("topological", [[NAND, 0, 4, -1, -1, -1], [NAND, 0, 1, -1, -1, -1]])
    bad("opcode", [[16, 0, 1, -1, -1, -1]])
    bad("opcode", [[XNOR if mk else AND3, 0, 1, 2, -1, -1]])
    rc, msg = _call(L, mk, OK_ROWS)
    assert rc == -1 and "null ctx" in msg


def _enc_int(K, m, sigma, seed):
    from thfhe import lut
    return R.encrypt_words(K, lut.encode(np.asarray(m), 4), sigma, seed)


def test_cpu_yardstick_decrypts_a_lut_adder_and_a_conversion_chain(O, sk_small):
    # reduced keys (n = 16): the yardstick composes the oracle's gates and PBS pieces row by row
    from thfhe import circuits as Cc, lut
    p, K, orc = sk_small
    sigma = 2.0**-15
    rng = np.random.default_rng(3)
    # 3-bit LUT adder on integer bits
    c = Cc.Circuit()
    a, b = c.inputs(3), c.inputs(3)
    s, cy = Cc.lut_ripple_add(c, a, b)
    assert c.census()["rotations"] == 3
    for trial in range(2):
        A, B = (int(v) for v in rng.integers(0, 8, 2))
        x = np.concatenate([_enc_int(K, [(A >> i) & 1 for i in range(3)], sigma, 10 + trial), _enc_int(K, [(B >> i) & 1 for i in range(3)], sigma, 20 + trial)])
        v = DR.evaluate(orc, c, x)
        bits = lut.decode(K.phases(v[s + [cy]]), 4)
        assert sum(int(bt) << i for i, bt in enumerate(bits)) == A + B, (A, B, bits)
    # gate bits -> from_gate_bit -> 2-bit LUT adder -> carry -> to_gate_bit -> MUX between two gate-encoded words
    c = Cc.Circuit()
    ga, gb, wx, wy = (c.inputs(2) for _ in range(4))
    ia, ib = [Cc.from_gate_bit(c, w) for w in ga], [Cc.from_gate_bit(c, w) for w in gb]
    s, cy = Cc.lut_ripple_add(c, ia, ib)
    sel = Cc.to_gate_bit(c, cy)
    out = [c.gate(O.MUX, sel, wx[j], wy[j]) for j in range(2)]
    for A, B in ((3, 2), (1, 2)):
        X, Y = [1, 0], [0, 1]
        bits = [(A >> i) & 1 for i in range(2)] + [(B >> i) & 1 for i in range(2)] + X + Y
        v = DR.evaluate(orc, c, K.encrypt_bits(bits, sigma, 30 + A))
        carry = (A + B) >> 2
        assert list(lut.decode(K.phases(v[s]), 4)) == [((A + B) >> i) & 1 for i in range(2)]
        assert K.decrypt_bits(v[[sel]])[0] == bool(carry)
        assert list(K.decrypt_bits(v[out])) == [bool(t) for t in (X if carry else Y)]
