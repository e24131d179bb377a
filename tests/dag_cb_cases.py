"""The cases of the circuit-bootstrap nodes of the gate DAG, shared by tests/test_gpu_dag_cb.py and the model-only test of
tests/test_dag_cb_host.py -- TEST INFRASTRUCTURE ONLY.  The keys are cb_cases.keys': SK-128 / SK-80 with n reduced to 16, the level-2 context at its
full ring degree 2048, the private key at (t, basebit) = (7, 4) and sigma_pks = 2^-31; a packing key is made as dag_lhe_cases.Keys makes one.
Every case is evaluated AND DECODED by the model when it is built, on fixed seeds, so the device is only ever asked for cases the model decodes."""
import numpy as np

import cb_cases as CC
import dag_cb_reference as DCB
from support import N, pmap

NAND, OR, AND, XOR = 0, 1, 2, 3
GATE = lambda v: np.where(np.asarray(v) > 0, 1 << 29, -(1 << 29))   # integers 0 / 1 -> the gate encoding +-1/8
_made = {}


def keys(O, name, device=None):
    """cb_cases.keys(name) with a packing key `pk` at the ring's noise"""
    S = CC.keys(O, name, device)
    if not hasattr(S, "pk"):
        from thfhe import keygen
        S.pk = keygen.gen_pack_key(np.random.default_rng(0x7EE0C00 + S.tp.l), S.K.lwe_key, S.K.rlwe_key, S.p.ks_t, S.p.ks_basebit, S.sig["bk"])
    return S


def model(S, cir, x, one_rotation=False, sets=(), only=None):
    """(wires int32[instances][n_wires][words], [per computed set int32[instances][d][2l][2][N]]) of the model"""
    res = pmap(lambda q: DCB.evaluate(S, cir, x[q], [C[q] for C in sets], CC.T, CC.BASEBIT, one_rotation, S.pk, only), range(x.shape[0]))
    rows = [np.stack([r[1][c] for r in res]) for c in range(len(cir.cb_specs))] if only is None else None
    return np.stack([r[0] for r in res]), rows


def encrypt(S, bits, seed):
    """int32[instances][n_inputs][n+1]: fresh gate-encoded encryptions of bits int[instances][n_inputs]"""
    return np.stack([S.K.encrypt(b, seed=seed + q) for q, b in enumerate(np.asarray(bits))])


def lookup(O, name="SK-128", one_rotation=False, d=3, d_tree=1, count=8, device=None):
    """cb_lookup_dag: d XOR gates -> CB -> LOOKUP at (d_tree, d - d_tree) in a table of gate bits -> NAND with one more input; the XORs take every
    address once (count = 2^d).  dict(S, cir, x, a, b, k, table, out, nand, ref, rows)."""
    key = ("lookup", name, one_rotation, d, d_tree, count)
    if key not in _made:
        from thfhe import circuits as CI
        S = keys(O, name, device)
        rng = np.random.default_rng(0xDCB100 + d)
        a = rng.integers(0, 1 << d, count)
        b = a ^ (rng.permutation(1 << d)[np.arange(count) % (1 << d)])
        k = rng.integers(0, 2, count)
        table = rng.integers(0, 2, 1 << d)
        table[:2] = (0, 1)
        cir = CI.Circuit()
        wa, wb, wk = cir.inputs(d), cir.inputs(d), cir.inputs(1)
        out = CI.cb_lookup_dag(cir, wa, wb, table, d_tree=d_tree, encode=GATE)
        nand = cir.gate(NAND, out, wk[0])
        bits = np.concatenate([(a[:, None] >> np.arange(d)) & 1, (b[:, None] >> np.arange(d)) & 1, k[:, None]], axis=1)
        x = encrypt(S, bits, 0xDCB200)
        ref, rows = model(S, cir, x, one_rotation)
        want = CI.cb_lookup_plain(a, b, table)
        assert sorted((a ^ b).tolist()) == sorted(np.arange(count) % (1 << d)), "every address"
        assert np.array_equal(S.K.decrypt(ref[:, out]), want.astype(bool)), "the model itself must decode every lookup"
        assert np.array_equal(S.K.decrypt(ref[:, nand]), ~(want.astype(bool) & k.astype(bool))), "... and the NAND on it"
        _made[key] = dict(S=S, cir=cir, x=x, bits=bits, a=a, b=b, k=k, table=table, out=out, nand=nand, want=want, ref=ref, rows=rows)
    return _made[key]


def array_read(O, name="SK-128", count=8, device=None):
    """cb_array_read of 8 computed wires at (1, 2) at a computed 3-bit index whose wires are not consecutive and one of which is an INPUT wire.
    dict(S, cir, x, g (the candidates), index (the wires), out, addr, want, ref, rows)."""
    key = ("array_read", name, count)
    if key not in _made:
        from thfhe import circuits as CI
        S = keys(O, name, device)
        rng = np.random.default_rng(0xDCB300)
        cir = CI.Circuit()
        x = cir.inputs(8)
        i1 = cir.gate(XOR, x[1], x[2])
        g = [cir.gate((NAND, XOR, AND, OR)[i % 4], x[i % 8], x[(3 * i + 1) % 8]) for i in range(8)]
        i2 = cir.gate(XOR, x[3], x[4])
        index = [x[0], i1, i2]                      # bit 0 is an input wire: the CB node's own wire is a copy of it
        out = CI.cb_array_read(cir, g, index, 1, 2)
        bits = rng.integers(0, 2, (count, 8))
        bits[:, 0] = np.arange(count) & 1           # the index takes every value when count = 8
        bits[:, 1] = ((np.arange(count) >> 1) & 1) ^ bits[:, 2]
        bits[:, 3] = ((np.arange(count) >> 2) & 1) ^ bits[:, 4]
        recs = encrypt(S, bits, 0xDCB400)
        ref, rows = model(S, cir, recs)
        plain = np.stack([CI.simulate(cir, GATE(bits[q])) > 0 for q in range(count)])
        addr = np.arange(count) % 8
        want = plain[np.arange(count), np.array(g)[addr]]
        assert np.array_equal(plain[:, index].astype(int) @ (1 << np.arange(3)), addr)
        assert np.array_equal(S.K.decrypt(ref[:, out]), want), "the model itself must decode every read"
        _made[key] = dict(S=S, cir=cir, x=recs, bits=bits, g=g, index=index, out=out, addr=addr, want=want, ref=ref, rows=rows)
    return _made[key]


def mux_max(O, name="SK-128", count=4, width=3, device=None):
    """cb_mux_max at `width` bits on `count` pairs held as gate bits only (MSB first): ONE computed set of d = 2 width.  Pair 0 is equal.
    dict(S, cir, x, out, A, B, ref, rows)."""
    key = ("mux_max", name, count, width)
    if key not in _made:
        from thfhe import circuits as CI
        S = keys(O, name, device)
        rng = np.random.default_rng(0xDCB500)
        A, B = rng.integers(0, 1 << width, count), rng.integers(0, 1 << width, count)
        A[0] = B[0]                                   # an equal pair: a < b is false
        cir = CI.Circuit()
        a, b = cir.inputs(width), cir.inputs(width)
        out = CI.cb_mux_max(cir, a, b, width)
        msb = lambda v: [(int(v) >> (width - 1 - i)) & 1 for i in range(width)]
        recs = encrypt(S, [msb(A[q]) + msb(B[q]) for q in range(count)], 0xDCB600)
        ref, rows = model(S, cir, recs)
        val = (S.K.decrypt(ref[:, out]).reshape(count, width) << np.arange(width - 1, -1, -1)).sum(axis=1)
        assert np.array_equal(val, np.maximum(A, B)), "the model itself must decode every maximum"
        _made[key] = dict(S=S, cir=cir, x=recs, out=out, A=A, B=B, ref=ref, rows=rows)
    return _made[key]


def three_sets(O, name="SK-128", count=7, device=None):
    """Two CB nodes on one level (d = 2 on two XOR outputs, d = 3 on three NAND outputs) and a third (d = 2) one level later on gates that read a
    LOOKUP on the first set; a LOOKUP on each set.  dict(S, cir, x, sets (the ids), outs (the three lookups' wires), tables, ref, rows)."""
    key = ("three_sets", name, count)
    if key not in _made:
        from thfhe import circuits as CI, lut
        S = keys(O, name, device)
        rng = np.random.default_rng(0xDCB700)
        cir = CI.Circuit()
        x = cir.inputs(6)
        xo = [cir.gate(XOR, x[0], x[1]), cir.gate(XOR, x[2], x[3])]
        na = [cir.gate(NAND, x[i], x[i + 3]) for i in range(3)]
        s0, s1 = cir.cb_set(xo), cir.cb_set(na)
        tables = [rng.integers(0, 2, 4), rng.integers(0, 2, 8), rng.integers(0, 2, 4)]
        row = lambda tb, d_tree, d_rot: cir.lhe_table(lut.lhe_table(tb, d_tree, d_rot, encode=GATE))
        o0 = cir.lhe_lookup(s0, row(tables[0], 0, 2), 0, 2)[0]
        o1 = cir.lhe_lookup(s1, row(tables[1], 1, 2), 1, 2)[0]
        later = [cir.gate(AND, o0, x[4]), cir.gate(OR, o1, x[5])]
        s2 = cir.cb_set(later)
        o2 = cir.lhe_lookup(s2, row(tables[2], 1, 1), 1, 1)[0]
        bits = rng.integers(0, 2, (count, 6))
        recs = encrypt(S, bits, 0xDCB800)
        ref, rows = model(S, cir, recs)
        plain = np.stack([CI.simulate(cir, GATE(bits[q])) > 0 for q in range(count)])
        assert np.array_equal(S.K.decrypt(ref[:, [o0, o1, o2]]).reshape(count, 3), plain[:, [o0, o1, o2]]), "the model itself must decode every lookup"
        _made[key] = dict(S=S, cir=cir, x=recs, bits=bits, sets=[s0, s1, s2], outs=[o0, o1, o2], tables=tables, ref=ref, rows=rows, plain=plain)
    return _made[key]


SLICE_INSTANCES = CC.SLICE_BITS // 3 + 1       # 683 instances of d = 3: 2 049 bits, slices of 682 + 1 instances
SLICE_READ = [0, SLICE_INSTANCES - 3, SLICE_INSTANCES - 2, SLICE_INSTANCES - 1]


def slice_boundary(O, one_rotation=False, device=None):
    """One CB node, d = 3, on INPUT wires: a cb_cases.drawn batch of 683 instances from the lookup bits of cb_cases.case (a fixed seed), so that
    the rows are case rows [idx] (per-level mode; cb_one_reference.models' in one-rotation mode); a LOOKUP at (1, 2) in cb_cases' table, whose model
    is computed for the instances SLICE_READ.  dict(S, cir, x, idx, rows, out, ref (the model's lookup records of SLICE_READ), want)."""
    key = ("slice", one_rotation)
    if key not in _made:
        import lhe_reference as LR
        from thfhe import circuits as CI, lut
        S = keys(O, "SK-128", device)
        c = CC.case(O, "SK-128", device)
        recs, idx = CC.drawn(c, 3 * SLICE_INSTANCES, 0xDCB900, pool=24)
        l = S.tp.l
        if one_rotation:
            pool_rows = DCB.cb_rows(S, c["recs"][:24], CC.T, CC.BASEBIT, True)
        else:
            pool_rows = c["rows"][:24]
        rows = pool_rows[idx]
        cir = CI.Circuit()
        x = cir.inputs(3)
        tset = cir.cb_set(x)
        out = cir.lhe_lookup(tset, cir.lhe_table(c["tab"]), 1, 2)[0]
        Cs = rows.reshape(SLICE_INSTANCES, 3, 2 * l, 2, N)
        ref = np.stack(pmap(lambda s: LR.lookup(S.orc, Cs[s], None, c["tab"], 1, 2, 1)[0], SLICE_READ))
        addr = (c["bits"][:24][idx].reshape(-1, 3) << np.arange(3)).sum(axis=1)
        want = c["table"][addr[SLICE_READ]]
        assert np.array_equal(lut.decode(S.K.phase(ref), CC.P_OUT), want), "the model itself must decode every lookup"
        _made[key] = dict(S=S, cir=cir, x=recs.reshape(SLICE_INSTANCES, 3, -1), idx=idx, rows=rows, out=out, ref=ref, want=want)
    return _made[key]


TWO_LEVEL_INSTANCES = CC.SLICE_BITS // 2     # 1 024 instances: the d = 2 group's slice holds 2 048 bits, the d = 3 group's 682 x 3 = 2 046


def two_levels(O, device=None):
    """Two CB levels of different width at 1 024 instances: d = 3 on input wires on level 1, d = 2 on two NAND(x, x) outputs on level 2.  A slice
    is min(instances, 2 048 / sum d) instances, so the NARROWER group holds more bits per slice (2 048) than the wider one (2 046): the workspace
    must be sized by the largest slice of any group, not by the widest group.  The inputs are a cb_cases.drawn batch from the 24 lookup records of
    cb_cases.case, so every stage's model is a gather: set 0's rows are case rows [idx], a NAND output is one of 24 oracle gates, and set 1's rows
    are the model's rows of those 24.  dict(S, cir, x, rows (per set), nand (the model's NAND wires), wires (the two gate wires))."""
    key = ("two_levels",)
    if key not in _made:
        from thfhe import circuits as CI
        S = keys(O, "SK-128", device)
        c = CC.case(O, "SK-128", device)
        Q = TWO_LEVEL_INSTANCES
        recs, idx = CC.drawn(c, 5 * Q, 0xDCBA00, pool=24)
        idx = idx.reshape(Q, 5)
        cir = CI.Circuit()
        x = cir.inputs(5)
        na = [cir.gate(NAND, x[3], x[3]), cir.gate(NAND, x[4], x[4])]
        cir.cb_set(x[:3])
        cir.cb_set(na)
        pool = c["recs"][:24]
        nand_pool = S.orc.gates(O.NAND, pool, pool)
        assert np.array_equal(S.K.decrypt(nand_pool), ~c["bits"][:24].astype(bool)), "the model itself must decode every NAND"
        nand_rows = DCB.cb_rows(S, nand_pool, CC.T, CC.BASEBIT, False)
        assert 0.5 <= CC.row_noise(S, nand_rows, ~c["bits"][:24].astype(bool)) / S.sigma_row() <= 2, "... and its rows are TGSW samples of the bits"
        l = S.tp.l
        rows = [c["rows"][:24][idx[:, :3].reshape(-1)].reshape(Q, 3, 2 * l, 2, N), nand_rows[idx[:, 3:].reshape(-1)].reshape(Q, 2, 2 * l, 2, N)]
        _made[key] = dict(S=S, cir=cir, x=recs.reshape(Q, 5, -1), rows=rows, nand=nand_pool[idx[:, 3:]], wires=na, ref=rows[0])
    return _made[key]


ALL = [("lookup, per level", lambda O: lookup(O)), ("lookup, one rotation", lambda O: lookup(O, one_rotation=True)),
       ("lookup, SK-80 at d = 1", lambda O: lookup(O, "SK-80", d=1, d_tree=0, count=2)), ("array read", array_read), ("mux max", mux_max),
       ("three sets", three_sets), ("slice boundary, per level", lambda O: slice_boundary(O)),
       ("slice boundary, one rotation", lambda O: slice_boundary(O, True)), ("two levels of different width", two_levels)]
