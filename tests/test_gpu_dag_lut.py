"""LUT nodes in the gate-DAG executor on the MI355X (pytest -m gpu): thfhe_dag_run_lut_batch / thfhe_mk_dag_run_lut_batch against the host-driven
level loop (evaluate_levels, lut_bootstrap per (theta, spec)) bit for bit on random mixed DAGs, against the composed oracle reference at full
size, instances against single runs with slices that straddle instances and theta records, a LUT level on every rotation shape, and
circuits that decrypt: a 16-bit LUT ripple adder and a gate -> LUT -> gate conversion chain."""
import numpy as np
import pytest

import dag_lut_reference as DR
import lut_reference as R
from support import SIGMA, words

pytestmark = pytest.mark.gpu


def _random_table(rng, N, torus_bits):
    if torus_bits == 64:
        return rng.integers(-2**63, 2**63 - 1, N, dtype=np.int64)
    return words(rng, N)


def random_mixed_dag(rng, n_in, n_rows, gate_ops, N=1024, torus_bits=32, n_tables=3):
    """Gates of every class in gate_ops and LUT nodes (theta 1 / 2 / 4, 1-3 inputs, random weights, bias and table) reading each other;
    NOT / COPY of LUT outputs."""
    import thfhe
    from thfhe import circuits as Cc
    c = Cc.Circuit()
    c.inputs(n_in)
    tids = [c.table(_random_table(rng, N, torus_bits)) for _ in range(n_tables)]
    while len(c.gates) < n_rows:
        w = c.n_wires()
        pick = lambda: int(rng.integers(0, w))
        if rng.random() < 0.35:
            nin = int(rng.integers(1, 4))
            outs = c.lut(int(rng.choice(tids)), [pick() for _ in range(nin)], weights=tuple(int(v) for v in rng.integers(-7, 8, nin)),
                         bias=int(rng.integers(-2**31, 2**31)), theta=int(rng.choice([1, 2, 4])))
            if rng.random() < 0.5:
                c.gate(int(rng.choice([thfhe.NOT, thfhe.COPY])), int(rng.choice(outs)))
        else:
            op = int(rng.choice(gate_ops))
            if op in (thfhe.NOT, thfhe.COPY):
                c.gate(op, pick())
            elif op in (thfhe.MUX, thfhe.AND3):
                c.gate(op, pick(), pick(), pick())
            else:
                c.gate(op, pick(), pick())
    return c


def _sk_small(n=64, seed=4):
    import thfhe
    from thfhe import keygen
    p = thfhe.make_params("SK-128", n=n)
    K = keygen.SecretKeySet(p, seed=seed)
    return p, K, thfhe.CloudKey(p, K.bk, K.ksk, device=0)


def _mk_small(O, n=64, seed=5):
    import thfhe
    pm = O.make_params("MK2", n=n)
    sg = O.SIGMAS["MK2"]
    KM = O.MKKeys(pm, seed, sg["bk"], sg["ks"])
    return pm, KM, thfhe.MKCloudKey(thfhe.make_params(**pm.as_dict()), KM.bk, KM.ksk, device=0)


SK_OPS = list(range(13))                  # NAND .. ORYN, MUX, NOT, COPY
MK_OPS = [0, 1, 2, 3, 13, 10, 11, 12]     # NAND, OR, AND, XOR, AND3, MUX, NOT, COPY


def test_random_mixed_dags_equal_the_level_loop(O):
    import thfhe
    from thfhe import circuits as Cc
    rng = np.random.default_rng(41)
    p, K, ck = _sk_small()
    mp, KM, mk = _mk_small(O)
    try:
        for key, ops, torus_bits, trials in ((ck, SK_OPS, 32, 3), (mk, MK_OPS, 64, 2)):
            for trial in range(trials):
                cir = random_mixed_dag(rng, 6, 90, ops, torus_bits=torus_bits)
                assert cir.has_luts()
                x = words(rng, 6, key.words)
                stats = {}
                got = Cc.evaluate(key, cir, x, stats)
                ref = Cc.evaluate_levels(key, cir, x)
                assert np.array_equal(got, ref), (torus_bits, trial)
                cen = cir.census()
                assert stats["levels"] == cen["depth"] and stats["rotations"] == cen["rotations"], (stats, cen)
    finally:
        ck.close()
        mk.close()


def _small_full_size_dag(rng, N, torus_bits):
    from thfhe import circuits as Cc
    c = Cc.Circuit()
    x = c.inputs(3)
    t = [c.table(_random_table(rng, N, torus_bits)) for _ in range(2)]
    l1 = c.lut(t[0], [x[0], x[1]], weights=(2, -3), bias=12345, theta=1)
    l2 = c.lut(t[1], [l1[0], x[2]], weights=(1, 5), bias=-777, theta=2)
    g = c.gate(0, l2[1], x[0])   # NAND of a LUT output
    l4 = c.lut(t[0], [g, l2[0], x[1]], weights=(1, 1, -1), bias=2**30, theta=4)
    return c, l1 + l2 + l4


def test_full_size_lut_nodes_equal_the_oracle(O, sk128):
    import thfhe
    from thfhe import circuits as Cc
    rng = np.random.default_rng(42)
    p, K, orc = sk128
    ck = thfhe.CloudKey(thfhe.make_params("SK-128"), K.bk, K.ksk, device=0)
    try:
        c, outs = _small_full_size_dag(rng, 1024, 32)
        x = words(rng, 3, p.n + 1)
        got = Cc.evaluate(ck, c, x)
        ref = DR.evaluate(orc, c, x)
        assert np.array_equal(got[outs], ref[outs])
    finally:
        ck.close()
    mp = O.make_params("MK2")
    sg = O.SIGMAS["MK2"]
    KM = O.MKKeys(mp, 0x5EED0003, sg["bk"], sg["ks"])
    mk = thfhe.MKCloudKey(thfhe.make_params(**mp.as_dict()), KM.bk, KM.ksk, device=0)
    try:
        c, outs = _small_full_size_dag(rng, mp.N, 64)
        x = words(rng, 3, mk.words)
        got = Cc.evaluate(mk, c, x)
        ref = DR.evaluate(O.MKOracle(mp, KM.bk, KM.ksk), c, x, multi_key=True)
        assert np.array_equal(got[outs], ref[outs])
    finally:
        mk.close()


def test_instances_equal_single_runs_with_slices(O):
    import thfhe
    from thfhe import circuits as Cc
    rng = np.random.default_rng(43)
    p, K, ck = _sk_small()
    mp, KM, mk = _mk_small(O)
    try:
        for key, ops, torus_bits in ((ck, SK_OPS, 32), (mk, MK_OPS, 64)):
            cir = random_mixed_dag(rng, 5, 60, ops, torus_bits=torus_bits)
            Q = 6
            x = words(rng, Q, 5, key.words)
            single = np.stack([Cc.evaluate(key, cir, x[q]) for q in range(Q)])
            lut_outs = [cir.n_inputs + g for g, row in enumerate(cir.gates) if row[0] == thfhe.LUT_OUT]
            assert lut_outs
            sel = lut_outs[::2] + [cir.n_wires() - 1, 0]
            for slice_ in (1, 5, 7, 28672 if key is ck else 8192):
                key.set_dag_slice(slice_)
                assert np.array_equal(Cc.evaluate_batch(key, cir, x), single), (torus_bits, slice_)
                assert np.array_equal(Cc.evaluate_batch(key, cir, x, sel), single[:, sel]), (torus_bits, slice_)
    finally:
        ck.close()
        mk.close()


def test_lut_level_on_every_rotation_shape():
    # one launch group of 2 048 + 1 100 nodes: an eight-wave round, a four-wave remainder of 1 024 and a cooperative remainder of 76
    from thfhe import circuits as Cc
    rng = np.random.default_rng(44)
    p, K, ck = _sk_small()
    try:
        c = Cc.Circuit()
        x = c.inputs(2)
        t = [c.table(_random_table(rng, 1024, 32)) for _ in range(3)]
        a = c.lut(t[1], [x[0], x[1]], weights=(3, -1), bias=99, theta=1)
        b = c.lut(t[2], [x[1]], weights=(5,), bias=-4, theta=4)
        Q = 2048 + 1100
        xs = words(rng, Q, 2, ck.words)
        st = {}
        got = Cc.evaluate_batch(ck, c, xs, a + b, st)
        assert st["launches"] == 2 and st["levels"] == 1 and st["rotations"] == 2 * Q
        tvs = np.stack(c.tables)
        ra = ck.lut_bootstrap(tvs, xs[:, 0], xs[:, 1], weights=(3, -1), bias=99, theta=1, lut_index=np.full(Q, t[1]))
        rb = ck.lut_bootstrap(tvs, xs[:, 1], weights=(5,), bias=-4, theta=4, lut_index=np.full(Q, t[2]))
        assert np.array_equal(got[:, 0], ra[:, 0])
        assert np.array_equal(got[:, 1:], rb)
    finally:
        ck.close()


def _enc_int(K, m, seed):
    from thfhe import lut
    return R.encrypt_words(K, lut.encode(np.asarray(m), 4), SIGMA, seed)


def test_lut_ripple_adder_16_bit(sk128):
    import thfhe
    from thfhe import circuits as Cc, lut
    p, K, orc = sk128
    rng = np.random.default_rng(45)
    ck = thfhe.CloudKey(thfhe.make_params("SK-128"), K.bk, K.ksk, device=0)
    try:
        c = Cc.Circuit()
        a, b = c.inputs(16), c.inputs(16)
        s, cy = Cc.lut_ripple_add(c, a, b)
        Q = 64
        A, B = rng.integers(0, 1 << 16, Q), rng.integers(0, 1 << 16, Q)
        bits = lambda V: np.array([[(int(v) >> i) & 1 for i in range(16)] for v in V])
        enc = _enc_int(K, np.concatenate([bits(A), bits(B)], axis=1).reshape(-1), 900).reshape(Q, 32, -1)
        st = {}
        out = Cc.evaluate_batch(ck, c, enc, s + [cy], st)
        dec = lut.decode(K.phases(out.reshape(-1, p.n + 1)), 4).reshape(Q, 17)
        assert np.all(dec <= 1)
        total = (dec.astype(np.int64) << np.arange(17)).sum(axis=1)
        assert np.array_equal(total, A + B)
        assert st["rotations"] == 16 * Q and st["levels"] == 16
        g = Cc.Circuit()
        ga, gb, z = g.inputs(16), g.inputs(16), g.inputs(1)[0]
        Cc.full_adder(g, ga, gb, z)
        assert g.census()["rotations"] == 79
    finally:
        ck.close()


def _conversion_chain(N, torus_bits):
    from thfhe import circuits as Cc
    c = Cc.Circuit()
    ga, gb, wx, wy = (c.inputs(4) for _ in range(4))
    kw = dict(N=N, torus_bits=torus_bits)
    ia, ib = [Cc.from_gate_bit(c, w, **kw) for w in ga], [Cc.from_gate_bit(c, w, **kw) for w in gb]
    s, cy = Cc.lut_ripple_add(c, ia, ib, **kw)
    sel = Cc.to_gate_bit(c, cy, **kw)
    out = [c.gate(10, sel, wx[j], wy[j]) for j in range(4)]
    return c, s, sel, out


def _check_chain(key, K, enc_bits, decrypt_bits, phases, N, torus_bits, rng, max_error_frac=0.0):
    """max_error_frac: the share of decrypted bits allowed to be wrong.  0 on SK-128.  On MK2 every adder input is a key-switched p = 4 bit at
    about 2.7 sigma, summed two or three at a time: single errors are expected there, a wiring or executor fault is not (it
    breaks about half of the bits)."""
    from thfhe import circuits as Cc, lut
    c, s, sel, out = _conversion_chain(N, torus_bits)
    Q = 16
    A, B = rng.integers(0, 16, Q), rng.integers(0, 16, Q)
    X, Y = rng.integers(0, 2, (Q, 4)), rng.integers(0, 2, (Q, 4))
    bits = np.concatenate([[(A >> i) & 1 for i in range(4)], [(B >> i) & 1 for i in range(4)], X.T, Y.T]).T   # [Q][16]
    enc = enc_bits(bits.reshape(-1)).reshape(Q, 16, -1)
    got = Cc.evaluate_batch(key, c, enc, s + [sel] + out)
    carry = (A + B) >> 4
    dec_s = lut.decode(phases(got[:, :4].reshape(-1, key.words)), 4).reshape(Q, 4)
    dec_sel = decrypt_bits(got[:, 4])
    dec_out = decrypt_bits(got[:, 5:].reshape(-1, key.words)).reshape(Q, 4)
    wrong = [np.mean(dec_s != np.stack([((A + B) >> i) & 1 for i in range(4)], axis=1)), np.mean(dec_sel != carry.astype(bool)),
             np.mean(dec_out != np.where(dec_sel[:, None], X, Y).astype(bool))]   # the MUX judged on the select it received
    assert max(wrong) <= max_error_frac, wrong


def test_gate_lut_gate_conversion_chain_decrypts(O, sk128):
    import thfhe
    p, K, orc = sk128
    rng = np.random.default_rng(46)
    ck = thfhe.CloudKey(thfhe.make_params("SK-128"), K.bk, K.ksk, device=0)
    try:
        _check_chain(ck, K, lambda b: K.encrypt_bits(b, SIGMA, 950), K.decrypt_bits, K.phases, 1024, 32, rng)
    finally:
        ck.close()
    mp = O.make_params("MK2")
    sg = O.SIGMAS["MK2"]
    KM = O.MKKeys(mp, 0x5EED0004, sg["bk"], sg["ks"])
    mk = thfhe.MKCloudKey(thfhe.make_params(**mp.as_dict()), KM.bk, KM.ksk, device=0)
    try:
        _check_chain(mk, KM, lambda b: KM.encrypt_bits(b, sg["lwe"], 951), KM.decrypt_bits, KM.phases, mp.N, 64, rng, max_error_frac=0.2)
    finally:
        mk.close()


def test_old_entry_points_reject_lut_opcodes(O):
    import thfhe
    p, K, ck = _sk_small()
    mp, KM, mk = _mk_small(O)
    try:
        for key in (ck, mk):
            x = np.zeros((1, 2, key.words), np.int32)
            for op in (thfhe.LUT, thfhe.LUT_OUT):
                with pytest.raises(thfhe.ThfheError, match="opcode"):
                    key.dag_run_batch(x, np.array([[op, 0, 1, -1]], np.int32))
    finally:
        ck.close()
        mk.close()
