"""Layered automata on TGSW-encrypted bits without a GPU: the entry points exist in the built library and every host
check answers in the documented order before a set or a context is looked at; the builders of thfhe.circuits agree with plain integer
arithmetic; the model of wfa_reference.py on noiseless TGSW samples equals the plain run word for word; and the real-key cases of
tests/test_gpu_wfa.py decrypt on the model, with the noise inside the band the GPU test asserts."""
import ctypes as C

import numpy as np
import pytest

import lhe_reference as LR
import wfa_cases
import wfa_reference as WR

N = 1024


def _err(L):
    return L.thfhe_last_error().decode()


def test_symbols_exist_and_every_host_check_answers_in_order():
    import thfhe
    L = thfhe.lib()
    for name in ("thfhe_lhe_wfa", "thfhe_lhe_wfa_wo_keyswitch", "thfhe_set_wfa_chunk"):
        assert hasattr(L, name), name
    i32 = lambda v: np.ascontiguousarray(v, np.int32)
    p = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))
    INV = -1
    for g in (-1, 65):
        assert L.thfhe_set_wfa_chunk(None, g) == INV and "wfa chunk" in _err(L)
    assert L.thfhe_set_wfa_chunk(None, 0) == INV and "wfa chunk" in _err(L)      # a null context
    vp = C.c_void_p
    null_sets = (vp * 64)()
    buf = np.zeros((3, 2, N), np.int32)
    for fn in (L.thfhe_lhe_wfa, L.thfhe_lhe_wfa_wo_keyswitch):
        def call(sets=null_sets, n_sets=1, count=2, n_steps=1, n_states=2, trans=None, step_bit=None, fin_b=buf, n_tables=1, index=None, theta=1,
                 start=None, n_out=1, out=buf, keep=[]):
            trans = i32(np.zeros((max(n_steps, 1), max(n_states, 1), 2))) if trans is None else trans
            step_bit = i32(np.zeros(max(n_steps, 1))) if step_bit is None else step_bit
            start = i32(np.zeros(max(n_out, 1))) if start is None else start
            none = lambda a: None if isinstance(a, str) else a
            return fn(None, none(sets), n_sets, 0, count, n_steps, n_states, p(none(trans)), p(none(step_bit)), None, p(none(fin_b)), n_tables, p(index),
                      theta, p(none(start)), n_out, p(none(out)))
        # null pointers
        for hole in ("sets", "trans", "step_bit", "fin_b", "start", "out"):
            assert call(**{hole: "null"}) == INV and "null argument" in _err(L), hole
        # the limits, in the order of the argument list
        for v in (0, 65):
            assert call(n_sets=v) == INV and "n_sets must be 1 .. 64" in _err(L)
        for v in (0, 4097):
            assert call(n_steps=v) == INV and "n_steps must be 1 .. 4096" in _err(L)
        for v in (0, 65):
            assert call(n_states=v) == INV and "n_states must be 1 .. 64" in _err(L)
        for v in (0, 65):
            assert call(n_out=v) == INV and "n_out must be 1 .. 64" in _err(L)
        for v in (0, 3, 8):
            assert call(theta=v) == INV and "theta must be 1, 2 or 4" in _err(L)
        assert call(n_tables=0) == INV and "n_tables n_states" in _err(L)
        assert call(n_states=64, n_tables=4097) == INV and "n_tables n_states" in _err(L)
        # a limit answers before the entries are read: n_states = 0 with a bad table
        assert call(n_states=0, trans=i32([[[7, 7]]])) == INV and "n_states" in _err(L)
        # entries: trans, then start, then table_index
        for bad in (-1, 2):
            assert call(trans=i32([[[0, 1], [bad, 0]]]), start=i32([5])) == INV and "trans entry out of range" in _err(L)
            assert call(start=i32([bad]), index=i32([0, 9])) == INV and "start entry out of range" in _err(L)
        assert call(n_tables=3, index=i32([0, 3])) == INV and "table_index out of range" in _err(L)
        # ... and only then the sets
        assert call(step_bit=i32([99])) == INV and "null tgsw set" in _err(L)
        assert call(n_sets=64) == INV and "null tgsw set" in _err(L)
        assert call(count=0) == INV and "null tgsw set" in _err(L)


@pytest.mark.parametrize("width", [1, 2, 3, 4])
def test_comparison_builders_exhaustively(width):
    from thfhe import circuits
    a, b = (v.reshape(-1) for v in np.meshgrid(np.arange(1 << width), np.arange(1 << width)))
    bits = circuits.wfa_pair_bits(a, b, width)
    assert len(bits) == 2 and bits[0].shape == (a.shape[0], width)
    lt, eq = circuits.wfa_less_than(width), circuits.wfa_equal(width)
    assert lt[0].shape == (2 * width, 4, 2) and lt[1].shape == (2 * width,)
    assert np.array_equal(circuits.wfa_run_plain(lt, bits)[:, 0, 0], a < b)
    assert np.array_equal(circuits.wfa_run_plain(eq, bits)[:, 0, 0], a == b)


def test_comparison_builders_on_random_32_bit_pairs():
    from thfhe import circuits
    rng = np.random.default_rng(32)
    a, b = rng.integers(0, 1 << 32, 500), rng.integers(0, 1 << 32, 500)
    b[:100] = a[:100]
    b[100:150] = a[100:150] ^ (1 << 31)
    b[150:200] = a[150:200] ^ 1
    bits = circuits.wfa_pair_bits(a, b, 32)
    assert [v.shape for v in bits] == [(500, 16)] * 4                  # two numbers in four sets
    lt, eq = circuits.wfa_less_than(32), circuits.wfa_equal(32)
    assert set((lt[1] >> 4).tolist()) == {0, 1, 2, 3} and (lt[1] & 15).max() == 15
    assert np.array_equal(circuits.wfa_run_plain(lt, bits)[:, 0, 0], a < b)
    assert np.array_equal(circuits.wfa_run_plain(eq, bits)[:, 0, 0], a == b)
    k = circuits.wfa_noise_steps(lt, bits)
    assert k.shape == (500, 1) and k.min() >= 32 and k.max() <= 64      # every even step is a CMux, an odd step where a_i == b_i is a copy


def test_match_builder_against_a_string_search():
    from thfhe import circuits
    rng = np.random.default_rng(7)
    for pat in ([1], [1, 0, 1, 1], [0, 0, 1, 0, 0, 1, 0], [1, 1, 1, 1, 1]):
        text = rng.integers(0, 2, (400, 37))
        aut = circuits.wfa_match(pat, 37)
        assert aut[0].shape == (37, len(pat) + 1, 2) and len(circuits.wfa_text_bits(text)) == 3
        want = ["".join(map(str, pat)) in "".join(map(str, r)) for r in text]
        assert np.array_equal(circuits.wfa_run_plain(aut, circuits.wfa_text_bits(text))[:, 0, 0], want)
    pat = rng.integers(0, 2, 20)
    text = rng.integers(0, 2, (6, 20))
    text[2] = pat
    assert np.array_equal(circuits.wfa_run_plain(circuits.wfa_match(pat), circuits.wfa_text_bits(text))[:, 0, 0], [0, 0, 1, 0, 0, 0])
    with pytest.raises(ValueError):
        circuits.wfa_match([1] * 64)
    with pytest.raises(ValueError):
        circuits.wfa_match([1, 0, 1], 2)


def test_finals_layout():
    from thfhe import lut
    f = lut.wfa_finals([[1, 0, 3], [2, 2, 0]], 2, encode=lambda v: lut.encode(v, 4))
    assert f.shape == (3, N) and not f[:, 2:].any()
    assert np.array_equal(f[:, 0], lut.encode([1, 0, 3], 4)) and np.array_equal(f[:, 1], lut.encode([2, 2, 0], 4))
    assert np.array_equal(lut.wfa_finals([5, 6], 1)[:, 0], [5, 6])
    with pytest.raises(ValueError):
        lut.wfa_finals([[1, 2]], 2)
    with pytest.raises(ValueError):
        lut.wfa_finals([1, 2], 3)


def test_model_on_noiseless_samples_equals_the_plain_run(O):
    from thfhe import circuits, lut
    p = O.make_params("SK-128", n=16)
    rng = np.random.default_rng(12)
    a, b = rng.integers(0, 1 << 20, 6), rng.integers(0, 1 << 20, 6)
    b[0], b[1] = a[0], a[1] ^ 1
    bits = circuits.wfa_pair_bits(a, b, 20)                            # four sets: 16 + 4 bits per number
    sets = [np.stack([LR.trivial_tgsw(p, row) for row in s]) for s in bits]
    unit = 1 << (32 - p.l * p.Bgbit)                                  # words the decomposition represents exactly
    for aut in (circuits.wfa_less_than(20), circuits.wfa_equal(20)):
        trans, step_bit, fin, start = aut
        words = rng.integers(1, 1 << (p.l * p.Bgbit), (2, 4)) * unit  # a word per state and function, not 0 / 1
        fin_b = lut.wfa_finals(words, 2)
        state = [int(np.flatnonzero(fin[0] == v)[0]) for v in circuits.wfa_run_plain(aut, bits)[:, 0, 0]]   # 0 and 1 name one reachable state each
        for s in range(6):
            u = WR.wfa_wo_keyswitch(p, [C[s] for C in sets], trans, step_bit, None, fin_b, 2, start)
            assert u.shape == (1, 2, N + 1) and not u[:, :, :N].any()
            assert np.array_equal(u[0, :, N], lut._to_i32(words[:, state[s]])), s


@pytest.mark.parametrize("which", ["less_than", "equal"])
def test_model_decrypts_the_real_key_cases(O, which):
    from thfhe import lut
    S, c = wfa_cases.keys(O), wfa_cases.case(O, which)
    want = c["want"]
    assert want.shape == (8, 1, 2) and 0 < want[:, 0, 0].sum() < 8
    assert np.array_equal(lut.decode(S.K.ring_phase(c["wo"]).reshape(want.shape), wfa_cases.P_OUT), want)
    assert np.array_equal(lut.decode(S.K.phase(c["ks"]).reshape(want.shape), wfa_cases.P_OUT), want)


def test_model_noise_of_the_real_key_cases_is_inside_the_band(O):
    S = wfa_cases.keys(O)
    cases = [wfa_cases.case(O, w) for w in ("less_than", "equal")]
    std = wfa_cases.noise(S, np.concatenate([c["wo"] for c in cases]), np.concatenate([c["want"] for c in cases]))
    pred = wfa_cases.predicted(S, cases)
    print(f"\nwfa noise SK-128 (CPU model): std {std:.3e} over 32 outputs, predicted {pred:.3e}, ratio {std / pred:.2f}")
    assert 0.5 * pred <= std <= 2 * pred
