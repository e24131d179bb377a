"""CPU checks of tests/decomp_edges.py: the target words decompose as their labels say (the oracle's decomposition against the definition in
Python integers), and the tables the GPU sweeps run (test_gpu_cmux_amounts.py, test_gpu_mk_cmux_amounts.py) put a coefficient of X^a t - t on every
target word at EVERY amount, in the mask and in the body, with a negated rotated 0 and 2^(bits-1) -- asserted here, coefficient by coefficient."""
import numpy as np
import pytest

import bound_inputs as B
import decomp_edges as D

SK_GADGETS = [(1, 8), (2, 10), (3, 7), (4, 8)]
MK_SETS = ["MK2", "MK4-N2048", "MK256", "MK64-fft"]
SHAPES = [("sk-l%d-Bg%d" % g, 32, 1024) + g for g in SK_GADGETS]


def shapes(O):
    return SHAPES + [(name, 64, O.PARAM_SETS[name]["N"], O.PARAM_SETS[name]["l"], O.PARAM_SETS[name]["Bgbit"]) for name in MK_SETS]


IDS = [s[0] for s in SHAPES] + MK_SETS


def test_target_words_decompose_as_labelled(O):
    for name, bits, N, l, Bgbit in shapes(O):
        targets = D.edge_targets(bits, l, Bgbit)
        words = D.edge_words(bits, l, Bgbit)
        assert len(set(words.tolist())) == len(words) == len(targets) >= 8
        labelled = D.edge_targets(bits, l, Bgbit, unique=False)     # every label, the words that two labels share twice
        assert set(labelled.values()) == set(targets.values())
        digits = B.decompose(D.to_words(labelled.values(), bits), bits, l, Bgbit)      # the oracle's: int64[l][labels]
        for k, (label, d) in enumerate(labelled.items()):
            assert digits[:, k].tolist() == D.expected_digits(d, bits, l, Bgbit), (name, label)
        at = {label: digits[:, k].tolist() for k, label in enumerate(labelled)}
        half = 1 << (Bgbit - 1)
        assert at["every field 0"] == [-half] * l and at["d + offset all ones"] == [half - 1] * l
        # d + offset = 1: the sum wrapped, every field is 0 again (but for the 1 itself where no bit is dropped)
        assert at["d + offset wraps"] == [-half] * (l - 1) + [-half + (l * Bgbit == bits)]
        assert at["0"] == [0] * l and at["sign bit"] == [-half] + [0] * (l - 1)
        if l * Bgbit < bits:
            assert at["dropped bits all set"] == [0] * l and at["last kept bit"] == [0] * (l - 1) + [1]
        for p in range(1, l + 1):                                   # field p holds Bg/2 + Bg/2: it reads -Bg/2 and carries one into field p - 1
            assert at["level %d overflows" % p] == [0] * (p - 2) + [1] * (p > 1) + [-half] + [0] * (l - p), (name, p)
        parts, pw = B.digit_parts(Bgbit)
        assert (parts > 1) == (name in ("MK256", "MK64-fft"))
        for label, v in D.part_digits(Bgbit).items():
            assert at[label] == [v] * l, (name, label)
        if parts > 1:                                               # the part values the wide kernels' split meets on these words
            cut = np.array([B.cut_parts(int(v), parts, pw) for v in digits.ravel()])
            hp = 1 << (pw - 1)
            assert cut[:, :-1].min() == -hp and cut[:, :-1].max() == hp - 1
            assert cut[:, -1].min() == -hp and cut[:, -1].max() == hp    # the top part takes the carry: one more than a low part can hold
            assert all(sum(int(c) << (pw * w) for w, c in enumerate(row)) == int(v) for row, v in zip(cut, digits.ravel()))


@pytest.mark.parametrize("shape", range(len(IDS)), ids=IDS)
def test_tables_reach_every_target_at_every_amount(O, shape):
    name, bits, N, l, Bgbit = shapes(O)[shape]
    targets = list(D.edge_targets(bits, l, Bgbit).values())
    tables = D.edge_tables(bits, N, l, Bgbit)
    assert len(tables) == D.TABLES and all(t.shape == (N,) and t.dtype == (np.int32 if bits == 32 else np.int64) for pair in tables for t in pair)
    again = D.edge_tables(bits, N, l, Bgbit)
    assert all(np.array_equal(t, u) for pair, pair2 in zip(tables, again) for t, u in zip(pair, pair2))
    missing = D.coverage(tables, bits, targets, used=lambda a: D.tables_at(a, N))
    assert missing == [], (name, len(missing), missing[:8])
    assert all(len(D.tables_at(a, N)) == 1 for a in range(2, 2 * N - 1)) and {D.tables_at(a, N) for a in range(0, 2 * N, 64)} == {(0,), (1,)}
    # the same by the direct route at the amounts of every class: the differences themselves, searched for the words
    want = D.to_words(targets, bits).view(np.uint32 if bits == 32 else np.uint64)
    zero, msb = want.dtype.type(0), want.dtype.type(1 << (bits - 1))
    for a in [1, 2, 63, 64, 65, N // 2, N - 1, N, N + 1, N + 64, 3 * N // 2, 2 * N - 2, 2 * N - 1]:
        for j in range(2):
            got = [D.rotate_minus_self(tables[k][j], a, bits) for k in D.tables_at(a, N)]
            diffs = np.concatenate([g[0] for g in got])
            negated = np.concatenate([g[1][g[2]] for g in got])
            need = want[want % 2 == 0] if a == N else want
            assert np.isin(need, diffs).all(), (name, a, j)
            assert (negated == zero).any() and (negated == msb).any(), (name, a, j)


def test_the_check_itself_can_fail(O):
    # one table alone misses a negated word at the amounts whose only negated coefficient is an end of the polynomial; a table of random words
    # misses nearly everything
    bits, N, l, Bgbit = 32, 1024, 3, 7
    targets = list(D.edge_targets(bits, l, Bgbit).values())
    tables = D.edge_tables(bits, N, l, Bgbit)
    for k in range(D.TABLES):
        alone = D.coverage(tables[k:k + 1], bits, targets)
        assert {(a, what) for a, _, what in alone} == {(1, "negated sign bit" if k == 0 else "negated 0"),
                                                        (2 * N - 1, "negated sign bit" if k == 0 else "negated 0")}
    rng = np.random.default_rng(5)
    rnd = rng.choice(rng.integers(-2**31, 2**31, 16), (1, 2, N)).astype(np.int32)
    assert len(D.coverage(rnd, bits, targets)) > 2 * (2 * N - 1) * len(targets) * 0.9


def test_tables_reach_the_extreme_and_carrying_parts(O):
    # the tlev and r4k kernels cut their digits into 9-bit parts: the digit rows of the CMux on the edge tables, cut as those kernels cut them
    for name in ("MK256", "MK64-fft"):
        s = O.PARAM_SETS[name]
        N, l, Bgbit = s["N"], s["l"], s["Bgbit"]
        parts, pw = B.digit_parts(Bgbit)
        hp = 1 << (pw - 1)
        assert parts == (2 if name == "MK256" else 3) and pw == 9
        for a in (1, 64, N + 65):
            for pair in D.edge_tables(64, N, l, Bgbit):
                rows = B.step_digit_rows(np.stack(pair), a, 64, l, Bgbit)
                assert len(rows) == 2 * l * parts
                for row, w, d in rows:                     # every row of both polynomials: both extremes of its part, the top part's carry
                    assert d.min() == -hp and d.max() == (hp if w == parts - 1 else hp - 1), (name, a, row, w)
