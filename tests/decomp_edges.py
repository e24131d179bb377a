"""Accumulators whose CMux difference X^a acc - acc lands on the digit edges of the gadget decomposition at EVERY rotation amount -- TEST
INFRASTRUCTURE ONLY; only numpy (and conv_edges) is imported at the top, bound_inputs (and with it the oracle) by the functions that cut digits.

A blind-rotation kernel opens a CMux by forming d = X^a acc - acc from the accumulator in the LDS and cutting d into gadget digits: the index
and sign of the rotated word depend on the amount a, the digits on the word d.  edge_words() lists the words d at which that cut can go wrong
(all fields 0, all fields full, the wrap of d + offset, the last dropped bit, a field that overflows into its neighbour, the 9-bit part split
of the wide Torus64 digits); edge_tables() builds (mask, body) polynomial pairs t on the words {0, e, -e} such that the difference has a
coefficient at every target word for every amount, and meets the sign path (r + M) ^ M on the rotated words 0 and 2^(bits-1).  coverage() checks
that, coefficient by coefficient; tests/test_decomp_edges_host.py asserts it for every shape the GPU tests use.

Two things no polynomial can do:
  * at a = 1 the only negated rotated word is t[N-1] (at a = 2N - 1: t[0]); it cannot be 0 and 2^(bits-1) at once.  So edge_tables() returns two
    tables, each complete at every other amount; a job at amount a takes one of tables_at(a, N) through lut_index -- both at those two amounts --
    and the condition is "for every amount, over the tables used at that amount";
  * at a = N the difference is -2 t: only the even targets exist there, and coverage() asks for those alone at that amount."""
import numpy as np

import conv_edges as E

TABLES = 2
ZEROS = 0.4        # share of a polynomial's coefficients that hold 0: the partner of every target word


def tables_at(a, N):
    """the edge tables a sweep runs at the amount a: one of them, by a hash of a (no class of amounts falls to one table); both where one cannot
    hold the two negated words"""
    a = int(a) % (2 * N)
    return (0, 1) if a in (1, 2 * N - 1) else ((a * 2654435761 >> 15) & 1,)


def unsigned(v, bits):
    return int(v) & ((1 << bits) - 1)


def to_words(values, bits):
    """Python integers taken mod 2^bits as int32 / int64 words"""
    return E.to_i64(values) if bits == 64 else E.to_i32([unsigned(v, 32) for v in values])


def digit_target(v, bits, l, Bgbit):
    """the word that decomposes to the digit v at every level"""
    import bound_inputs as B
    half = 1 << (Bgbit - 1)
    assert -half <= v < half
    return unsigned(sum((v + half) << (bits - p * Bgbit) for p in range(1, l + 1)) - B.decomp_offset(bits, l, Bgbit), bits)


def part_digits(Bgbit):
    """Digits of a base cut into balanced 9-bit parts (label -> digit): every part at its most negative (the top part as far as the digit range
    allows: bound_inputs.extreme_digit), every part at its largest, a low part of exactly 2^(pw-1) that carries one into the next part, and that
    carry running through every part into the top one."""
    import bound_inputs as B
    parts, pw = B.digit_parts(Bgbit)
    if parts == 1:
        return {}
    hp = 1 << (pw - 1)
    out = {
        "parts all lowest": B.extreme_digit(Bgbit),
        "parts all highest": sum((hp - 1) << (pw * w) for w in range(parts)),
        "low part carries": hp,
        "carry through every part": hp + sum((hp - 1) << (pw * w) for w in range(1, parts)),
    }
    assert B.cut_parts(out["parts all lowest"], parts, pw)[:-1] == [-hp] * (parts - 1)
    assert B.cut_parts(out["parts all highest"], parts, pw) == [hp - 1] * parts
    assert B.cut_parts(out["low part carries"], parts, pw) == [-hp, 1] + [0] * (parts - 2)
    assert B.cut_parts(out["carry through every part"], parts, pw) == [-hp] * (parts - 1) + [hp]
    return out


def edge_targets(bits, l, Bgbit, unique=True):
    """label -> target difference d (unsigned, mod 2^bits); unique: a word reached under two labels keeps the first"""
    import bound_inputs as B
    M, off, half = 1 << bits, B.decomp_offset(bits, l, Bgbit), 1 << (Bgbit - 1)
    t = {
        "every field 0": -off,
        "d + offset all ones": M - 1 - off,
        "d + offset wraps": M - off + 1,
        "0": 0, "1": 1, "-1": -1, "sign bit": M >> 1, "sign bit - 1": (M >> 1) - 1,
    }
    if l * Bgbit < bits:
        t["dropped bits all set"] = (1 << (bits - l * Bgbit)) - 1
        t["last kept bit"] = 1 << (bits - l * Bgbit)
    for p in range(1, l + 1):
        t["level %d overflows" % p] = half << (bits - p * Bgbit)
    for name, v in part_digits(Bgbit).items():
        t[name] = digit_target(v, bits, l, Bgbit)
    out, seen = {}, set()
    for name, v in t.items():
        if not unique or unsigned(v, bits) not in seen:
            seen.add(unsigned(v, bits))
            out[name] = unsigned(v, bits)
    return out


def edge_words(bits, l, Bgbit):
    """the target differences d as int32 / int64 words"""
    return to_words(edge_targets(bits, l, Bgbit).values(), bits)


def expected_digits(d, bits, l, Bgbit):
    """the gadget digits of the word d from the definition, with Python integers: ((d + offset) >> (bits - p Bgbit)) mod Bg - Bg/2, p = 1 .. l"""
    import bound_inputs as B
    s = unsigned(unsigned(d, bits) + B.decomp_offset(bits, l, Bgbit), bits)
    return [((s >> (bits - p * Bgbit)) & ((1 << Bgbit) - 1)) - (1 << (Bgbit - 1)) for p in range(1, l + 1)]


def _polynomial(targets, bits, N, rng, k):
    """One polynomial of table k: 0 at ZEROS of the coefficients, the rest dealt evenly over the words e and -e of every target at pseudo-random
    places (so that some pair (c, c - a) holds (-e, 0), (0, e) or (0, -e) with the sign that makes the difference e, whatever a is), one word w with
    -2 w = e for every even target (a = N), and the four end coefficients that carry the negated words of the amounts next to 0 and 2N."""
    M, msb = 1 << bits, 1 << (bits - 1)
    words = list(dict.fromkeys(w for e in targets if e for w in (e, (M - e) % M)))
    halves = [((M - e) % M) // 2 + k * msb for e in targets if e and e % 2 == 0]
    free = rng.permutation(np.arange(2, N - 2))
    copies = (int((1 - ZEROS) * N) - len(halves)) // len(words)
    assert copies >= 8, (N, len(words))
    t = [0] * N
    for i, w in enumerate(halves + words * copies):
        t[free[i]] = w
    ends = (0, msb, msb, 0) if k == 0 else (msb, 0, 0, msb)
    t[0], t[1], t[N - 2], t[N - 1] = ends
    return to_words(t, bits)


def edge_table(bits, N, l, Bgbit, rng):
    """TABLES tables, each a (mask, body) pair of N words: over the tables of tables_at(a, N), every amount a in 1 .. 2N - 1 finds every target of
    edge_words() (a = N: every even one) among the coefficients of X^a t - t, in the mask and in the body, and a negated rotated word 0 and
    2^(bits-1) in both.  (The words are placed at random: coverage() is what says so, in test_decomp_edges_host.py.)"""
    targets = list(edge_targets(bits, l, Bgbit).values())
    return [(_polynomial(targets, bits, N, rng, k), _polynomial(targets, bits, N, rng, k)) for k in range(TABLES)]


def edge_tables(bits, N, l, Bgbit):
    """the tables of a shape, the same wherever they are asked for: what the host test asserts holds for the tables the GPU tests run"""
    return edge_table(bits, N, l, Bgbit, np.random.default_rng([0xDEC0, bits, N, l, Bgbit]))


def amount_word(a, N, rng=None):
    """the Torus32 mask or body word that mod-switches to the amount a of Z_2N: a 2^32 / 2N, with rng anywhere inside its rounding interval"""
    step = E.mod_step(N, 1)
    a = np.asarray(a, np.int64)
    return E.to_i32(a * step + (rng.integers(-(step // 2) + 1, step // 2, a.shape) if rng is not None else 0))


def structured_members(N):
    """the amounts every structured set holds: each multiple of 64 (the register a lane's read starts in), +-1 around 0, N/2, N and 3N/2 (the sign
    wrap entering, crossing the middle of, and leaving a lane's 16 reads), 2N - 1"""
    return set(range(0, 2 * N, 64)) | {(c + s) % (2 * N) for c in (0, N // 2, N, 3 * N // 2) for s in (-1, 1)} | {2 * N - 1}


def structured_amounts(N, rng, extra=64):
    """structured_members(N), every residue mod 64 (the lane) each in a register of its own choice, and `extra` random amounts: sorted, no amount twice"""
    lanes = {r + 64 * int(k) for r, k in zip(range(64), rng.integers(0, 2 * N // 64, 64))}
    fixed = structured_members(N) | lanes
    rest = rng.choice(np.setdiff1d(np.arange(2 * N), sorted(fixed)), extra, replace=False)
    return np.array(sorted(fixed | set(rest.tolist())), np.int64)


def rotate_minus_self(t, a, bits):
    """(X^a t - t mod X^N + 1, the rotated words before their sign, where the sign is minus) for one amount, as unsigned words"""
    u = np.ascontiguousarray(t).view(np.uint32 if bits == 32 else np.uint64)
    N = len(u)
    idx = (np.arange(N) - a) & (2 * N - 1)
    r, neg = u[idx & (N - 1)], idx >= N
    return np.where(neg, (~r) + u.dtype.type(1), r) - u, r, neg


def coverage(tables, bits, targets, used=None, chunk=256):
    """What the tables miss: a list of (amount, polynomial 0 = mask / 1 = body, what) -- empty when the condition of edge_table() holds.  used:
    amount -> indices of the tables run at that amount (tables_at; default: all of them at every amount).  Every pair (amount, coefficient) is
    visited: the tables hold few distinct words, so the difference of a pair is looked up by the two words' codes and the sign in a table that
    Python integers filled."""
    M, msb = 1 << bits, 1 << (bits - 1)
    targets = [unsigned(e, bits) for e in targets]
    T, N = len(targets), len(tables[0][0])
    where = {e: i for i, e in enumerate(targets)}
    found = np.zeros((len(tables), 2, 2 * N, T + 3), bool)   # T: no target; T + 1 / T + 2 (second lookup): a negated rotated 0 / 2^(bits-1)
    for k, pair in enumerate(tables):
        for j, t in enumerate(pair):
            u = [unsigned(v, bits) for v in np.asarray(t).tolist()]
            values = sorted(set(u))
            at = {v: i for i, v in enumerate(values)}
            code = np.array([at[v] for v in u])
            V = len(values)
            lut = np.full((2, V, V), T, np.int16)       # [sign][rotated word][own word] -> target index
            for s in range(2):
                for ie, ve in enumerate(values):
                    for ic, vc in enumerate(values):
                        lut[s, ie, ic] = where.get(((M - ve if s else ve) - vc) % M, T)
            special = np.full((2, V), T, np.int16)
            if 0 in values:
                special[1, values.index(0)] = T + 1
            if msb in values:
                special[1, values.index(msb)] = T + 2
            for a0 in range(0, 2 * N, chunk):
                a = np.arange(a0, min(a0 + chunk, 2 * N))
                idx = (np.arange(N)[None, :] - a[:, None]) & (2 * N - 1)
                s, ce = (idx >= N).astype(np.intp), code[idx & (N - 1)]
                found[k, j, a[:, None], lut[s, ce, code[None, :]]] = True
                found[k, j, a[:, None], special[s, ce]] = True
    missing = []
    names = list(range(T)) + [None, "negated 0", "negated sign bit"]
    for j in range(2):
        for a in range(1, 2 * N):
            run = list(used(a)) if used else list(range(len(tables)))
            for i in np.flatnonzero(~found[run, j, a].any(axis=0)):
                if i == T or (a == N and i < T and targets[i] % 2):
                    continue
                missing.append((a, j, names[i]))
    return missing
