"""Rounding edges of the 3-gen engine's two ends -- TEST INFRASTRUCTURE ONLY; only numpy is imported here, the oracle and
the HIP library are loaded by the tests that need them.

  * the Torus64 -> Torus32 conversion t64tot32 = trunc(Int32, Float64(d) / 2^32) (J/numeric-functions.jl:109-111): the Int64 -> Float64 step rounds
    to nearest-even, so from |d| >= 2^53 on a word at most half an ulp below a multiple of 2^32 converts to that multiple's quotient, not to the
    one below it, and 2^63 - 512 and above wrap to INT32_MIN.  edge_words() holds such words for every binade; trunc_shift() is the exact-integer
    truncation that uniform random words cannot tell from the real thing (test_conv_edges_host.py);
  * the start X^{-bar} tv and the extraction at coefficient j over Torus64, vectorised over whole batches (mk_lut_reference's go through the oracle
    word by word), and body words whose mod-switch takes every rotation amount of a ring degree, the interval ends included."""
import numpy as np

BINADES = range(53, 63)   # |d| in [2^e, 2^(e+1)): the spacing of doubles there is ulp = 2^(e-52) >= 2


def to_i64(values):
    """Python integers taken mod 2^64 as int64 words."""
    return np.array([((int(v) + (1 << 63)) % (1 << 64)) - (1 << 63) for v in values], np.int64)


def neg64(a):
    """negation mod 2^64 (-(-2^63) = -2^63)"""
    return (np.uint64(0) - np.ascontiguousarray(a, np.int64).view(np.uint64)).view(np.int64)


def edge_words():
    """int64 words around the multiples of 2^32 where Float64(d) rounds: for every binade e = 53 .. 62 and quotients k just above 2^(e-32) (odd,
    even) and just below 2^(e-31) (even, odd) the words k 2^32 +- r, r in {1, ulp/2 - 1, ulp/2, ulp/2 + 1, ulp, ulp + 1} (r > 0), and their
    negations; then the small and the saturating words.  No word twice."""
    w = []
    for e in BINADES:
        ulp, base = 1 << (e - 52), 1 << (e - 32)
        for k in (base + 1, base + 2, 2 * base - 2, 2 * base - 1):
            for r in (1, ulp // 2 - 1, ulp // 2, ulp // 2 + 1, ulp, ulp + 1):
                if r > 0:
                    for v in (k * (1 << 32) + r, k * (1 << 32) - r):
                        w += [v, -v]
    w += [0, 1, -1, 2**32 - 1, -(2**32 - 1), 2**32, -2**32, 2**32 + 1, -(2**32 + 1), 2**63 - 1, 2**63 - 512, 2**63 - 513, -2**63, -2**63 + 1,
          -2**63 + 512, -2**63 + 513]
    return to_i64(dict.fromkeys(w))


SATURATING = to_i64([2**63 - 1, 2**63 - 512])   # Float64(d) = 2^63: the quotient 2^31 wraps to INT32_MIN


def binade(a):
    """floor(log2 |d|) of every word (-1 for 0; 63 for -2^63)"""
    return np.array([abs(int(v)).bit_length() - 1 for v in np.ravel(a)]).reshape(np.shape(a))


def t64tot32(d):
    """oracle_t64tot32 on an array: trunc(Float64(d) / 2^32) toward zero, the one double that reaches 2^31 wrapped to INT32_MIN
    (test_conv_edges_host.py holds it against the oracle's word by word)."""
    v = np.trunc(np.asarray(d, np.int64).astype(np.float64) / 4294967296.0)
    return np.where(v >= 2147483648.0, -2147483648.0, v).astype(np.int64).astype(np.int32)


def trunc_shift(d):
    """The WRONG conversion, for the tests that show the edge words bite: the exact integer quotient d / 2^32 truncated toward zero (what shifts,
    or an integer division, would give).  It equals t64tot32 on every word the GPU suite's random inputs are likely to contain."""
    d = np.asarray(d, np.int64)
    q = d >> 32                                                # floor
    return (q + ((d < 0) & ((d & 0xFFFFFFFF) != 0))).astype(np.int32)


def biting_words():
    """the edge words on which the two conversions differ, dealt round-robin over (binade, sign): any run of 20 neighbours meets every binade with
    both signs as long as the groups last (the smallest, binade 53, holds 4 words per sign)"""
    e = edge_words()
    e = e[t64tot32(e) != trunc_shift(e)]
    group = 2 * binade(e) + (e < 0)
    rank, seen = np.zeros(len(e), np.int64), {}
    for i, g in enumerate(group.tolist()):
        rank[i] = seen.get(g, 0)
        seen[g] = rank[i] + 1
    return e[np.lexsort((group, rank))]


def tiled(words, N, offset=0):
    """int64[N]: the words from cyclic position `offset` on, repeated to N"""
    return np.resize(np.roll(np.asarray(words, np.int64), -offset), N)


def start64(tv, bar, N):
    """X^{-bar} tv mod X^N + 1 over Torus64 for a batch: tv int64[N] or int64[jobs][N], bar int[jobs] -> int64[jobs][N]; coefficient q is
    tv[(q + bar) mod N], negated mod 2^64 where (q + bar) mod 2N >= N (mk_lut_reference.monomial64(tv, -bar, N))."""
    bar = np.asarray(bar, np.int64).reshape(-1)
    tv = np.broadcast_to(np.asarray(tv, np.int64), (bar.shape[0], N))
    e = (np.arange(N, dtype=np.int64)[None, :] + bar[:, None]) & (2 * N - 1)
    v = np.take_along_axis(tv, e & (N - 1), axis=1)
    return np.where((e & N) != 0, neg64(v), v)


def extract_at64(acc, j, N, convert=t64tot32):
    """LWE(N) records of coefficient j of the accumulators acc int64[..][2][N] (or [..][2N]): t64tot32(a_{j-i}) for i <= j, t64tot32(-a_{N+j-i}) for
    i > j (negated mod 2^64 first), t64tot32(body_j) -> int32[..][N+1] (mk_lut_reference.extract_at).  convert: what is applied to the int64 words
    instead of t64tot32 (the identity, or the wrong conversion)."""
    acc = np.asarray(acc, np.int64)
    acc = acc.reshape(acc.shape[:-2] + (2 * N,)) if acc.shape[-1] == N else acc
    i = np.arange(N)
    v = acc[..., (j - i) % N]
    v = np.where(i <= j, v, neg64(v))
    return convert(np.concatenate([v, acc[..., N + j:N + j + 1]], axis=-1))


def binades_told_apart(words):
    """the binades of the int64 words on which t64tot32 and trunc_shift differ: a comparison of their conversions could have failed there"""
    words = np.asarray(words, np.int64).reshape(-1)
    return set(binade(words[t64tot32(words) != trunc_shift(words)]).tolist())


def mod_step(N, theta):
    """one step of the theta-rounded mod-switch in Torus32 words: 2^32 theta / 2N"""
    return (1 << 32) // (2 * N // theta)


def interval_ends(N, theta):
    """the rounding-interval ends around 0 = 2^32 (the wrap), 1/2 (bar = N = -N), one step and 2^32 - one step: c, c +- 1, c - step/2 - 1,
    c - step/2, c + step/2 - 1, c + step/2 (a mod-switch rounds c + step/2 up and leaves c + step/2 - 1)"""
    step = mod_step(N, theta)
    out = []
    for c in (0, 1 << 31, step, (1 << 32) - step):
        out += [c, c - 1, c + 1, c - step // 2 - 1, c - step // 2, c + step // 2 - 1, c + step // 2]
    return to_i32(out)


def to_i32(v):
    """integers taken mod 2^32 as int32 words"""
    return (np.asarray(v, np.int64) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)


def amount_words(N, theta, rng):
    """int32 body words whose theta-rounded mod-switch takes every multiple of theta in Z_2N, each at a random place inside its rounding interval,
    followed by interval_ends(N, theta)"""
    step = mod_step(N, theta)
    k = np.arange(2 * N // theta, dtype=np.int64)
    w = k * step + rng.integers(-(step // 2) + 1, step // 2, k.shape[0])
    return np.concatenate([to_i32(w), interval_ends(N, theta)])


# multi-value taps at p = 2 (mk_mv_lut_reference.tap_positions: J_0 = 3N/4, J_1 = N/4, so an output word combines tv0[m] and tv0[m + N/2]): every
# single tap with both signs, and every sign pattern of the two taps -- whatever signs the rotation gives the two words, one of the four outputs is
# +(their sum) and one -(their sum)
MV_TAPS_ONE = np.array([[1, 0], [-1, 0], [0, 1], [0, -1]], np.int32)
MV_TAPS_TWO = np.array([[1, 1], [1, -1], [-1, 1], [-1, -1]], np.int32)


def two_tap_base(target, rng, N):
    """int64[N] = (R, target - R) mod 2^64 with R uniform random: words N/2 apart sum to the target words int64[N/2] while neither is one of them"""
    target = np.asarray(target, np.int64).view(np.uint64)
    r = rng.integers(-2**63, 2**63, N // 2, dtype=np.int64).view(np.uint64)
    return np.concatenate([r, target - r]).view(np.int64)
