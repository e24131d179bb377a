"""Cases shared by tests/test_mk_lhe_host.py (CPU model) and tests/test_gpu_mk_lhe*.py (device): the leveled CMux and lookup on the 64-bit ring
of degree 2048.  A plain module: parameters, the real key set, the word cases and their model results (computed once and
shared), and the crafted inputs at the transform's exactness bound.  Only numpy is imported at module level."""
import functools

import numpy as np

import bound_inputs as BI

N = 2048
KW = dict(n=8, N=N, k=1, l=2, Bgbit=18, ks_t=8, ks_basebit=2, torus_bits=64, parties=1)   # the CB sets' ring with a small LWE dimension
L, BGBIT = KW["l"], KW["Bgbit"]
SIGMA_BK = 2.0**-62
# lookups of the device file: (d_tree, d_rot), three samples each
LOOKUPS = [(0, 1), (1, 0), (1, 2), (2, 1), (3, 0), (0, 11)]
P_OUT = 8   # real-key tables hold multiples of 1/8


def thetas(d_rot):
    return [t for t in (1, 2, 4) if t <= (N >> d_rot)]


def words64(rng, *shape):
    return rng.integers(-2**63, 2**63, size=shape, dtype=np.int64)


@functools.lru_cache(None)
def keys():
    """(oracle params, MKSecretKeySet, MKOracle) of the real-key cases."""
    import oracle_lib as O
    import thfhe
    from thfhe import keygen
    K = keygen.MKSecretKeySet(thfhe.make_params(**KW), seed=0x5EED2048, sigma_lwe=2.0**-15, sigma_bk=SIGMA_BK, sigma_ks=2.0**-15)
    p = O.make_params(**KW)
    return p, K, O.MKOracle(p, K.bk, K.ksk)


def model_set(words, d):
    import mk_lhe_reference as M
    return M.Set(words, d, L, BGBIT)


@functools.lru_cache(None)
def word_case(d_tree, d_rot, count=3, n_tables=2):
    """Random words as a set of `count` samples and n_tables tables (masks, bodies), with the model's accumulators of every (sample, table,
    encrypted?) the device cases read: dict with set words, tab_a, tab_b, index, and acc(s, table, enc) -> int64[2][N] (memoised)."""
    import mk_lhe_reference as M
    d = d_tree + d_rot
    rng = np.random.default_rng(1000 + 16 * d_tree + d_rot)
    w = words64(rng, count, d, 4, L, N)
    tab_a, tab_b = words64(rng, n_tables, 1 << d_tree, N), words64(rng, n_tables, 1 << d_tree, N)
    S = M.Set(w, d, L, BGBIT)

    @functools.lru_cache(None)
    def acc(s, t, enc):
        return M.lookup_acc(S, s, d_tree, d_rot, tab_a[t] if enc else None, tab_b[t])
    return dict(words=w, d=d, tab_a=tab_a, tab_b=tab_b, acc=acc)


def records(acc, theta):
    """The _wo_keyswitch records int32[theta][N+1] of a model accumulator."""
    import mk_lut_reference as MR
    return np.stack([MR.extract_at(acc.reshape(-1), j, N) for j in range(theta)])


def encode64(v):
    """v / P_OUT as Torus64 words."""
    return (np.asarray(v, np.int64) % P_OUT) << 61


def decode32(phase):
    """Torus32 phases -> multiples of 1 / P_OUT."""
    return ((np.asarray(phase, np.int64) + (1 << 28)) >> 29) % P_OUT


@functools.lru_cache(None)
def real_case(d_tree, d_rot, seed=7):
    """A real-key lookup of every address of a d = d_tree + d_rot bit table of multiples of 1/8: (table values, address bits' TGSW words, encrypted
    table (a, b), public table polynomials)."""
    from thfhe import lut
    p, K, orc = keys()
    d = d_tree + d_rot
    rng = np.random.default_rng(seed)
    values = rng.integers(0, P_OUT, 1 << d)
    tab = lut.lhe_table(values, d_tree, d_rot, encode=encode64, N=N, torus_bits=64)
    bits = lut.lhe_address_bits(np.arange(1 << d), d)
    w = K.tgsw_encrypt(bits, seed=seed + 1).reshape(1 << d, d, 4, L, N)
    ta, tb = K.ring_encrypt(tab, seed=seed + 2)
    return values, w, ta, tb, tab


# ---- the crafted case at the transform's proven bound: 2 l parts N 2^(part bits - 1) 2^15 = 2^37 on this ring ---------------------------------
BOUND = BI.bound(2 * L, N, BGBIT)


def bound_cmux_case():
    """(set words int64[1][1][4][l][N], d1 int64[2][N], d0 = 0): every set word mk_key_word (limbs of the shifted copies near 2^15 with one sign),
    every word of d1 - d0 the word whose digits cut into extreme parts at every level, in all 2 l parts row parts."""
    w = np.full((1, 1, 4, L, N), BI.mk_key_word(BGBIT), np.int64)
    d1 = np.full((2, N), BI.digit_word(64, L, BGBIT), np.int64)
    return w, d1, np.zeros((2, N), np.int64)


def bound_rot_table(box):
    """Table polynomial(s) int64[N] whose rotation step by `box` has the difference digit_word everywhere (bound_inputs.lhe_rot_table on Torus64):
    segment r holds (r - m / 2) T."""
    m = N // box
    assert m >= 2 and m * box == N
    T = BI.digit_word(64, L, BGBIT)
    return np.array([BI.wrap((r - m // 2) * T, 64) for r in range(m)], np.int64).repeat(box)


def bound_reached(set_bit_words, diff):
    """Exact peak limb sum (Python integers) of C (.) diff over all row parts, the larger of the two outputs: set_bit_words int64[4][l][N], diff
    int64[2][N]."""
    import mk_lhe_reference as M
    parts, pw = BI.digit_parts(BGBIT)
    dg = M.decompose(diff, L, BGBIT)          # [2][l parts][N]
    best = 0
    for o in range(2):
        pairs = []
        for j in range(2):
            for lv in range(L):
                for part in range(parts):
                    key = BI.shifted(set_bit_words[M.part_index(j, o), lv], pw, part, 64)
                    pairs.append((dg[j, lv * parts + part], key))
        best = max(best, BI.peak_limb_sum(pairs, 64))
    return best
