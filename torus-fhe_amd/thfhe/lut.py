"""Host helpers of programmable bootstrapping (include/thfhe_hip.h, thfhe_lut_bootstrap): the padding-bit integer encoding and the
test-vector layout the blind rotation expects.

A message m in [0, p), p a power of two, is the Torus32 word m * 2^32 / (2p): its phase stays in [0, 1/2), so the negacyclic wrap never
inverts a valid input.  In a test vector of N words, message m owns the box of N/p coefficients centred on m*N/p; entry i of the box holds
f_{i mod theta}(m), and the lower half-box of m = 0 wraps to the top of the vector with its sign negated.  A rotation by a phase inside
m's box, rounded to a multiple of theta, then brings f_0(m) .. f_{theta-1}(m) to coefficients 0 .. theta-1.

The 3-gen multi-key engine (MKCloudKey.lut_bootstrap, thfhe_mk_lut_bootstrap) rotates a Torus64 accumulator: its test vectors and output
words take torus_bits=64 (m * 2^64 / (2p); booleans +-2^61, the 3-gen gate encoding).  The inputs stay Torus32 records (encode) either way.
"""
import numpy as np

MU8 = 1 << 29  # the boolean encoding of the gates: true = +2^29, false = -2^29
MU8_64 = 1 << 61  # the same on Torus64 (the 3-gen gates)


def _check_p(p):
    if p < 2 or p & (p - 1):
        raise ValueError(f"p must be a power of two >= 2, got {p}")


def _to_i32(v):
    return (np.asarray(v, np.int64) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)


def _check_bits(torus_bits):
    if torus_bits not in (32, 64):
        raise ValueError(f"torus_bits must be 32 or 64, got {torus_bits}")


def _to_i64(v):
    """Python integers taken mod 2^64 as int64 words."""
    return np.array([int(x) % (1 << 64) for x in np.ravel(v)], np.uint64).view(np.int64).reshape(np.shape(v))


def encode(m, p):
    """Torus32 words of the messages m in [0, p) (padding bit): m * 2^32 / (2p)."""
    _check_p(p)
    m = np.asarray(m, np.int64)
    if np.any((m < 0) | (m >= p)):
        raise ValueError(f"messages must lie in [0, {p})")
    return _to_i32(m * ((1 << 32) // (2 * p)))


def decode(phase_words, p):
    """Nearest message of each phase: round(phase * 2p / 2^32) mod 2p.  A valid result lies in [0, p); p .. 2p-1 means the phase left [0, 1/2)."""
    _check_p(p)
    u = np.asarray(phase_words, np.int64) & 0xFFFFFFFF
    step = (1 << 32) // (2 * p)
    return ((u + step // 2) // step) % (2 * p)


def test_vector(tables, p, theta=1, N=1024, torus_bits=32):
    """int32[N] test vector: tables = theta arrays of p Torus32 output words (tables[j][m] = f_j(m)); with theta = 1 one array of p words will do.
    torus_bits=64: int64[N] from Torus64 output words (the multi-key engine)."""
    _check_p(p)
    _check_bits(torus_bits)
    if theta not in (1, 2, 4):
        raise ValueError("theta must be 1, 2 or 4")
    T = np.asarray(tables, np.int64)
    if T.ndim == 1 and theta == 1:
        T = T[None]
    if T.shape != (theta, p):
        raise ValueError(f"expected {theta} tables of {p} words, got shape {T.shape}")
    box = N // p
    if box < 2 or (box // 2) % theta:
        raise ValueError(f"p = {p} leaves half-boxes of {box // 2} coefficients: not a multiple of theta = {theta}")
    i = np.arange(N)
    m = (i + box // 2) // box          # 0 .. p; p = the lower half-box of m = 0, wrapped to the top
    wrap = m == p
    v = T[i % theta, np.where(wrap, 0, m)]
    if torus_bits == 64:
        return np.where(wrap, -v, v)   # int64 negation wraps mod 2^64
    return _to_i32(np.where(wrap, -v, v))


def int_outputs(f, p_out, p=None, torus_bits=32):
    """Table of integer outputs: encode(f(m), p_out) for m in [0, p) (p defaults to p_out); f(m) is taken mod p_out.
    torus_bits=64: the Torus64 words f(m) * 2^64 / (2 p_out) as int64."""
    p = p_out if p is None else p
    _check_p(p)
    _check_bits(torus_bits)
    if torus_bits == 64:
        _check_p(p_out)
        return _to_i64([(int(f(m)) % p_out) * ((1 << 64) // (2 * p_out)) for m in range(p)])
    return encode(np.array([int(f(m)) % p_out for m in range(p)], np.int64), p_out)


def bool_outputs(f, p, torus_bits=32):
    """Table of boolean outputs in the gates' encoding (+2^29 if f(m) else -2^29): LUT results that feed thfhe's gates.
    torus_bits=64: +-2^61 as int64, the encoding of the 3-gen multi-key gates."""
    _check_p(p)
    _check_bits(torus_bits)
    if torus_bits == 64:
        return np.array([MU8_64 if f(m) else -MU8_64 for m in range(p)], np.int64)
    return _to_i32(np.array([MU8 if f(m) else -MU8 for m in range(p)], np.int64))


def tree_test_vectors(f, p_hi, p_lo, p_out, theta=1, N=1024, torus_bits=32):
    """Level-1 test vectors of the two-digit tree (thfhe_tree_lut_bootstrap) for f(hi, lo), taken mod p_out: int32[p_hi / theta][N],
    row r = test_vector of the theta functions lo -> f(r theta + j, lo), j < theta, at modulus p_lo.  torus_bits=64: int64 rows of Torus64 words
    (thfhe_mk_tree_lut_bootstrap)."""
    _check_p(p_hi)
    _check_bits(torus_bits)
    if theta not in (1, 2, 4) or p_hi % theta:
        raise ValueError("theta must be 1, 2 or 4 and divide p_hi")
    return np.stack([test_vector([int_outputs(lambda lo, h=r * theta + j: f(h, lo), p_out, p_lo, torus_bits) for j in range(theta)], p_lo, theta, N,
                                 torus_bits) for r in range(p_hi // theta)])


def mv_base(step, N=1024, torus_bits=32):
    """Base vector of a multi-value bootstrap (thfhe_mv_lut_bootstrap): int32[N] = (step/2, ..., step/2).  Times the factor of an integer
    table f (mv_factors) it is test_vector(f * step, p): output j of the rotation carries f_j(m) * step.  step: an even Torus32 word, e.g.
    2^32 / (2 p_out) for outputs in the padding-bit encoding at modulus p_out.  torus_bits=64: int64[N] from an even Torus64 step (the multi-key
    engine, thfhe_mk_mv_lut_bootstrap)."""
    _check_bits(torus_bits)
    step = int(step)
    if step % 2:
        raise ValueError("step must be even (the base vector holds step / 2)")
    if torus_bits == 64:
        return _to_i64([step // 2] * N)
    return _to_i32(np.full(N, step // 2, np.int64))


def mv_factors(int_tables, p):
    """Factors int32[q][p] of q integer tables (int_tables[j][m] = f_j(m), m in [0, p)): c_k = f(k+1) - f(k) for k < p-1, c_{p-1} = -(f(0) + f(p-1)),
    the coefficient of X^(N/(2p) + k N/p).  The integers are taken as given, not reduced: f and f + p_out give outputs half a torus apart.  The
    rotation's noise reaches output j times the 2-norm of row j, so small differences between neighbouring entries are cheap."""
    _check_p(p)
    f = np.asarray(int_tables, np.int64)
    if f.ndim == 1:
        f = f[None]
    if f.ndim != 2 or f.shape[1] != p:
        raise ValueError(f"expected q tables of {p} integers, got shape {f.shape}")
    c = np.empty_like(f)
    c[:, :-1] = f[:, 1:] - f[:, :-1]
    c[:, -1] = -(f[:, 0] + f[:, -1])
    if np.any(np.abs(c) >= 1 << 31):
        raise ValueError("factor out of the int32 range")
    return c.astype(np.int32)


def mv_bool_factors(bit_tables, p, torus_bits=32, N=1024):
    """(tv0, factors, out_bias) of q bit tables (bit_tables[j][m] in {0, 1}, m in [0, p)) whose outputs leave the rotation in the gates' encoding
    +-mu (mu = 2^29, or 2^61 with torus_bits=64): the 0/1 tables at step 2 mu with the bias -mu added after the combination, so that a tap is a
    difference of bits -- half the taps, and half the rotation noise at the output, of +-1 tables at step mu.  out_bias is the argument of that name of
    thfhe_mk_mv_lut_bootstrap; the single-key entry has none (add it to the body words)."""
    _check_bits(torus_bits)
    f = np.asarray(bit_tables, np.int64)
    if np.any((f != 0) & (f != 1)):
        raise ValueError("bit tables hold 0 and 1 only")
    mu = MU8_64 if torus_bits == 64 else MU8
    return mv_base(2 * mu, N, torus_bits), mv_factors(f, p), -mu


def tree_mv_factors(f, p_hi, p_lo, p_out, N=1024, torus_bits=32):
    """(tv0, factors) of thfhe_tree_lut_bootstrap_mv for f(hi, lo), taken mod p_out: the base vector at step 2^32 / (2 p_out) and int32[p_hi][p_lo],
    row h = the factor of lo -> f(h, lo).  Candidate h of the one level-1 rotation then carries encode(f(h, lo), p_out).  torus_bits=64: the int64
    base vector at step 2^64 / (2 p_out) (thfhe_mk_tree_lut_bootstrap_mvk); the factors are the same integers."""
    _check_p(p_hi)
    _check_p(p_out)
    _check_bits(torus_bits)
    tab = [[int(f(h, lo)) % p_out for lo in range(p_lo)] for h in range(p_hi)]
    return mv_base((1 << torus_bits) // (2 * p_out), N, torus_bits), mv_factors(tab, p_lo)


def tree_mvk_factors(fs, p_hi, p_lo, p_out=2, N=1024, torus_bits=32):
    """(tv0, factors) of thfhe_tree_lut_bootstrap_mvk for the k functions fs[j](hi, lo), taken mod p_out: one base vector and
    int32[k][p_hi][p_lo], block j = tree_mv_factors(fs[j]).  Output j p_hi + h of the one level-1 rotation is candidate h of function j.  p_out = 2
    (bit-valued outputs) is what the named parameter sets carry through the two rotations; k p_hi <= 64.  torus_bits=64: the int64 base vector of
    thfhe_mk_tree_lut_bootstrap_mvk."""
    fs = list(fs)
    if not fs or len(fs) * p_hi > 64:
        raise ValueError("1 <= k and k * p_hi <= 64 (the outputs of one multi-value rotation)")
    parts = [tree_mv_factors(f, p_hi, p_lo, p_out, N, torus_bits) for f in fs]
    return parts[0][0], np.stack([w for _, w in parts])


def tree_mvk_bool_factors(fs, p_hi, p_lo, N=1024, torus_bits=32):
    """(tv0, factors, out_bias) of a multi-value tree whose k bit functions fs[j](hi, lo) in {0, 1} leave the tree in the gates' encoding +-mu: the
    0/1 tables of mv_bool_factors (a tap is a difference of bits: half the taps of +-1 tables) as int32[k][p_hi][p_lo], and the bias -mu that
    thfhe_mk_tree_lut_bootstrap_mvk adds to every level-1 candidate (its out_bias), so that the packed tables hold +-mu."""
    fs = list(fs)
    _check_p(p_hi)
    if not fs or len(fs) * p_hi > 64:
        raise ValueError("1 <= k and k * p_hi <= 64 (the outputs of one multi-value rotation)")
    tabs = [[[int(f(h, lo)) for lo in range(p_lo)] for h in range(p_hi)] for f in fs]
    tv0, w, bias = mv_bool_factors(np.asarray(tabs, np.int64).reshape(len(fs) * p_hi, p_lo), p_lo, torus_bits, N)
    return tv0, w.reshape(len(fs), p_hi, p_lo), bias


def lhe_table(functions, d_tree, d_rot, theta=1, encode=None, N=1024, torus_bits=32):
    """Table polynomials of a leveled lookup (thfhe_lhe_lookup): int32[2^d_tree][N] from theta integer tables of 2^(d_tree + d_rot)
    entries (functions[j][e] = f_j(e); with theta = 1 one table will do).  Entry e of function j sits at coefficient (e mod 2^d_rot) * box + j of
    polynomial e >> d_rot, box = N >> d_rot -- the many-LUT layout without the half-box offset: the address is exact, not a noisy phase.  The other
    coefficients of a box are zero.  encode: integers -> Torus32 words (e.g. lambda v: lut.encode(v, 8)); None: the entries are the words.
    N = 2048, torus_bits = 64 (thfhe_mk_lhe_lookup): int64[2^d_tree][2048] of Torus64 words, d_rot up to 11."""
    if torus_bits not in (32, 64):
        raise ValueError("torus_bits must be 32 or 64")
    max_rot = N.bit_length() - 1
    if not (0 <= d_tree <= 6 and 0 <= d_rot <= max_rot):
        raise ValueError(f"d_tree must be 0 .. 6 and d_rot 0 .. {max_rot}")
    box = N >> d_rot
    if theta not in (1, 2, 4) or theta > box:
        raise ValueError("theta must be 1, 2 or 4 and at most box = N >> d_rot")
    F = np.asarray(functions, np.int64)
    if F.ndim == 1 and theta == 1:
        F = F[None]
    entries = 1 << (d_tree + d_rot)
    if F.shape != (theta, entries):
        raise ValueError(f"expected {theta} tables of {entries} entries, got shape {F.shape}")
    words = np.asarray(encode(F), np.int64) if encode is not None else F
    tab = np.zeros((1 << d_tree, N), np.int64)
    e = np.arange(entries)
    for j in range(theta):
        tab[e >> d_rot, (e & ((1 << d_rot) - 1)) * box + j] = words[j]
    return tab if torus_bits == 64 else _to_i32(tab)


def lhe_value(values, encode=None, N=1024):
    """Value polynomial(s) of a leveled scatter (thfhe_lhe_scatter): values int[k] -> int32[N] with f_j = values[j] at coefficient j
    and zero elsewhere; int[n_vals][k] -> int32[n_vals][N].  Written at address e with box = N >> d_rot >= k, f_j lands where entry e of function j
    sits in lhe_table's layout; k > box spills into the neighbouring entries.  encode: integers -> Torus32 words; None: the values are the words."""
    F = np.asarray(values, np.int64)
    if F.ndim == 0:
        F = F[None]
    if F.ndim > 2 or F.shape[-1] < 1 or F.shape[-1] > N:
        raise ValueError(f"expected int[k] or int[n_vals][k] with 1 <= k <= {N}, got shape {F.shape}")
    words = np.asarray(encode(F), np.int64) if encode is not None else F
    val = np.zeros(F.shape[:-1] + (N,), np.int64)
    val[..., :F.shape[-1]] = words
    return _to_i32(val)


def lhe_table_entries(polys, d_tree, d_rot, theta=1, N=1024):
    """The inverse of lhe_table's layout: from words int[2^d_tree][N] (e.g. the phases of a scattered table) the entries int[theta][2^(d_tree + d_rot)],
    entry e of function j read at coefficient (e mod 2^d_rot) * box + j of polynomial e >> d_rot."""
    if not (0 <= d_tree <= 6 and 0 <= d_rot <= 10) or theta < 1 or theta > (N >> d_rot):
        raise ValueError("d_tree must be 0 .. 6, d_rot 0 .. 10 and 1 <= theta <= box = N >> d_rot")
    P = np.asarray(polys).reshape(1 << d_tree, N)
    e = np.arange(1 << (d_tree + d_rot))
    return np.stack([P[e >> d_rot, (e & ((1 << d_rot) - 1)) * (N >> d_rot) + j] for j in range(theta)])


def lhe_address_bits(addresses, d):
    """Bits of the addresses, low bit first, sample-major: int32[len(addresses) * d], bit i of address s at s d + i -- the order
    SecretKeySet.tgsw_encrypt -> CloudKey.tgsw_set expects."""
    a = np.asarray(addresses, np.int64).reshape(-1)
    if not 1 <= d <= 16 or np.any((a < 0) | (a >= 1 << d)):
        raise ValueError(f"addresses must lie in [0, 2^{d}), 1 <= d <= 16")
    return ((a[:, None] >> np.arange(d)[None, :]) & 1).astype(np.int32).reshape(-1)


def wfa_finals(values, theta=1, encode=None, N=1024):
    """Final weights of a layered automaton (thfhe_lhe_wfa): int32[n_states][N] from theta integer tables over the states
    (values[j][q] = f_j(q); with theta = 1 one table will do).  State q becomes the polynomial with f_j(q) at coefficient j < theta and zero
    elsewhere, so output j of the automaton carries f_j of the state it ends in.  encode: integers -> Torus32 words (e.g. lambda v:
    lut.encode(v, 8)); None: the values are the words."""
    if theta not in (1, 2, 4):
        raise ValueError("theta must be 1, 2 or 4")
    F = np.asarray(values, np.int64)
    if F.ndim == 1 and theta == 1:
        F = F[None]
    if F.ndim != 2 or F.shape[0] != theta or F.shape[1] < 1:
        raise ValueError(f"expected {theta} tables over the states, got shape {F.shape}")
    words = np.asarray(encode(F), np.int64) if encode is not None else F
    fin = np.zeros((F.shape[1], N), np.int64)
    fin[:, :theta] = words.T
    return _to_i32(fin)


def encrypt_table(rlwe_key, tv, sigma, rng, torus_bits=32):
    """The client side of an encrypted table (thfhe_lut_bootstrap_enc): a fresh TLWE sample (tv_a, tv_b) of the test vector(s) tv int32[..., N]
    under the bootstrapping ring key: tv_a uniform, tv_b = tv_a (*) z + tv + e, e Gaussian of standard deviation sigma; exact product.
    torus_bits=64 (thfhe_mk_lut_bootstrap_enc): int64 test vectors and samples, rlwe_key the small ring key the table is under -- on
    the 3-gen engine the summed key Z = sum_q z_q."""
    from .keygen import dtot32, dtot64, polymul_small32, polymul_small64
    _check_bits(torus_bits)
    if torus_bits == 64:
        z = np.asarray(rlwe_key, np.int64).reshape(-1)
        tv = np.ascontiguousarray(tv, np.int64)
        flat = tv.reshape(-1, z.shape[0])
        a = rng.integers(-2**63, 2**63, size=flat.shape, dtype=np.int64)
        b = polymul_small64(a, z).view(np.uint64) + flat.view(np.uint64) + dtot64(rng.standard_normal(flat.shape) * sigma).view(np.uint64)
        return a.reshape(tv.shape), b.view(np.int64).reshape(tv.shape)
    z = np.asarray(rlwe_key, np.int32).reshape(-1)
    tv = np.ascontiguousarray(tv, np.int32)
    flat = tv.reshape(-1, z.shape[0])
    a = rng.integers(-2**31, 2**31, size=flat.shape, dtype=np.int64).astype(np.int32)
    b = polymul_small32(a, z).astype(np.int64) + flat.astype(np.int64) + dtot32(rng.standard_normal(flat.shape) * sigma).astype(np.int64)
    return a.reshape(tv.shape), _to_i32(b).reshape(tv.shape)
