"""The definition of thfhe_mk_lhe_cmux / thfhe_mk_lhe_lookup in numpy, exact mod 2^64: the decomposition rule of the
batched N = 2048 rotation (v = D + offset; digit = ((v >> shift) & mask) - Bg/2, cut into balanced parts), the one-party 3-gen external product
on the set's own words, the CMux, the tree, the rotation chain and the extraction.

Negacyclic products run as float64 transforms of small integers: digit parts (|d| <= 2^9) against the set words cut into 8-bit limbs, the row
parts summed in the spectral domain.  A coefficient of such a sum is below 2 l parts N 2^9 2^8 = 2^31, the transform's rounding error some
2^-20 of a unit; every product asserts that what it rounds lies within 2^-8 of an integer, and tests/test_mk_lhe_host.py pins the product to
keygen.polymul_small64 and the whole CMux to the oracle's mk_mux_rotate."""
import numpy as np

import mk_lut_reference as MR

N = 2048
PART_INDEX = ((2, 1), (3, 0))   # mk_part_index(j, o): digit rows of polynomial j (0: mask, 1: body) meet part_{..+1} for output polynomial o


def part_index(j, o):
    return PART_INDEX[j][o]


def digit_parts(Bgbit):
    """(parts, pw) of launch_plan::mk_digit_parts."""
    parts = (Bgbit + 8) // 9 if Bgbit > 10 else 1
    return parts, ((Bgbit + parts - 1) // parts if parts > 1 else 0)


def decompose(D, l, Bgbit):
    """Digit rows of the Torus64 polynomials D int64[..., n]: int64[..., l * parts, n], row level * parts + part, low part first."""
    parts, pw = digit_parts(Bgbit)
    assert parts <= 2
    off = sum((1 << (Bgbit - 1)) << (64 - p * Bgbit) for p in range(1, l + 1)) & ((1 << 64) - 1)
    v = np.ascontiguousarray(D, np.int64).view(np.uint64) + np.uint64(off)
    rows = []
    for lv in range(l):
        dg = ((v >> np.uint64(64 - (lv + 1) * Bgbit)) & np.uint64((1 << Bgbit) - 1)).astype(np.int64) - (1 << (Bgbit - 1))
        if parts == 2:
            half = 1 << (pw - 1)
            lo = ((dg + half) & ((1 << pw) - 1)) - half
            rows += [lo, (dg - lo) >> pw]
        else:
            rows.append(dg)
    return np.stack(rows, axis=-2)


_twist = {}


def _tw(n):
    if n not in _twist:
        _twist[n] = np.exp(1j * np.pi * np.arange(n) / n)
    return _twist[n]


def _fwd(x):
    return np.fft.fft(np.asarray(x, np.float64) * _tw(x.shape[-1]), axis=-1)


def key_spectra(bit_words, l, Bgbit):
    """Spectra of one TGSW sample int64[4][l][n] as the product reads it: complex[row part][o][8 limbs][n], row part (j l + level) parts + part of
    output o being part_{part_index(j, o)}[level] shifted left by part * pw bits (wrapping)."""
    parts, pw = digit_parts(Bgbit)
    w = np.ascontiguousarray(bit_words, np.int64).view(np.uint64)
    rows = []
    for j in range(2):
        for lv in range(l):
            for part in range(parts):
                rows.append(np.stack([w[part_index(j, o), lv] << np.uint64(part * pw) for o in range(2)]))
    k = np.stack(rows)                                                                       # [RP][2][n]
    limbs = np.stack([((k >> np.uint64(8 * q)) & np.uint64(255)).astype(np.float64) for q in range(8)], axis=2)
    return _fwd(limbs)


def spectral_product(digits, kspec):
    """sum over the row parts of digits[..., rp, :] (*) key[rp][o] mod (X^n + 1, 2^64): int64[..., 2, n]."""
    n = digits.shape[-1]
    P = np.einsum("...rn,rokn->...okn", _fwd(digits), kspec)
    x = np.fft.ifft(P, axis=-1) * np.conj(_tw(n))
    r = np.rint(x.real)
    assert np.abs(x.real - r).max() < 2.0**-8 and np.abs(x.imag).max() < 2.0**-8, "the float64 product left the integers"
    r = r.astype(np.int64).view(np.uint64)
    out = np.zeros(r.shape[:-2] + (n,), np.uint64)
    for q in range(8):
        out += r[..., q, :] << np.uint64(8 * q)
    return out.view(np.int64)


def negacyclic(small, torus):
    """small (*) torus mod (X^n + 1, 2^64) for one polynomial each, through the same limbs: what keygen.polymul_small64 computes."""
    t = np.ascontiguousarray(torus, np.int64).view(np.uint64)
    limbs = np.stack([((t >> np.uint64(8 * q)) & np.uint64(255)).astype(np.float64) for q in range(8)])
    return spectral_product(np.asarray(small, np.int64)[None, :], _fwd(limbs)[None, None])[0]


class Set:
    """The words of a set int64[count][d][4][l][n] with the spectra of every (sample, bit), made on first use."""

    def __init__(self, words, d, l, Bgbit):
        w = np.ascontiguousarray(words, np.int64)
        self.n = w.shape[-1]
        self.words = w.reshape(-1, d, 4, l, self.n)
        self.count, self.d, self.l, self.Bgbit = self.words.shape[0], d, l, Bgbit
        self._spec = {}

    def spec(self, s, i):
        if (s, i) not in self._spec:
            self._spec[(s, i)] = key_spectra(self.words[s, i], self.l, self.Bgbit)
        return self._spec[(s, i)]


def extern(S, s, i, D):
    """C_(s,i) (.) D for samples D int64[..., 2, n] (mask, body): int64[..., 2, n]."""
    dg = decompose(D, S.l, S.Bgbit)                                    # [..., 2, l parts, n]
    dg = dg.reshape(dg.shape[:-3] + (-1, dg.shape[-1]))                # row part (j l + level) parts + part
    return spectral_product(dg, S.spec(s, i))


def _add(x, y):
    return (np.asarray(x, np.int64).view(np.uint64) + np.asarray(y, np.int64).view(np.uint64)).view(np.int64)


def _sub(x, y):
    return (np.asarray(x, np.int64).view(np.uint64) - np.asarray(y, np.int64).view(np.uint64)).view(np.int64)


def cmux(S, s, i, d1, d0):
    """d0 + C_(s,i) (.) (d1 - d0) on samples int64[..., 2, n]."""
    return _add(d0, extern(S, s, i, _sub(d1, d0)))


def monomial(acc, a):
    """X^a * acc mod X^n + 1 on int64[..., n], 0 <= a < 2n."""
    n = acc.shape[-1]
    e = (np.arange(n) - a) % (2 * n)
    v = np.asarray(acc, np.int64)[..., e % n]
    return np.where(e >= n, -v, v)


def tree(S, s, d_rot, polys):
    """The CMux tree over polys int64[2^d_tree][2][n]: level t pairs neighbours on bit d_rot + t."""
    t = 0
    while polys.shape[0] > 1:
        polys = cmux(S, s, d_rot + t, polys[1::2], polys[0::2])
        t += 1
    return polys[0]


def rotate_chain(S, s, d_rot, acc):
    """ACC += C_(s,i) (.) (X^(2n - box 2^i) ACC - ACC) for i < d_rot, box = n >> d_rot."""
    n = acc.shape[-1]
    box = n >> d_rot
    for i in range(d_rot):
        acc = cmux(S, s, i, monomial(acc, (2 * n - (box << i)) % (2 * n)), acc)
    return acc


def lookup_acc(S, s, d_tree, d_rot, tab_a, tab_b):
    """The accumulator of sample s on the table (tab_a, tab_b) int64[2^d_tree][n] (tab_a None: public) before the extraction: int64[2][n]."""
    tab_b = np.ascontiguousarray(tab_b, np.int64).reshape(1 << d_tree, -1)
    tab_a = np.zeros_like(tab_b) if tab_a is None else np.ascontiguousarray(tab_a, np.int64).reshape(tab_b.shape)
    return rotate_chain(S, s, d_rot, tree(S, s, d_rot, np.stack([tab_a, tab_b], axis=1)))


def lookup_wo_keyswitch(S, s, d_tree, d_rot, theta, tab_a, tab_b):
    """Reference of thfhe_mk_lhe_lookup_wo_keyswitch for sample s of the set: int32[theta][n+1]."""
    acc = lookup_acc(S, s, d_tree, d_rot, tab_a, tab_b)
    n = acc.shape[-1]
    return np.stack([MR.extract_at(acc.reshape(-1), j, n) for j in range(theta)])


def lookup(S, orc, s, d_tree, d_rot, theta, tab_a, tab_b):
    """... and of thfhe_mk_lhe_lookup: the context's key switch (MKOracle.keyswitch) of every record."""
    return np.stack([orc.keyswitch(r) for r in lookup_wo_keyswitch(S, s, d_tree, d_rot, theta, tab_a, tab_b)])
