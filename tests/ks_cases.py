"""The case table of the key-switch module's own tests (csrc/thfhe_keyswitch.h): shared by tests/test_ks_reference_host.py (CPU: the table
covers every compiled kernel instance) and tests/test_gpu_ks_*.py (GPU: every (case, count) against ks_reference and against the same engine
on another kernel).

ks_enqueue chooses among ks_plain_kernel<NX4, NX2> (12 row widths), ks_staged_kernel<W, R, SJ> (7 instances, spans of 64 or 128 coordinates)
and sk_keyswitch_mfma_kernel<T, ROT> (4 instances); every engine adds its own nsplit rule for the plain kernel.  That rule is restated here
ONCE, in route(), with the line it restates next to every constant; the host test reads the constants out of the sources' text and fails
when they move, so a changed threshold or an added instance cannot silently leave the GPU tests covering nothing.

Cost rules: key-switch keys are uniform int32 words of the key's shape with the crafted rows of craft_key() planted in them; bootstrapping
keys are zeros of the right shape (only the key switch runs, and any key is a valid input to it), except in the MUX cases, which go through
gates() and need real keys; no host key array exceeds KEY_CAP bytes, so every case picks t / basebit to fit (4-bit digits with t = 2 keep
n = 1407 at 173 MB).  Multi-key contexts override named sets so that the ring-side parameters stay valid.

CCS has no key-switch entry point of its own; its layout is the KMS one (one mask per party) at N = 1024, its nsplit rule is exercised by its
gate tests (tests/test_gpu_ccs.py), and the layout itself is checked against oracle_ccs_keyswitch on the CPU (test_ks_reference_host.py).

t basebit = 31 is reachable only as (31, 1): 31 is prime, and (1, 31) would need 2^31 - 1 key rows per coordinate.  The largest products
with wider digits are 30 ((6, 5), (15, 2), (10, 3): rounding offset 2)."""
from collections import namedtuple

import numpy as np

import ks_reference as R

KEY_CAP = 256 << 20   # bytes of a host key array

# ---- the launcher's rule, restated -----------------------------------------------------------------------------------------------------------
KS_MFMA_MIN = 512      # thfhe_keyswitch.h:45  kKsMfmaMinSamples
KS_STAGED_MIN = 192    # thfhe_keyswitch.h:46  kKsStagedMinSamples
PACK_MFMA_MIN = 8      # thfhe_threshold.hip:199  kPackMfmaMinSamples (passed as mfma_min at :223)
PLAIN_WIDTHS = (128, 256, 384, 512, 640, 768, 896, 1024, 1152, 1280, 1408, 2048)   # thfhe_keyswitch.h:552-554  THFHE_KS_CASE(W, ..): rows of 64 W words
STAGED = {  # thfhe_keyswitch.h:526-527 (eligible rows and digits) and :532-542 (the instance of each): (row words, basebit) -> (W, R, SJ)
    (512, 2): (8, 3, 4), (512, 3): (8, 7, 2), (640, 2): (10, 3, 4), (640, 3): (10, 7, 2), (768, 2): (12, 3, 2), (768, 3): (12, 7, 1),
    (1152, 2): (18, 3, 2),
}
STAGED_MAX_BITS = 16   # thfhe_keyswitch.h:527  a.t * a.basebit <= 16
SPAN128_MIN = 2048     # thfhe_keyswitch.h:525  the single key's 2-bit span: 64 below this many samples, 128 from it on
MFMA_T = (4, 8)        # thfhe_keyswitch.h:457 (single key, N = 1024) and :477 (packing key): planes for 2-bit digits, t = 4 or 8
MFMA_INSTANCES = {(4, 1), (4, 2), (8, 1), (8, 2)}   # thfhe_keyswitch.h:512-517  <T, ROT>
MAX_SLICE = 2048       # thfhe_keyswitch.h:87 / :547  sA[2048]: N / nsplit coordinates per workgroup of the plain kernel


def row_words(n):
    return 128 * ((n + 1 + 127) // 128)   # thfhe_keyswitch.h:449


def has_planes(engine, basebit, t, N):
    if engine == "pack":
        return basebit == 2 and t in MFMA_T              # thfhe_keyswitch.h:477
    return engine == "sk" and basebit == 2 and t in MFMA_T and N == 1024   # thfhe_keyswitch.h:457


def nsplit_plain(engine, samples, N):
    if engine == "sk":     # thfhe_sk.hip:655
        return 16 if samples <= 32 else 8 if samples <= 128 else 2 if samples <= 512 else 1
    if engine == "mk":     # thfhe_mk.hip:990
        return 16 if samples <= 64 else 4 if samples <= 256 else 2 if N > 2048 else 1
    if engine == "kms":    # thfhe_kms.hip:153
        return 8 if samples <= 64 else 2
    assert engine == "pack"
    return N // 64         # thfhe_threshold.hip:223  (N = the padded LWE dimension)


def mfma_nsplit(row, samples):
    """chunk ranges of the matrix-core kernel: doubled up to 8 until the grid has 1 024 workgroups (thfhe_keyswitch.h:507-509); 1 stores, the others
    accumulate into the zeroed output"""
    gtiles, wtiles, k = (samples + 255) // 256, row // 32, 1
    while k < 8 and gtiles * wtiles * k < 1024:
        k *= 2
    return k


def route(row, basebit, t, N, single, planes, samples, engine, rot=1):
    """the kernel ks_enqueue sends `samples` samples to: ("mfma", T, ROT), ("staged", W, R, SJ, span) or ("plain", row words, nsplit)"""
    if planes and samples >= (PACK_MFMA_MIN if engine == "pack" else KS_MFMA_MIN):   # thfhe_keyswitch.h:505
        return ("mfma", t, rot)
    span = 64 if basebit == 3 or (single and samples < SPAN128_MIN) else 128        # thfhe_keyswitch.h:525
    if (row, basebit) in STAGED and t * basebit <= STAGED_MAX_BITS and N % span == 0 and samples >= KS_STAGED_MIN:   # :526-528
        return ("staged",) + STAGED[(row, basebit)] + (span,)
    return ("plain", row, nsplit_plain(engine, samples, N))                          # thfhe_keyswitch.h:548-549


# ---- the cases -------------------------------------------------------------------------------------------------------------------------------
# engine: "sk" CloudKey.keyswitch | "mux" CloudKey.gates(MUX) (rot_per_gate = 2) | "mk" thfhe_mk_keyswitch_dev | "kms" KMSCloudKey.keyswitch |
# "pack" PackLwe(slots = 1).  base: the named set a multi-key context overrides.  counts: {samples: the kernel family the case claims for them}.
Case = namedtuple("Case", "id family engine n t basebit N parties base counts")


def _c(id, family, engine, n, t, basebit, counts, N=1024, parties=1, base=None):
    return Case(id, family, engine, n, t, basebit, N, parties, base, dict(counts))


def _all(kind, *counts):
    return {c: kind for c in counts}


P, S, M = "plain", "staged", "mfma"
CASES = []
# single key, every plain width (row words in the id) and the rows that exactly fill their padding (n + 1 = 128, 1024, 1408; n = 128 is the
# first past one): 4-bit digits are never staged and have no planes
for n in (100, 127, 128, 200, 300, 500, 630, 700, 800, 1000, 1023, 1024, 1200, 1407):
    CASES.append(_c("sk-w%d-n%d" % (row_words(n), n), "plain", "sk", n, 2, 4, _all(P, 9, 130)))
# ... the nsplit tiers (<= 32 / <= 128 / <= 512 / more) at two widths
for n in (100, 700):
    CASES.append(_c("sk-tiers-n%d" % n, "plain", "sk", n, 2, 4, _all(P, 1, 32, 33, 128, 129, 512, 513)))
# ... digit shapes: the limit t basebit = 31 (rounding offset 1), t = 1, wide digits with few levels, products of 30
for t, bb in ((31, 1), (1, 1), (1, 2), (6, 5), (3, 8), (15, 2), (10, 3)):
    CASES.append(_c("sk-digits-%dx%d" % (t, bb), "plain", "sk", 20, t, bb, _all(P, 5, 40, 200)))
# ... at least 192 samples that stay on the plain kernel: t basebit > 16, 4-bit digits, a row width without a staged instance
CASES.append(_c("sk-fallback-9x2", "plain", "sk", 500, 9, 2, _all(P, 200)))
CASES.append(_c("sk-fallback-2x4", "plain", "sk", 500, 2, 4, _all(P, 200)))
CASES.append(_c("sk-fallback-w896", "plain", "sk", 800, 5, 2, _all(P, 200)))
# single key, all seven staged instances with t = 5 (no planes; a stage of SJ pairs straddles coordinates): the threshold and a ragged last
# workgroup of 32; one 2-bit case also crosses span 64 -> 128
for n, bb in ((500, 2), (500, 3), (630, 2), (630, 3), (700, 2), (700, 3), (1100, 2)):
    counts = {191: P, 192: S, 193: S}
    if (n, bb) == (500, 2):
        counts.update({2047: S, 2048: S})
    CASES.append(_c("sk-staged-w%d-5x%d" % (row_words(n), bb), "staged", "sk", n, 5, bb, counts))
for t, bb in ((1, 2), (3, 2), (7, 2), (1, 3), (2, 3)):
    CASES.append(_c("sk-staged-w512-%dx%d" % (t, bb), "staged", "sk", 500, t, bb, {192: S, 193: S}))
# single key on the matrix cores: 4 word tiles .. 44, rows that fill their padding, a last tile that holds just the b column (n = 800: 25 x 32)
for t in (4, 8):
    for n in (100, 127, 128, 800, 1023, 1407):
        CASES.append(_c("sk-mfma-n%d-%dx2" % (n, t), "mfma", "sk", n, t, 2, {511: P, 512: M, 513: M, 769: M, 1024: M}))
# ... its chunk ranges: 4, 2 and 1 (a plain store into an output that was not zeroed) need 256 and more tiles, i.e. 44 word tiles and thousands
# of samples; 6 145 samples make a grid that is no multiple of 8, which the renumbering of the workgroups over the XCDs leaves as it is
CASES.append(_c("sk-mfma-ranges-n1407-4x2", "mfma", "sk", 1407, 4, 2, _all(M, 1500, 3000, 6000, 6145)))
# MUX (rot_per_gate = 2) through gates(): the 512-word plain instance and the staged <8, 7, 2>; the two ROT = 2 matrix-core instances
CASES.append(_c("mux-n500-5x3", "mux", "mux", 500, 5, 3, {24: P, 200: S}))
for t in (4, 8):
    CASES.append(_c("mux-n100-%dx2" % t, "mux", "mux", 100, t, 2, {513: M}))
# 3-gen: one mask for all parties.  Widths 256 / 384 / 768 with 2 .. 5 parties, party blocks off the 16-byte alignment (n = 130, 131), the
# three ring degrees, the nsplit tiers 64 / 256; N = 2048 above 256 samples is a 2048-word slice (nsplit = 1), N = 4096 runs nsplit = 2
CASES.append(_c("mk-w256-p5", "layouts", "mk", 255, 5, 2, _all(P, 64, 65, 256, 257), parties=5, base="MK3"))
CASES.append(_c("mk-w384-p3", "layouts", "mk", 383, 3, 3, _all(P, 64, 65, 256, 257), parties=3, base="MK3"))
CASES.append(_c("mk-w768-p2", "layouts", "mk", 767, 5, 2, {64: P, 65: P, 191: P, 192: S, 257: S}, parties=2, base="MK3"))
CASES.append(_c("mk-n130-p3", "layouts", "mk", 130, 4, 2, _all(P, 5, 65), parties=3, base="MK3"))
CASES.append(_c("mk-n131-p4", "layouts", "mk", 131, 2, 3, _all(P, 5, 65), parties=4, base="MK3"))
CASES.append(_c("mk-N2048-w256", "layouts", "mk", 255, 2, 4, _all(P, 256, 257, 300), N=2048, parties=2, base="MK16"))
CASES.append(_c("mk-N4096-w256", "layouts", "mk", 255, 2, 3, _all(P, 64, 256, 257), N=4096, parties=2, base="MK64-fft"))
CASES.append(_c("mk-N4096-staged", "layouts", "mk", 500, 1, 3, {192: S, 200: S}, N=4096, parties=2, base="MK64-fft"))   # 64 coordinate ranges
# KMS: one mask per party, N = 2048.  (Rows of 512 words with three parties or ks 5/3 pass KEY_CAP: two parties, ks 3/3 and 5/2 there.)
CASES.append(_c("kms-w384-p3-8x2", "layouts", "kms", 383, 8, 2, _all(P, 64, 65, 191, 192, 225), N=2048, parties=3, base="KMS2"))
CASES.append(_c("kms-w512-p2-3x3", "layouts", "kms", 500, 3, 3, {64: P, 65: P, 191: P, 192: S, 225: S}, N=2048, parties=2, base="KMS2"))
CASES.append(_c("kms-w512-p2-5x2", "layouts", "kms", 500, 5, 2, {64: P, 65: P, 191: P, 192: S, 225: S}, N=2048, parties=2, base="KMS2"))
# the packing key: LWE dimensions at the coordinate padding's edge (N = the padded dimension: 128, 128, 256)
for n in (127, 128, 129):
    CASES.append(_c("pack-n%d-5x3" % n, "layouts", "pack", n, 5, 3, _all(P, 1, 7)))
    for t in (4, 8):
        CASES.append(_c("pack-n%d-%dx2" % (n, t), "layouts", "pack", n, t, 2, {7: P, 8: M, 300: M}))

BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)


def family(name):
    return [c for c in CASES if c.family == name]


def case_route(c, samples):
    """route() with the arguments KsKey / KsArgs hold for the case"""
    if c.engine == "pack":   # upload_pack (thfhe_keyswitch.h:467-481): rows of 2 N_ring words, coordinates padded to a multiple of 128
        N = 128 * ((c.n + 127) // 128)
        return route(2048, c.basebit, c.t, N, True, has_planes("pack", c.basebit, c.t, N), samples, "pack")
    eng = "sk" if c.engine == "mux" else c.engine
    return route(row_words(c.n), c.basebit, c.t, c.N, eng == "sk", has_planes(eng, c.basebit, c.t, c.N), samples, eng, 2 if c.engine == "mux" else 1)


def key_shape(c):
    rows = (1 << c.basebit) - 1
    if c.engine == "pack":
        return (c.n, c.t, rows, 2, 1024)
    return (c.parties, c.N, c.t, rows, c.n + 1)


def key_bytes(c):
    return 4 * int(np.prod(key_shape(c), dtype=np.int64))


def rec_words(c):
    return c.n + 1 if c.engine == "pack" else (c.parties * c.N + 1 if c.engine == "kms" else c.N + 1)


# ---- crafted data --------------------------------------------------------------------------------------------------------------------------
# key rows that drive the balanced-byte split of the matrix-core planes through its carry chains; the sums over N t such rows wrap
KEY_WORDS = (0x7F7F7F80, 0x80808080, 0xFFFFFF80, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF)
N_CRAFTED = 7


def random_words(rng, shape):
    return np.frombuffer(rng.bytes(4 * int(np.prod(shape, dtype=np.int64))), np.int32).reshape(shape).copy()


def craft_key(K):
    """plant the crafted rows in K [.., coordinates, t, rows, row]: two coordinates per word of KEY_WORDS, from coordinate 5 on and again at the
    end of the coordinates (another coordinate range of every kernel); every level, digit value and party"""
    coords = K.shape[-4]
    Ku = K.view(np.uint32)
    for q, w in enumerate(KEY_WORDS):
        for lo in (5, coords - 2 * len(KEY_WORDS)):
            if 0 <= lo and lo + 2 * len(KEY_WORDS) <= coords:
                Ku[..., lo + 2 * q:lo + 2 * q + 2, :, :, :] = w
    return K


def make_key(c, seed=0x4B53):
    shape = key_shape(c)
    K = random_words(np.random.default_rng(seed + c.n), shape)
    return craft_key(K.reshape(1, c.n, c.t, shape[2], 2048) if c.engine == "pack" else K).reshape(shape)


def crafted_positions(count):
    """rows of a batch that hold the crafted records: spread over the first and the last workgroup from 64 samples on"""
    if count >= 64:
        return [0, 1, 2, count // 2, count - 3, count - 2, count - 1]
    return list(range(min(count, N_CRAFTED)))


def make_inputs(c, count, seed):
    """int32[count][rec]: uniform words with the crafted records planted: all zero, all -1, 0x7FFFFFFF, 0x80000000, every mask word -offset
    (the rounding offset carries through every digit and wraps: all digits zero), -offset - 1 (all digits maximal), and the two alternating.
    The shortest batches take the last records first."""
    off = R.prec_offset(c.t, c.basebit)
    u = random_words(np.random.default_rng(seed), (count, rec_words(c)))
    uu = u.view(np.uint32)
    alt = np.where(np.arange(rec_words(c)) % 2 == 0, (-off) & 0xFFFFFFFF, (-off - 1) & 0xFFFFFFFF).astype(np.uint32)
    rows = [0, 0xFFFFFFFF, 0x7FFFFFFF, 0x80000000, (-off) & 0xFFFFFFFF, (-off - 1) & 0xFFFFFFFF, alt]
    pos = crafted_positions(count)
    for k, g in enumerate(pos):
        uu[g, :] = rows[N_CRAFTED - len(pos) + k]
    return u


def check_rows(c, count, rt):
    """the rows compared with ks_reference: the crafted rows, the first and last row of the first and last workgroup / tile (32 samples for
    the staged kernel, 256 and 32 for the matrix cores) and a stride through the rest; every row where n <= 128"""
    if c.n <= 128 or count <= 16:
        return list(range(count))
    rows = set(crafted_positions(count))
    for tile in ((256, 32) if rt[0] == "mfma" else (32,)):
        last = tile * ((count - 1) // tile)
        rows |= {0, min(tile - 1, count - 1), last, max(last - 1, 0), count - 1}
    rows |= set(range(3, count, max(1, count // 6)))
    return sorted(rows)


def piece_size(c, rt):
    """batches of this size run the same records on another kernel: the plain kernel for matrix-core and staged batches (<= 128 samples;
    the packing key: below its threshold), the plain kernel with nsplit = 16 (KMS: 8) for plain batches"""
    if c.engine == "pack":
        return PACK_MFMA_MIN - 1 if rt[0] == "mfma" else None
    return 128 if rt[0] != "plain" else 32


def reference(c, K, u, rows):
    if c.engine == "pack":
        return R.pack_keyswitch(u, K, c.t, c.basebit, rows)
    return R.keyswitch(u, K, c.t, c.basebit, u_pstride=c.N if c.engine == "kms" else 0, rows=rows)


# ---- running a case on the GPU (thfhe is imported here, not at module level: the host test imports this module without the HIP library) -------
class Runner:
    """the case's context and `run(u) -> int32[count][output record]`; closed by close()"""

    def __init__(self, c, K):
        import thfhe
        self.c, self.keep = c, []
        if c.engine == "sk":
            p = thfhe.make_params(n=c.n, N=1024, k=1, l=1, Bgbit=8, ks_t=c.t, ks_basebit=c.basebit, torus_bits=32, parties=1)
            self.ctx = thfhe.CloudKey(p, np.zeros((c.n, 2, 2, 1024), np.int32), K, device=0)
            self.run, self.out_words = self.ctx.keyswitch, c.n + 1
        elif c.engine == "mk":
            p = thfhe.make_params(c.base, n=c.n, parties=c.parties, ks_t=c.t, ks_basebit=c.basebit)
            assert p.N == c.N
            self.ctx = thfhe.MKCloudKey(p, np.zeros((c.parties, c.n, 4, p.l, p.N), np.int64), K, device=0)
            self.run, self.out_words = self._mk, c.parties * c.n + 1
        elif c.engine == "kms":
            from thfhe import kms
            p = thfhe.make_kms_params(c.base, n=c.n, parties=c.parties, l_gsw=1, bg_gsw=8, l_uni=1, ks_t=c.t, ks_basebit=c.basebit)
            assert p.N == c.N
            z = lambda *s: np.zeros(s, np.int64)
            self.ctx = kms.KMSCloudKey(p, z(c.parties, c.n, 2, 2, p.N), z(c.parties, 3, 1, p.N), z(c.parties, 1, p.N), z(1, p.N), K, device=0)
            self.run, self.out_words = self.ctx.keyswitch, c.parties * c.n + 1
        else:
            assert c.engine == "pack"
            from thfhe import threshold as T
            self.ctx = T.PolyContext(0)
            self.ctx.set_pack_key(K, c.t, c.basebit)
            self.run, self.out_words = self._pack, 2048

    def _mk(self, u):
        import thfhe
        count = u.shape[0]
        out = np.empty((count, self.out_words), np.int32)
        if count == 0:
            return out
        du = thfhe.DeviceBuffer(self.ctx, u.nbytes).upload(np.ascontiguousarray(u))
        do = thfhe.DeviceBuffer(self.ctx, out.nbytes)
        try:
            thfhe._check(thfhe.lib().thfhe_mk_keyswitch_dev(self.ctx.h, du.ptr, do.ptr, count))
            self.ctx.sync()
            return do.download(out.shape)
        finally:
            du.free()
            do.free()

    def _pack(self, x):
        from thfhe import threshold as T
        return np.concatenate(T.PackLwe(self.ctx, x, slots=1), axis=1)   # one sample per output: (alpha, beta) = the key switch's record

    def close(self):
        self.ctx.close()


def check_case(c, seed=0):
    """every count of the case: shape, determinism, every output row against the same engine on another kernel, rows against ks_reference"""
    from support import differing
    K = make_key(c)
    r = Runner(c, K)
    try:
        empty = r.run(np.zeros((0, rec_words(c)), np.int32))
        assert empty.shape == (0, r.out_words) and empty.dtype == np.int32
        for count in c.counts:
            rt = case_route(c, count)
            u = make_inputs(c, count, 1000 * seed + count)
            got = r.run(u)
            assert got.shape == (count, r.out_words), (c.id, count)
            assert np.array_equal(r.run(u), got), (c.id, count, "second call differs")
            rows = check_rows(c, count, rt)
            assert len(rows) >= min(count, N_CRAFTED + 4) and set(crafted_positions(count)) <= set(rows)
            ref = reference(c, K, u, rows)
            assert np.array_equal(got[rows], ref), (c.id, count, rt, [[rows[g], w] for g, w in differing(got[rows], ref)])
            piece = piece_size(c, rt)
            if piece and count > piece and case_route(c, piece) != rt:
                other = np.concatenate([r.run(u[q:q + piece]) for q in range(0, count, piece)])
                assert np.array_equal(got, other), (c.id, count, rt, differing(got, other))
    finally:
        r.close()
