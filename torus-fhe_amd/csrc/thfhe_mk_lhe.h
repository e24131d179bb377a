// thfhe_mk_lhe.h -- leveled CMux and table lookup on the Torus64 ring of degree 2048: kernels, launcher, the set's fill and this
// engine's adaptors over the call bodies of thfhe_lhe_host.h for thfhe_mk_tgsw_set_create, thfhe_mk_lhe_cmux and
// thfhe_mk_lhe_lookup(_wo_keyswitch).  Included by thfhe_mk.hip INSIDE its second anonymous
// namespace, after thfhe_mk_ctx and mk_keyswitch: the contexts are the one-party sets on the batched rotation path (thfhe_rot2k.h), whose external
// product is the ordinary TGSW (.) TLWE product (J/tgsw_3gen.jl:102-113).  A set keeps the spectra of count x d TGSW samples in the layout of that
// path's key table with (sample d + bit) in the place of the key index, so a job's key chunks are chunk(step, rp, half) of kms_tlev_rotate_kernel
// behind a per-job base.  Both kernels are that kernel's step (row parts through the LDS in batches of six, half spectra S0 / S1, LDS atomics)
// on other digits: X^a ACC - ACC with public amounts, or d1 - ACC with d1 read from global memory where the digits are cut.  The transforms are
// the table-free twisted halves of the one-pass kernels (wave_fft_*_tq_two): no T1 table in the LDS, 128 KiB per workgroup.
#pragma once

constexpr int kMkLheN = 2048, kMkLheMaxRot = 11;   // ring degree and its log2

struct MkLheDigits {
    int lg, bg, parts, lo_bits;
};

// One CMux ACC += C (.) D on the accumulator sAcc (int64[2][2048] in LDS), C's spectra at `key` ([row part][o][h][half][512]).
//   ROT:  D = X^a2n ACC - ACC;  else D = d1 - ACC, polynomial j of d1 at d1[j] in global memory (null: zero).
// The body of kms_tlev_rotate_kernel's step (thfhe_rot2k.h): entered and left with the workgroup in step.
template <bool ROT>
__device__ __forceinline__ void mk_lhe_step(int wave, int lane, const MkLheDigits &g, int64_t *sAcc, cplx *sSpec, const cplx *tw,
                                            const cplx *key, int a2n, const int64_t *const (&d1)[2]) {
    constexpr int BATCH = 6;  // row parts whose spectra sit in the LDS at the same time (16 KiB each)
    const int lg = g.lg, bg = g.bg, parts = g.parts, lo_bits = g.lo_bits;
    const int RP = 2 * lg * parts;
    uint64_t offset = 0;
    for (int p = 1; p <= lg; p++) offset += (1ull << (bg - 1)) << (64 - p * bg);
    const int o = wave >> 2, h = wave & 3;
    unsigned long long *accu = reinterpret_cast<unsigned long long *>(sAcc) + o * 2048;
    auto chunk = [&](int rp, int half) { return key + (((((size_t)rp) * 2 + o) * 4 + h) * 2 + half) * 512; };
    cplx S0[8], S1[8];
#pragma unroll
    for (int m = 0; m < 8; m++) S0[m] = S1[m] = cplx{0.0, 0.0};
    for (int b0 = 0; b0 < RP; b0 += BATCH) {
        const int nb = RP - b0 < BATCH ? RP - b0 : BATCH;
        if (wave < nb) {
            const int rp = b0 + wave, r = rp / parts, part = rp % parts;
            const int64_t *ap = sAcc + (r / lg) * 2048;
            const int64_t *dp = d1[r / lg];   // uniform over the wave
            const int shift = 64 - ((r % lg) + 1) * bg;
            const uint64_t mask = (1ull << bg) - 1ull;
            const int32_t half_bg = 1 << (bg - 1), half_lo = 1 << (lo_bits - 1), mask_lo = (1 << lo_bits) - 1;
            constexpr double R = 0.70710678118654752440;
            cplx y0[8], y1[8];
            int a2n_b = a2n;
            asm volatile("" : "+s"(a2n_b));   // opaque per batch, as in kms_tlev_rotate_kernel
#pragma unroll
            for (int m = 0; m < 8; m++) {
                uint64_t x[4] = {0, 0, 0, 0};
                if (!ROT && dp) {
#pragma unroll
                    for (int q = 0; q < 4; q++) x[q] = (uint64_t)dp[lane + 64 * m + 512 * q];
                }
                double d[4];
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const int c = lane + 64 * m + 512 * q;
                    const uint64_t v = (ROT ? rot_minus_self64_n<2048>(ap, c, a2n_b) : x[q] - (uint64_t)ap[c]) + offset;
                    int32_t dg = (int32_t)((v >> shift) & mask) - half_bg;                     // decompose, J/tgsw.jl:112-138 (64-bit words)
                    if (parts == 2) {
                        const int32_t lo = ((dg + half_lo) & mask_lo) - half_lo;               // balanced low part
                        dg = part ? (dg - lo) >> lo_bits : lo;
                    }
                    d[q] = (double)dg;
                }
                const cplx w{(d[1] - d[3]) * R, (d[1] + d[3]) * R};
                y0[m] = cplx{d[0] + w.re, d[2] + w.im};
                y1[m] = cplx{d[0] - w.re, d[2] - w.im};
                if (m & 1) kms_pin();   // at most 8 of the 32 64-bit reads in flight
            }
            cplx *xb = sSpec + wave * 1024;
            // the table-free twisted transforms of the one-pass kernels, both halves side by side inside the row part's own, not yet published, slot.
            // The lane index and the per-lane constants are formed here (L1 / L2 hits), not carried across the multiply
            const int ln = opaque_lane(lane);
            const W64 w64{tw[TwRing2k::T2 + 1 * 8 + (ln & 7)]};
            const LaneRoots r1{opaque_cplx(tw[TwRing2k::T1_TWIST1 + ln]), opaque_cplx(tw[TwRing2k::RATIO + ln])};
            const LaneRoots r5{opaque_cplx(tw[TwRing2k::T1_TWIST5 + ln]), opaque_cplx(tw[TwRing2k::RATIO + ln])};
            wave_fft_fwd_tq_two<1, 5>(ln, y0, y1, xb, xb + 512, r1, r5, w64);
            wave_sync();
#pragma unroll
            for (int m = 0; m < 8; m++) {
                xb[m * 64 + lane] = y0[m];
                xb[512 + m * 64 + lane] = y1[m];
            }
        }
        cplx bA[8], bB[8];
        load8(lane, bA, chunk(b0, 0));
        load8(lane, bB, chunk(b0, 1));
        __syncthreads();  // this batch's spectra published (and, for the first batch, every read of the accumulator done)
        for (int q = 0; q < nb; q++) {
            const int rp = b0 + q;
            const int rn = q + 1 < nb ? rp + 1 : rp;   // the last row part of a batch re-requests itself (unconditional loads)
            cplx z[8];
#pragma unroll
            for (int m = 0; m < 8; m++) z[m] = sSpec[q * 1024 + m * 64 + lane];
            mac8r(S0, z, bA);
            kms_pin();
            load8(lane, bA, chunk(rn, 0));
            kms_pin();
#pragma unroll
            for (int m = 0; m < 8; m++) z[m] = sSpec[q * 1024 + 512 + m * 64 + lane];
            mac8r(S1, z, bB);
            kms_pin();
            load8(lane, bB, chunk(rn, 1));
            kms_pin();
        }
        __syncthreads();  // spectra consumed: the area is free for the next batch / the inverse transforms
    }
    {
        cplx *xb = sSpec + wave * 512;
        const int ln = opaque_lane(lane);
        const W64 w64{tw[TwRing2k::T2 + 1 * 8 + (ln & 7)]};
        const LaneRoots r1{opaque_cplx(tw[TwRing2k::T1_TWIST1 + ln]), opaque_cplx(tw[TwRing2k::RATIO + ln])};
        const LaneRoots r5{opaque_cplx(tw[TwRing2k::T1_TWIST5 + ln]), opaque_cplx(tw[TwRing2k::RATIO + ln])};
        wave_fft_inv_tq_two<1, 5>(ln, S0, S1, xb, r1, r5, w64);
        cplx lo[8], hi[8];
        merge2048(S0, S1, lo, hi);
#pragma unroll
        for (int m = 0; m < 8; m++) {
            const int q = ln + 64 * m;
            atomicAdd(accu + q, (unsigned long long)round_i64(lo[m].re) << (16 * h));
            atomicAdd(accu + q + 512, (unsigned long long)round_i64(hi[m].re) << (16 * h));
            atomicAdd(accu + q + 1024, (unsigned long long)round_i64(lo[m].im) << (16 * h));
            atomicAdd(accu + q + 1536, (unsigned long long)round_i64(hi[m].im) << (16 * h));
        }
    }
    __syncthreads();  // accumulator updated and scratch free
}

// the rotation chain of one sample: ACC += C_(s,i) (.) (X^(2N - box 2^i) ACC - ACC) for i = 0 .. d_rot-1, from a given accumulator
struct MkLheRotArgs {
    const cplx *spec;            // the spectra at the launch's first sample
    const cplx *tw;
    const int64_t *src_a, *src_b;   // the starting samples; src_a null: trivial samples (0, src_b)
    const int32_t *src_idx;      // null: sample s starts from s * src_stride, else from src_idx[s] * src_stride
    size_t src_stride;           // words
    int64_t *acc_out;            // [samples][2][2048] for mk_extract_at_kernel
    size_t step_stride;          // complex slots of one bit's spectra (row parts x 8192)
    int d, d_rot, box;
    MkLheDigits g;
};
__global__ __launch_bounds__(512, 2) void mk_lhe_rotate2k_kernel(MkLheRotArgs a) {
    __shared__ int64_t sAcc[4096];
    __shared__ cplx sSpec[6 * 1024];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const size_t s = blockIdx.x;
    const size_t in = (a.src_idx ? (size_t)a.src_idx[s] : s) * a.src_stride;
    for (int q = threadIdx.x; q < 2048; q += 512) {
        sAcc[q] = a.src_a ? a.src_a[in + q] : 0;
        sAcc[2048 + q] = a.src_b[in + q];
    }
    __syncthreads();
    const int64_t *const none[2] = {nullptr, nullptr};
    for (int i = 0; i < a.d_rot; i++) {
        const int a2n = (4096 - (a.box << i)) & 4095;   // public and uniform over the launch
        mk_lhe_step<true>(wave, lane, a.g, sAcc, sSpec, a.tw, a.spec + (s * a.d + i) * a.step_stride, a2n, none);
    }
    for (int q = opaque_lane(wave * 64 + lane); q < 4096; q += 512) a.acc_out   // not threadIdx.x: that register would be carried across the chain
       [s * 4096 + q] = sAcc[q];
}

// one CMux between two samples: out = d0 + C_(s,bit) (.) (d1 - d0); grid (pairs, samples).  Pair p of sample s reads d0 / d1 at
// index(s) * in_sample + p * in_pair words (index(s) = in_idx[s] or s) and writes at s * out_sample + p * out_pair; out may be d0's own slot.
struct MkLheCmuxArgs {
    const cplx *spec;
    const cplx *tw;
    const int64_t *d0_a, *d0_b, *d1_a, *d1_b;   // d0_a / d1_a null: trivial samples
    int64_t *out_a, *out_b;
    const int32_t *in_idx;
    size_t in_sample, in_pair, out_sample, out_pair;
    size_t step_stride;
    int d, bit;
    MkLheDigits g;
};
__global__ __launch_bounds__(512, 2) void mk_lhe_cmux2k_kernel(MkLheCmuxArgs a) {
    __shared__ int64_t sAcc[4096];
    __shared__ cplx sSpec[6 * 1024];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const size_t s = blockIdx.y, p = blockIdx.x;
    const size_t in = (a.in_idx ? (size_t)a.in_idx[s] : s) * a.in_sample + p * a.in_pair;
    const size_t out = s * a.out_sample + p * a.out_pair;
    for (int q = threadIdx.x; q < 2048; q += 512) {
        sAcc[q] = a.d0_a ? a.d0_a[in + q] : 0;
        sAcc[2048 + q] = a.d0_b[in + q];
    }
    __syncthreads();
    const int64_t *const d1[2] = {a.d1_a ? a.d1_a + in : nullptr, a.d1_b + in};
    mk_lhe_step<false>(wave, lane, a.g, sAcc, sSpec, a.tw, a.spec + (s * a.d + a.bit) * a.step_stride, 0, d1);
    for (int q = opaque_lane(wave * 64 + lane); q < 2048; q += 512) {   // addresses formed here, not carried across the step
        a.out_a[out + q] = sAcc[q];
        a.out_b[out + q] = sAcc[2048 + q];
    }
}

inline MkLheDigits mk_lhe_digits(const thfhe_mk_ctx *c) { return MkLheDigits{c->p.l, c->p.Bgbit, c->parts, c->pw}; }
// complex slots of one bit's spectra ([row part][o][h][half][512]) and of one sample of a set
inline size_t mk_lhe_bit_slots(const thfhe_mk_ctx *c) { return (size_t)2 * c->p.l * c->parts * 8192; }
inline size_t mk_lhe_sample_slots(const thfhe_mk_ctx *c, int d) { return (size_t)d * mk_lhe_bit_slots(c); }

// the contexts the leveled calls run on: one party, N = 2048, the batched rotation path (the CB sets)
int mk_lhe_ctx_check(const thfhe_mk_ctx *c) {
    if (c->p.parties != 1) return thfhe_fail(THFHE_E_UNSUPPORTED, "mk lhe: the context must have parties = 1 (the 3-gen product of one party is TGSW (.) TLWE)");
    if (c->p.N != kMkLheN) return thfhe_fail(THFHE_E_UNSUPPORTED, "mk lhe: the context must be on the ring of degree N = 2048");
    if (!c->batched) return thfhe_fail(THFHE_E_UNSUPPORTED, "mk lhe: the context must be on the batched rotation path (l x digit parts > 3, the CB sets)");
    return THFHE_OK;
}

// thfhe_mk_tgsw_set_create after its host checks: the size check, then stage_party_keys with the samples as parties and the bits as key indices
int mk_tgsw_set_fill(thfhe_mk_ctx *c, thfhe_mk_tgsw_set *set, const int64_t *tgsw) {
    DevLock lk(*c);
    if (lk.rc) return lk.rc;
    THFHE_TRY(mk_lhe_ctx_check(c));
    const int l = c->p.l, d = set->d;
    const size_t bytes = set->count * mk_lhe_sample_slots(c, d) * sizeof(cplx);                            // count d row parts 128 KiB
    const size_t stage_bytes = (size_t)d * 2 * l * c->parts * 2 * kMkLheN * sizeof(int64_t);               // one sample's polynomials
    size_t free_b = 0, total_b = 0;
    THFHE_HIP(hipMemGetInfo(&free_b, &total_b));
    if (bytes + stage_bytes > free_b) return thfhe_fail(THFHE_E_NOMEM, "mk tgsw set: count d row parts 128 KiB of spectra exceed the free device memory");
    auto src = [&](int q, int i, int r, int o) { return tgsw + ((((size_t)q * d + i) * 4 + mk_part_index(r / l, o)) * l + r % l) * kMkLheN; };
    return stage_party_keys<2048>(*c, set->spec, (int)set->count, d, 2 * l, c->parts, c->pw, src);   // a slice per sample
}

int mk_launch_lhe_cmux(thfhe_mk_ctx *c, const MkLheCmuxArgs &a, size_t pairs, size_t samples) {
    hipLaunchKernelGGL(mk_lhe_cmux2k_kernel, dim3((unsigned)pairs, (unsigned)samples), dim3(512), 0, c->stream, a);
    THFHE_HIP(hipGetLastError());
    return THFHE_OK;
}

// what the shared leveled bodies (thfhe_lhe_host.h) admit on this engine: N = 2048, up to 4 096 samples per launch of the flat CMux
constexpr LheRules<thfhe_mk_ctx> kMkLheRules{
    kMkLheN, kMkLheMaxRot, 4096, mk_lhe_sample_slots,   // N, d_rot_max, cmux_slice, sample_slots
    "mk tgsw set: d must be 1 .. 16",                                  // set_d_text
    "mk tgsw set: count must be 1 .. 2^24",                            // set_count_text
    "mk lhe: samples first .. first+count-1 are not all in the set",   // range_text
    "mk lhe: the set belongs to another context",                      // ctx_text
    "mk lhe_cmux: bit must be 0 .. d-1",                               // bit_text
    "mk lhe_lookup: d_tree must be 0 .. 6",                            // d_tree_text
    "mk lhe_lookup: d_rot must be 0 .. 11",                            // d_rot_text
    "mk lhe_lookup: theta must be 1, 2 or 4",                          // theta_text
    "mk lhe_lookup: theta must not exceed box = N >> d_rot",           // box_text
    "mk lhe_lookup: n_tables 2^d_tree must be 1 .. 262144",            // n_tables_text
    "mk lhe_lookup: d_tree + d_rot must equal the set's d"};           // d_sum_text

// a CMux launch of the shared bodies on mk_lhe_cmux2k_kernel, over a set of d bits; io.pub is not looked at: a null mask already means a
// trivial sample here
int mk_lhe_cmux_level(thfhe_mk_ctx *c, int d, const LheCmuxIo<int64_t> &io, size_t pairs, size_t S) {
    const MkLheCmuxArgs a{io.spec, c->d_tw.as<cplx>(), io.d0_a, io.d0_b, io.d1_a, io.d1_b, io.out_a, io.out_b, io.in_idx,
                          io.in_sample, io.in_pair, io.out_sample, io.out_pair, mk_lhe_bit_slots(c), d, io.bit, mk_lhe_digits(c)};
    return mk_launch_lhe_cmux(c, a, pairs, S);
}

// thfhe_mk_lhe_cmux: ctx_lhe_cmux (thfhe_lhe_host.h) on this engine's launch
int mk_lhe_cmux(thfhe_mk_ctx *c, const thfhe_mk_tgsw_set *set, int bit, const int64_t *d1_a, const int64_t *d1_b, const int64_t *d0_a, const int64_t *d0_b,
                int64_t *out_a, int64_t *out_b, size_t count) {
    return ctx_lhe_cmux(c, set, bit, d1_a, d1_b, d0_a, d0_b, out_a, out_b, count, kMkLheRules,
                        [&](const LheCmuxIo<int64_t> &io, size_t S) { return mk_lhe_cmux_level(c, set->d, io, 1, S); });
}

// The launch chain of a leveled lookup over S samples: ctx_enqueue_lhe_lookup (thfhe_lhe_host.h) on mk_lhe_cmux2k_kernel, the rotation chain
// into d_acc with the extraction of theta coefficients into d_u, and the context's key switch.  d: the bits of the set the spectra belong to.
// The caller has sized d_acc too.
int mk_enqueue_lhe_lookup(thfhe_mk_ctx *c, const cplx *spec, int d, size_t S, int d_tree, int d_rot, int theta, const int64_t *t_a, const int64_t *t_b,
                          const int32_t *idx, size_t tab_stride, int32_t *ks_out, bool prof) {
    return ctx_enqueue_lhe_lookup(
        c, spec, S, d_tree, d_rot, theta, t_a, t_b, idx, tab_stride, ks_out, prof, kMkLheRules,
        [&](const LheCmuxIo<int64_t> &io, size_t pairs) { return mk_lhe_cmux_level(c, d, io, pairs, S); },
        [&](const int64_t *src_a, const int64_t *src_b, const int32_t *src_idx, size_t src_stride) {
            int64_t *const acc = c->d_acc.as<int64_t>();
            const MkLheRotArgs r{spec, c->d_tw.as<cplx>(), src_a, src_b, src_idx, src_stride, acc, mk_lhe_bit_slots(c), d, d_rot, kMkLheN >> d_rot, mk_lhe_digits(c)};
            hipLaunchKernelGGL(mk_lhe_rotate2k_kernel, dim3((unsigned)S), dim3(512), 0, c->stream, r);
            hipLaunchKernelGGL(mk_extract_at_kernel, dim3((unsigned)S, (unsigned)theta), dim3(256), 0, c->stream, (const int64_t *)acc, c->d_u.as<int32_t>(), (long)S,
                               kMkLheN, theta);
            THFHE_HIP(hipGetLastError());
            return (int)THFHE_OK;
        },
        [&](int32_t *out, size_t records) { return mk_keyswitch(c, c->d_u.as<int32_t>(), out, records); });
}

// thfhe_mk_lhe_lookup (keyswitch) / thfhe_mk_lhe_lookup_wo_keyswitch: ctx_lhe_lookup (thfhe_lhe_host.h) on this engine's chain and its
// accumulators; the tree workspace is 2^(d_tree-1) accumulators of 32 KiB per sample
int mk_lhe_lookup(thfhe_mk_ctx *c, const thfhe_mk_tgsw_set *set, size_t first, size_t count, int d_tree, int d_rot, int theta, const int64_t *tab_a,
                  const int64_t *tab_b, int n_tables, const int32_t *table_index, int32_t *out, bool keyswitch) {
    return ctx_lhe_lookup(c, set, first, count, d_tree, d_rot, theta, tab_a, tab_b, n_tables, table_index, out, keyswitch, kMkLheRules,
                          [&](size_t S_max) { return c->d_acc.grow(S_max * 2 * kMkLheN * sizeof(int64_t)); },
                          [&](const cplx *spec, size_t S, const int64_t *t_a, const int64_t *t_b, const int32_t *idx, size_t tab_stride, int32_t *ks_out, bool prof) {
                              return mk_enqueue_lhe_lookup(c, spec, set->d, S, d_tree, d_rot, theta, t_a, t_b, idx, tab_stride, ks_out, prof);
                          });
}
