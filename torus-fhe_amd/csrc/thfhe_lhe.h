// thfhe_lhe.h -- leveled table lookup on TGSW-encrypted address bits (single key, N = 1024, k = 1): kernels, launchers, the set's
// fill and this engine's adaptors over the call bodies of thfhe_lhe_host.h for thfhe_tgsw_set_create, thfhe_lhe_cmux and
// thfhe_lhe_lookup(_wo_keyswitch).  Included by thfhe_sk.hip INSIDE its second anonymous namespace, after thfhe_ctx, the cooperative blind-rotate
// kernel (whose barriers and phases it reuses) and enqueue_keyswitch.
//
// Also the layered automata of DESIGN 4.16, thfhe_lhe_wfa(_wo_keyswitch): sk_lhe_wfa_step_kernel and its host side, further down; and the leveled
// scatter of DESIGN 4.17, thfhe_lhe_demux and thfhe_lhe_scatter: sk_lhe_demux_kernel, sk_lhe_scatter_rotate_kernel, sk_lhe_scatter_sum_kernel, at the end.
//
// Data flow.  The blind-rotate kernels share ONE key stream among all jobs and give every job its own rotation amounts.  Here every job has its OWN
// TGSW spectra (the address bits of its sample, 2l x 32 KiB per bit) and the rotation amounts are public: X^(2N - box 2^i) for address bit i.  Nothing
// is shared between workgroups, so both kernels are the cooperative kernel's shape -- one job per 512-thread workgroup, accumulator and the 2l digit
// spectra in LDS, the F / M / I phases of one CMux with the spectra of the step in registers -- and they are bound by streaming those spectra once.
#ifndef THFHE_LHE_H
#define THFHE_LHE_H

constexpr int kLheMaxRot = 10;   // log2 N; kLheMaxBits and kLheMaxTree are thfhe_lhe_host.h's

// One CMux ACC += C (.) D in the cooperative kernel's F / M / I phases (sk_blind_rotate_coop_kernel), C's chunks of this wave's role in B.
//   ROT:  D = X^a2n ACC - ACC (rotated_digits_z);  else D = d1 - ACC, d1 in sD1 (diff_digits_z).
//   PUB:  the mask of D is known to be zero (first tree level of a public table): its l digit polynomials are zero, so their transforms and the
//         multiplies of waves 0 .. 3 (rows 0 .. l-1) are not issued.
//   NEXT: `next` holds the spectra of the CMux that follows, requested where the cooperative kernel requests them (idle waves after the hand-off,
//         transforming waves between the stages of the inverse); else nothing follows and B is left alone.  Three rows travel that way; at
//         l = 4 the fourth would not fit the 256 registers next to the transform (the cooperative kernel spills there), so it is requested from
//         `cur`, this step's own spectra, on entry and lands under the F phase.
// Ends with the accumulator updated and a workgroup barrier.
template <int L, bool ROT, bool PUB, bool NEXT>
__device__ __forceinline__ void lhe_cmux_step(int lane, int wave, int32_t *sAcc, const int32_t *sD1, cplx (*sSpec)[512], cplx (*sX)[kXbufSlots],
                                              cplx (&B)[L][8], const cplx *cur, const cplx *next, int a2n, int Bgbit, const LaneRoots &roots, const W64 &w64) {
    constexpr int ROWS = 2 * L;
    const int c = (wave >> 1) & 1, h = wave & 1, half = wave >> 2, r0 = half * L;  // role in M: rows r0 .. r0+L-1 of (column c, limb h)
    unsigned int *ap = reinterpret_cast<unsigned int *>(sAcc) + c * 1024;
    cplx *xb = sX[wave];
    constexpr int PF = L < 3 ? L : 3;   // rows requested a step ahead
    if constexpr (NEXT && L > PF) load8(lane, B[L - 1], cur + bk_spec_index(0, r0 + L - 1, c, h, ROWS));
    // ---- F ----
    if (wave < ROWS && !(PUB && wave < L)) {
        cplx z[8];
        if constexpr (ROT) rotated_digits_z(lane, sAcc + (wave / L) * 1024, a2n, (wave % L) + 1, L, Bgbit, z);
        else diff_digits_z(lane, sD1 + (wave / L) * 1024, sAcc + (wave / L) * 1024, (wave % L) + 1, L, Bgbit, z);
        wave_fft_fwd_q(lane, z, xb, roots, w64);
#pragma unroll
        for (int m = 0; m < 8; m++) sSpec[wave][m * 64 + lane] = z[m];
    }
    wg_barrier();  // spectra published; every read of the accumulator is done
    // ---- M ----
    cplx S[8];
#pragma unroll
    for (int m = 0; m < 8; m++) S[m] = cplx{0.0, 0.0};
    if (!(PUB && half == 0)) {
#pragma unroll
        for (int r = 0; r < L; r++) {
            cplx z[8];
#pragma unroll
            for (int m = 0; m < 8; m++) z[m] = sSpec[r0 + r][m * 64 + lane];
            mac8r(S, z, B[r]);
            pin();   // one row's spectrum in registers at a time
        }
    }
    if (half == 1) {
#pragma unroll
        for (int m = 0; m < 8; m++) xb[m * 64 + lane] = S[m];   // hand-off to wave - 4
        pin();
        wg_barrier();
        if constexpr (NEXT) {
#pragma unroll
            for (int r = 0; r < PF; r++) {
                const cplx *src = next + bk_spec_index(0, r0 + r, c, h, ROWS);
#pragma unroll
                for (int m = 0; m < 8; m++) {
                    B[r][m] = src[m * 64 + lane];
                    pin();
                    __builtin_amdgcn_s_sleep(1);   // paced: these waves have the whole inverse phase
                }
            }
        }
    } else {
        if constexpr (NEXT) load8(lane, B[0], next + bk_spec_index(0, r0, c, h, ROWS));
        pin();
        wg_barrier();
        // ---- I ----
        const cplx *px = sX[wave + 4];
#pragma unroll
        for (int m = 0; m < 8; m++) {
            const cplx v = px[m * 64 + lane];
            S[m].re += v.re;
            S[m].im += v.im;
        }
        wave_sync();
        invr_seg1(lane, S, xb, w64);
        pin();
        if constexpr (NEXT && L > 1) load8(lane, B[L > 1 ? 1 : 0], next + bk_spec_index(0, r0 + 1, c, h, ROWS));
        pin();
        wave_sync();
        inv_seg2_ld(lane, S, xb);
        dft8<-1>(S);
        pin();
        if constexpr (NEXT && L > 2) load8(lane, B[L > 2 ? 2 : 0], next + bk_spec_index(0, r0 + 2, c, h, ROWS));
        pin();
        wave_transpose_hi3(S);
        invq_seg3(S, roots);
#pragma unroll
        for (int m = 0; m < 8; m++) {
            const int q = lane + 64 * m;
            atomicAdd(ap + q, round_lo32(S[m].re) << (16 * h));
            atomicAdd(ap + q + 512, round_lo32(S[m].im) << (16 * h));
        }
    }
    wg_barrier();  // accumulator updated before anybody reads it again
}

// the chunks of one TGSW sample (at `key`) that this wave multiplies with
template <int L, bool PUB>
__device__ __forceinline__ void lhe_load_spectra(int lane, int wave, cplx (&B)[L][8], const cplx *key) {
    const int c = (wave >> 1) & 1, h = wave & 1, half = wave >> 2;
    if (PUB && half == 0) return;
#pragma unroll
    for (int r = 0; r < L; r++) load8(lane, B[r], key + bk_spec_index(0, half * L + r, c, h, 2 * L));
}

// arguments of sk_lhe_rotate_kernel: job s starts from the TLWE sample (src_a, src_b) + index(s) * src_stride words, index(s) = src_idx[s] or s
// (src_a null: the trivial sample (0, src_b)), runs ACC += C_(s,i) (.) (X^(2N - box 2^i) ACC - ACC) for i = 0 .. d_rot-1 and extracts theta records
struct LheRotArgs {
    const cplx *spec;        // spectra of the set, at the first sample of the launch: [sample][d][2l][2][2][512]
    const cplx *tw;
    const int32_t *src_a, *src_b;
    const int32_t *src_idx;  // [jobs] or null
    size_t src_stride;       // words between the samples of consecutive indices (0: every job starts from index 0)
    int32_t *out;            // [jobs][theta][N+1]
    int d, d_rot, box, theta, Bgbit;
};

template <int L>
__global__ __launch_bounds__(512, 2) void sk_lhe_rotate_kernel(LheRotArgs a) {
    constexpr int ROWS = 2 * L;
    __shared__ __attribute__((aligned(4096))) int32_t sAcc[2048];
    __shared__ cplx sSpec[ROWS][512];
    __shared__ cplx sX[8][kXbufSlots];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const W64 w64{a.tw[TwRing1k::T2 + 1 * 8 + (lane & 7)]};
    const LaneRoots roots{a.tw[TwRing1k::ROOTS + 2 * lane], a.tw[TwRing1k::ROOTS + 2 * lane + 1]};
    const size_t job = blockIdx.x;
    const size_t bit_stride = (size_t)ROWS * 2048;            // complex slots of one TGSW sample
    const cplx *key = a.spec + job * a.d * bit_stride;        // the job's own address bits
    if (wave == 0) {
        const size_t t = (a.src_idx ? (size_t)a.src_idx[job] : job) * a.src_stride;
        if (a.src_a) acc_init_tlwe16(lane, sAcc, sAcc + 1024, 0, a.src_a + t, a.src_b + t);
        else acc_init_tv16(lane, sAcc, sAcc + 1024, 0, a.src_b + t);
    }
    cplx B[L][8];
    if (a.d_rot > 0) lhe_load_spectra<L, false>(lane, wave, B, key);   // (l = 4: the step requests its fourth row again, a hit)
    wg_barrier();
    for (int i = 0; i < a.d_rot; i++) {   // public, wave-uniform steps: no step is skipped
        const int a2n = 2048 - (a.box << i);
        const int inl = i + 1 < a.d_rot ? i + 1 : i;   // the last step re-requests its own chunks: unconditional loads keep B one set of registers
        lhe_cmux_step<L, true, false, true>(lane, wave, sAcc, nullptr, sSpec, sX, B, key + i * bit_stride, key + inl * bit_stride, a2n, a.Bgbit, roots, w64);
    }
    if (wave < a.theta) extract_at16(lane, sAcc, sAcc + 1024, wave, a.out + (job * a.theta + wave) * 1025);   // one wave per output
}

// arguments of sk_lhe_cmux_kernel, grid (pairs, samples): out(s, p) = d0(s, p) + C_(s,bit) (.) (d1(s, p) - d0(s, p)).  Word offsets: inputs at
// index(s) * in_sample + p * in_pair, index(s) = in_idx[s] or s; output at s * out_sample + p * out_pair.  PUB: the masks are not read (zero).
struct LheCmuxArgs {
    const cplx *spec;   // spectra of the set, at the first sample of the launch
    const cplx *tw;
    const int32_t *d0_a, *d0_b, *d1_a, *d1_b;
    int32_t *out_a, *out_b;
    const int32_t *in_idx;   // [samples] or null
    size_t in_sample, in_pair, out_sample, out_pair;
    int d, bit, Bgbit;
};

template <int L, bool PUB>
__global__ __launch_bounds__(512, 2) void sk_lhe_cmux_kernel(LheCmuxArgs a) {
    constexpr int ROWS = 2 * L;
    __shared__ __attribute__((aligned(4096))) int32_t sAcc[2048];
    __shared__ int32_t sD1[2048];
    __shared__ cplx sSpec[ROWS][512];
    __shared__ cplx sX[8][kXbufSlots];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const W64 w64{a.tw[TwRing1k::T2 + 1 * 8 + (lane & 7)]};
    const LaneRoots roots{a.tw[TwRing1k::ROOTS + 2 * lane], a.tw[TwRing1k::ROOTS + 2 * lane + 1]};
    const size_t s = blockIdx.y, pair = blockIdx.x;
    const size_t in = (a.in_idx ? (size_t)a.in_idx[s] : s) * a.in_sample + pair * a.in_pair;
    cplx B[L][8];
    lhe_load_spectra<L, PUB>(lane, wave, B, a.spec + (s * a.d + a.bit) * ((size_t)ROWS * 2048));
    for (int q = threadIdx.x; q < 1024; q += 512) {
        sAcc[q] = PUB ? 0 : a.d0_a[in + q];
        sD1[q] = PUB ? 0 : a.d1_a[in + q];
        sAcc[1024 + q] = a.d0_b[in + q];
        sD1[1024 + q] = a.d1_b[in + q];
    }
    wg_barrier();
    lhe_cmux_step<L, false, PUB, false>(lane, wave, sAcc, sD1, sSpec, sX, B, nullptr, nullptr, 0, a.Bgbit, roots, w64);
    const size_t o = s * a.out_sample + pair * a.out_pair;
    for (int q = threadIdx.x; q < 1024; q += 512) {
        a.out_a[o + q] = sAcc[q];
        a.out_b[o + q] = sAcc[1024 + q];
    }
}

// ---- layered automata on TGSW-encrypted bits: thfhe_lhe_wfa(_wo_keyswitch) ---------------------------------------------------------
constexpr int kWfaMaxSets = 64, kWfaMaxSteps = 4096, kWfaMaxStates = 64, kWfaMaxOut = 64;

// arguments of sk_lhe_wfa_step_kernel, grid (ceil(n_states / chunk), samples): one step of the automaton for every state of the workgroup's chunk,
//   layer_j(s, q) = src(s, t0) + C_(s,bit) (.) (src(s, t1) - src(s, t0)),  (t0, t1) = trans[q],   a copy of src(s, t0) where t0 == t1.
// src is layer j+1, or the finals at the last step: state t of sample s at word index(s) * src_sample + t * src_state of src_a (masks; PUB: not read,
// zero) and src_b (bodies), index(s) = src_idx[s] or s.  dst is layer j, [samples][n_states][mask | body] of N words each, never the buffer of src:
// a state of layer j+1 is read by every state that moves to it.
struct LheWfaArgs {
    const cplx *spec;   // spectra of the step's set, at the first sample of the launch
    const cplx *tw;
    const int32_t *src_a, *src_b;
    int32_t *dst;
    const int32_t *src_idx;   // [samples] or null
    const int32_t *trans;     // the step's [n_states][2], validated on the host
    size_t src_sample, src_state;
    int d, bit, Bgbit, n_states, chunk;
};

// The workgroup keeps the spectra of its sample's TGSW sample of the step in registers and walks its chunk of states: per CMux only the two
// TLWE operands (16 KiB) come from memory, the 2l x 32 KiB of spectra once per workgroup.  The transitions are public, so the copy branch is
// wave-uniform and skips the barriers of the CMux as a whole workgroup.
template <int L, bool PUB>
__global__ __launch_bounds__(512, 2) void sk_lhe_wfa_step_kernel(LheWfaArgs a) {
    constexpr int ROWS = 2 * L;
    __shared__ __attribute__((aligned(4096))) int32_t sAcc[2048];
    __shared__ int32_t sD1[2048];
    __shared__ cplx sSpec[ROWS][512];
    __shared__ cplx sX[8][kXbufSlots];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const W64 w64{a.tw[TwRing1k::T2 + 1 * 8 + (lane & 7)]};
    const LaneRoots roots{a.tw[TwRing1k::ROOTS + 2 * lane], a.tw[TwRing1k::ROOTS + 2 * lane + 1]};
    const size_t s = blockIdx.y;
    const int q0 = blockIdx.x * a.chunk, q1 = q0 + a.chunk < a.n_states ? q0 + a.chunk : a.n_states;   // the last chunk may be ragged
    const size_t in = (a.src_idx ? (size_t)a.src_idx[s] : s) * a.src_sample;
    int32_t *const dst = a.dst + s * a.n_states * 2048;
    // l <= 3 (HOLD): the wave's chunks of the spectra stay in registers for all the states of the chunk.  l = 4: the four rows (128 registers) do not
    // fit next to the inverse transform, so this instantiation does not share them: every CMux requests its rows itself, as sk_lhe_cmux_kernel
    // does, and they are dead after its multiply.  After the chunk's first state these requests hit the lines the workgroup has just read.
    constexpr bool HOLD = L <= 3;
    const cplx *const key = a.spec + (s * a.d + a.bit) * ((size_t)ROWS * 2048);
    cplx B[L][8];
    if constexpr (HOLD) lhe_load_spectra<L, PUB>(lane, wave, B, key);
#pragma unroll 1
    for (int q = q0; q < q1; q++) {
        // The lane index and the lane's roots behind an empty asm: what the transforms derive from them (the swizzled LDS slot maps, the powers
        // of the roots: 80 registers) is rebuilt inside the state.  Hoisted out of the loop it would sit next to the spectra and spill at l = 3 too.
        const int ln = opaque_lane(lane);
        W64 w = w64;
        LaneRoots r = roots;
        asm volatile("" : "+v"(w.w1.re), "+v"(w.w1.im), "+v"(r.b.re), "+v"(r.b.im), "+v"(r.s.re), "+v"(r.s.im));
        const int t0 = __builtin_amdgcn_readfirstlane(a.trans[2 * q]), t1 = __builtin_amdgcn_readfirstlane(a.trans[2 * q + 1]);
        const size_t i0 = in + t0 * a.src_state, i1 = in + t1 * a.src_state;
        int32_t *const o = dst + (size_t)q * 2048;
        if (t0 == t1) {   // both bit values lead to one state: no product, no noise
            for (int x = threadIdx.x; x < 1024; x += 512) {
                o[x] = PUB ? 0 : a.src_a[i0 + x];
                o[1024 + x] = a.src_b[i0 + x];
            }
            continue;
        }
        for (int x = threadIdx.x; x < 1024; x += 512) {   // the slots this thread read out at the end of the previous state
            sAcc[x] = PUB ? 0 : a.src_a[i0 + x];
            sD1[x] = PUB ? 0 : a.src_a[i1 + x];
            sAcc[1024 + x] = a.src_b[i0 + x];
            sD1[1024 + x] = a.src_b[i1 + x];
        }
        if constexpr (!HOLD) lhe_load_spectra<L, false>(ln, wave, B, key);   // PUB too: rows left unloaded in half the waves made the compiler carry B round the loop
        wg_barrier();
        lhe_cmux_step<L, false, PUB, false>(ln, wave, sAcc, sD1, sSpec, sX, B, nullptr, nullptr, 0, a.Bgbit, r, w);
        for (int x = threadIdx.x; x < 1024; x += 512) {
            o[x] = sAcc[x];
            o[1024 + x] = sAcc[1024 + x];
        }
    }
}

// the outputs of the automaton: record (s, o, j) is the extraction at coefficient j of state start[o] of layer 0; grid (n_out theta, samples), one wave
struct LheWfaOutArgs {
    const int32_t *layer;   // [samples][n_states][mask | body]
    const int32_t *start;   // [n_out], validated on the host
    int32_t *out;           // [samples][n_out][theta][N+1]
    int n_states, n_out, theta;
};
__global__ __launch_bounds__(64) void sk_lhe_wfa_extract_kernel(LheWfaOutArgs a) {
    const int lane = threadIdx.x, o = blockIdx.x / a.theta, j = blockIdx.x % a.theta;
    const size_t s = blockIdx.y;
    const int32_t *const v = a.layer + (s * a.n_states + a.start[o]) * 2048;
    extract_at16(lane, v, v + 1024, j, a.out + ((s * a.n_out + o) * a.theta + j) * 1025);
}

template <int L>
void launch_lhe_cmux_l(const LheCmuxArgs &a, size_t pairs, size_t samples, bool pub, hipStream_t s) {
    const dim3 grid((unsigned)pairs, (unsigned)samples);
    if (pub) hipLaunchKernelGGL((sk_lhe_cmux_kernel<L, true>), grid, dim3(512), 0, s, a);
    else hipLaunchKernelGGL((sk_lhe_cmux_kernel<L, false>), grid, dim3(512), 0, s, a);
}
int launch_lhe_cmux(thfhe_ctx *c, const LheCmuxArgs &a, size_t pairs, size_t samples, bool pub) {
    THFHE_TRY(with_static_int<4>(c->p.l, kBadL, [&](auto l) { launch_lhe_cmux_l<decltype(l)::value>(a, pairs, samples, pub, c->stream); }));
    THFHE_HIP(hipGetLastError());
    return THFHE_OK;
}
int launch_lhe_rotate(thfhe_ctx *c, const LheRotArgs &a, size_t jobs) {
    const dim3 grid((unsigned)jobs), block(512);
    THFHE_TRY(with_static_int<4>(c->p.l, kBadL, [&](auto l) { hipLaunchKernelGGL(sk_lhe_rotate_kernel<decltype(l)::value>, grid, block, 0, c->stream, a); }));
    THFHE_HIP(hipGetLastError());
    return THFHE_OK;
}
template <int L>
void launch_lhe_wfa_l(const LheWfaArgs &a, size_t chunks, size_t samples, bool pub, hipStream_t s) {
    const dim3 grid((unsigned)chunks, (unsigned)samples);
    if (pub) hipLaunchKernelGGL((sk_lhe_wfa_step_kernel<L, true>), grid, dim3(512), 0, s, a);
    else hipLaunchKernelGGL((sk_lhe_wfa_step_kernel<L, false>), grid, dim3(512), 0, s, a);
}
int launch_lhe_wfa(thfhe_ctx *c, const LheWfaArgs &a, size_t samples, bool pub) {
    const size_t chunks = ((size_t)a.n_states + a.chunk - 1) / a.chunk;
    THFHE_TRY(with_static_int<4>(c->p.l, kBadL, [&](auto l) { launch_lhe_wfa_l<decltype(l)::value>(a, chunks, samples, pub, c->stream); }));
    THFHE_HIP(hipGetLastError());
    return THFHE_OK;
}

// complex slots of the spectra of one sample of a set (d bits of 2l rows x 2 columns x 2 limbs x 512)
inline size_t lhe_sample_slots(const thfhe_ctx *c, int d) { return (size_t)d * 2 * c->p.l * 2048; }

// thfhe_tgsw_set_create after its host checks: the size check, the allocation and the sliced upload + transform
int tgsw_set_fill(thfhe_ctx *c, thfhe_tgsw_set *set, const int32_t *tgsw) {
    DevLock lk(*c);
    if (lk.rc) return lk.rc;
    const size_t polys_per_bit = (size_t)2 * c->p.l * 2, bits = set->count * set->d;
    const size_t bytes = bits * polys_per_bit * 1024 * sizeof(cplx);   // count d 2l 32 KiB
    const size_t slice_bits = std::min<size_t>(bits, std::max<size_t>(1, ((size_t)64 << 20) / (polys_per_bit * 4096)));   // 64 MiB of coefficients at a time
    const size_t stage_bytes = slice_bits * polys_per_bit * 4096;
    size_t free_b = 0, total_b = 0;
    THFHE_HIP(hipMemGetInfo(&free_b, &total_b));
    if (bytes + stage_bytes > free_b) return thfhe_fail(THFHE_E_NOMEM, "tgsw set: count d 2l 32 KiB of spectra exceed the free device memory");
    DevBuf coeff;   // upload staging, freed on return
    THFHE_TRY(coeff.grow(stage_bytes));
    THFHE_TRY(set->spec.grow(bytes));
    for (size_t b0 = 0; b0 < bits; b0 += slice_bits) {
        const size_t nb = std::min(slice_bits, bits - b0), np = nb * polys_per_bit;
        THFHE_HIP(hipMemcpyAsync(coeff.as<int32_t>(), tgsw + b0 * polys_per_bit * 1024, np * 4096, hipMemcpyHostToDevice, c->stream));
        THFHE_TRY((launch_torus_transform<1024, 32>(c->stream, coeff.as<int32_t>(), (long)np, c->d_tw.as<cplx>(), set->spec.as<cplx>() + b0 * polys_per_bit * 1024)));
        THFHE_HIP(hipStreamSynchronize(c->stream));   // the staging buffer is reused by the next slice
    }
    return THFHE_OK;
}

// what the shared leveled bodies (thfhe_lhe_host.h) admit on this engine: N = 1024, up to 32 768 samples per launch of the flat CMux
constexpr LheRules<thfhe_ctx> kLheRules{
    1024, kLheMaxRot, 32768, lhe_sample_slots,   // N, d_rot_max, cmux_slice, sample_slots
    "tgsw set: d must be 1 .. 16",                                  // set_d_text
    "tgsw set: count must be 1 .. 2^24",                            // set_count_text
    "lhe: samples first .. first+count-1 are not all in the set",   // range_text
    "lhe: the set belongs to another context",                      // ctx_text
    "lhe_cmux: bit must be 0 .. d-1",                               // bit_text
    "lhe_lookup: d_tree must be 0 .. 6",                            // d_tree_text
    "lhe_lookup: d_rot must be 0 .. 10",                            // d_rot_text
    "lhe_lookup: theta must be 1, 2 or 4",                          // theta_text
    "lhe_lookup: theta must not exceed box = N >> d_rot",           // box_text
    "lhe_lookup: n_tables 2^d_tree must be 1 .. 262144",            // n_tables_text
    "lhe_lookup: d_tree + d_rot must equal the set's d"};           // d_sum_text

// a CMux launch of the shared bodies on sk_lhe_cmux_kernel, over a set of d bits
int lhe_cmux_level(thfhe_ctx *c, int d, const LheCmuxIo<int32_t> &io, size_t pairs, size_t S) {
    const LheCmuxArgs a{io.spec, c->d_tw.as<cplx>(), io.d0_a, io.d0_b, io.d1_a, io.d1_b, io.out_a, io.out_b, io.in_idx,
                        io.in_sample, io.in_pair, io.out_sample, io.out_pair, d, io.bit, c->p.Bgbit};
    return launch_lhe_cmux(c, a, pairs, S, io.pub);
}

// thfhe_lhe_cmux: ctx_lhe_cmux (thfhe_lhe_host.h) on this engine's launch
int lhe_cmux(thfhe_ctx *c, const thfhe_tgsw_set *set, int bit, const int32_t *d1_a, const int32_t *d1_b, const int32_t *d0_a, const int32_t *d0_b,
             int32_t *out_a, int32_t *out_b, size_t count) {
    return ctx_lhe_cmux(c, set, bit, d1_a, d1_b, d0_a, d0_b, out_a, out_b, count, kLheRules,
                        [&](const LheCmuxIo<int32_t> &io, size_t S) { return lhe_cmux_level(c, set->d, io, 1, S); });
}

// The launch chain of a leveled lookup over S samples (thfhe_lhe_lookup's slices and the LOOKUP / GATHER groups of the gate DAG):
// ctx_enqueue_lhe_lookup (thfhe_lhe_host.h) on sk_lhe_cmux_kernel, sk_lhe_rotate_kernel -- one launch, which extracts its theta records into d_u
// itself -- and the context's key switch.  d: the bits of the set the spectra belong to.
int enqueue_lhe_lookup(thfhe_ctx *c, const cplx *spec, int d, size_t S, int d_tree, int d_rot, int theta, const int32_t *t_a, const int32_t *t_b,
                       const int32_t *idx, size_t tab_stride, int32_t *ks_out, bool prof) {
    return ctx_enqueue_lhe_lookup(
        c, spec, S, d_tree, d_rot, theta, t_a, t_b, idx, tab_stride, ks_out, prof, kLheRules,
        [&](const LheCmuxIo<int32_t> &io, size_t pairs) { return lhe_cmux_level(c, d, io, pairs, S); },
        [&](const int32_t *src_a, const int32_t *src_b, const int32_t *src_idx, size_t src_stride) {
            const LheRotArgs r{spec, c->d_tw.as<cplx>(), src_a, src_b, src_idx, src_stride, c->d_u.as<int32_t>(), d, d_rot, 1024 >> d_rot, theta, c->p.Bgbit};
            return launch_lhe_rotate(c, r, S);
        },
        [&](int32_t *out, size_t records) { return enqueue_keyswitch(c, c->d_u.as<int32_t>(), out, records, 1, false); });
}

// thfhe_lhe_lookup (keyswitch) / thfhe_lhe_lookup_wo_keyswitch: ctx_lhe_lookup (thfhe_lhe_host.h) on this engine's chain; the tree workspace is
// 2^(d_tree-1) TLWE samples of 8 KiB per sample
int lhe_lookup(thfhe_ctx *c, const thfhe_tgsw_set *set, size_t first, size_t count, int d_tree, int d_rot, int theta, const int32_t *tab_a,
               const int32_t *tab_b, int n_tables, const int32_t *table_index, int32_t *out, bool keyswitch) {
    return ctx_lhe_lookup(c, set, first, count, d_tree, d_rot, theta, tab_a, tab_b, n_tables, table_index, out, keyswitch, kLheRules,
                          [](size_t) { return (int)THFHE_OK; },
                          [&](const cplx *spec, size_t S, const int32_t *t_a, const int32_t *t_b, const int32_t *idx, size_t tab_stride, int32_t *ks_out, bool prof) {
                              return enqueue_lhe_lookup(c, spec, set->d, S, d_tree, d_rot, theta, t_a, t_b, idx, tab_stride, ks_out, prof);
                          });
}

// compute units of the context's device, asked once per context
int ctx_cus(thfhe_ctx *c, int *cus) {
    if (!c->cus) THFHE_HIP(hipDeviceGetAttribute(&c->cus, hipDeviceAttributeMultiprocessorCount, c->device));
    *cus = c->cus;
    return THFHE_OK;
}

// states per workgroup of a step on S samples: the forced value (thfhe_set_wfa_chunk), else the largest for which ceil(n_states / G) S workgroups
// still give every compute unit one -- all the states of a sample once S reaches the number of compute units
int wfa_chunk_for(const thfhe_ctx *c, int n_states, size_t S, int cus) {
    if (c->wfa_chunk) return std::min(c->wfa_chunk, n_states);
    for (int g = n_states; g > 1; g--)
        if ((size_t)((n_states + g - 1) / g) * S >= (size_t)cus) return g;
    return 1;
}

// The launch chain of a layered automaton over S samples, on device pointers only (thfhe_lhe_wfa's slices and the WFA groups of the gate DAG, DESIGN
// 4.18): one launch per step, the extraction, and with ks_out the key switch of the S n_out theta records into it (else they stay in d_u).  Samples
// first .. first + S - 1 of the sets; step_bit is the HOST array; d_trans / d_start: the transitions and start states on the device; sample s reads
// its n_states finals at (f_a, f_b) + index(s) * fin_stride words, index(s) = idx[s] or s (f_a null: public).  The caller has sized d_lhe_a / d_lhe_b
// (S layers each), d_u and ks_out.
int enqueue_lhe_wfa(thfhe_ctx *c, const thfhe_tgsw_set *const *sets, size_t first, size_t S, int n_steps, int n_states, const int32_t *step_bit,
                    const int32_t *d_trans, const int32_t *d_start, const int32_t *f_a, const int32_t *f_b, const int32_t *idx, size_t fin_stride, int theta,
                    int n_out, int cus, int32_t *ks_out, bool prof) {
    hipStream_t st = c->stream;
    const size_t recs = (size_t)n_out * theta, layer_words = (size_t)n_states * 2048;
    int32_t *const layer[2] = {c->d_lhe_a.as<int32_t>(), c->d_lhe_b.as<int32_t>()};
    if (prof) THFHE_HIP(hipEventRecord(c->ev[0], st));
    const int chunk = wfa_chunk_for(c, n_states, S, cus);
    for (int j = n_steps - 1; j >= 0; j--) {
        const thfhe_tgsw_set *set = sets[step_bit[j] >> 4];
        LheWfaArgs a{set->spec.as<cplx>() + first * lhe_sample_slots(c, set->d), c->d_tw.as<cplx>(), nullptr, nullptr, layer[j & 1], nullptr,
                     d_trans + (size_t)j * n_states * 2, 0, 0, set->d, step_bit[j] & 15, c->p.Bgbit, n_states, chunk};
        const bool last = j == n_steps - 1;   // the first launch: it reads the finals, of the sample's table if there is an index
        if (last) {
            a.src_a = f_a, a.src_b = f_b, a.src_idx = idx;
            a.src_sample = fin_stride, a.src_state = 1024;
        } else {
            a.src_a = layer[(j + 1) & 1], a.src_b = a.src_a + 1024;
            a.src_sample = layer_words, a.src_state = 2048;
        }
        THFHE_TRY(launch_lhe_wfa(c, a, S, last && !f_a));
    }
    if (prof) THFHE_HIP(hipEventRecord(c->ev[1], st));
    const LheWfaOutArgs x{layer[0], d_start, c->d_u.as<int32_t>(), n_states, n_out, theta};
    hipLaunchKernelGGL(sk_lhe_wfa_extract_kernel, dim3((unsigned)recs, (unsigned)S), dim3(64), 0, st, x);
    THFHE_HIP(hipGetLastError());
    if (prof) THFHE_HIP(hipEventRecord(c->ev[2], st));
    if (ks_out) THFHE_TRY(enqueue_keyswitch(c, c->d_u.as<int32_t>(), ks_out, S * recs, 1, false));
    if (prof) {
        THFHE_HIP(hipEventRecord(c->ev[3], st));
        c->ev_valid = true;
    }
    return THFHE_OK;
}

// thfhe_lhe_wfa (keyswitch) / thfhe_lhe_wfa_wo_keyswitch: out = count x n_out x theta records of n+1 (resp. N+1) words.  One launch per step on the
// context's stream: step j reads layer j+1 (the finals at j = n_steps-1) and writes layer j, the layers alternating between d_lhe_a and d_lhe_b,
// layer j in buffer j & 1, so layer 0 -- the one the outputs are extracted from -- is always in d_lhe_a.
int lhe_wfa(thfhe_ctx *c, const thfhe_tgsw_set *const *sets, int n_sets, size_t first, size_t count, int n_steps, int n_states, const int32_t *trans,
            const int32_t *step_bit, const int32_t *fin_a, const int32_t *fin_b, int n_tables, const int32_t *table_index, int theta, const int32_t *start,
            int n_out, int32_t *out, bool keyswitch) {
    // host checks, before any set or context is looked at
    if (!sets || !trans || !step_bit || !fin_b || !start || !out) return thfhe_fail(THFHE_E_INVALID, "null argument");
    if (n_sets < 1 || n_sets > kWfaMaxSets) return thfhe_fail(THFHE_E_INVALID, "lhe_wfa: n_sets must be 1 .. 64");
    if (n_steps < 1 || n_steps > kWfaMaxSteps) return thfhe_fail(THFHE_E_INVALID, "lhe_wfa: n_steps must be 1 .. 4096");
    if (n_states < 1 || n_states > kWfaMaxStates) return thfhe_fail(THFHE_E_INVALID, "lhe_wfa: n_states must be 1 .. 64");
    if (n_out < 1 || n_out > kWfaMaxOut) return thfhe_fail(THFHE_E_INVALID, "lhe_wfa: n_out must be 1 .. 64");
    if (theta != 1 && theta != 2 && theta != 4) return thfhe_fail(THFHE_E_INVALID, "lhe_wfa: theta must be 1, 2 or 4");
    if (n_tables < 1 || (long)n_tables * n_states > kMaxEncLuts) return thfhe_fail(THFHE_E_INVALID, "lhe_wfa: n_tables n_states must be 1 .. 262144");
    const size_t n_trans = (size_t)n_steps * n_states * 2;
    for (size_t i = 0; i < n_trans; i++)
        if (trans[i] < 0 || trans[i] >= n_states) return thfhe_fail(THFHE_E_INVALID, "lhe_wfa: trans entry out of range (0 .. n_states-1)");
    for (int o = 0; o < n_out; o++)
        if (start[o] < 0 || start[o] >= n_states) return thfhe_fail(THFHE_E_INVALID, "lhe_wfa: start entry out of range (0 .. n_states-1)");
    THFHE_TRY(tree_validate_index(table_index, n_tables, count));
    // the sets
    for (int i = 0; i < n_sets; i++)
        if (!sets[i]) return thfhe_fail(THFHE_E_INVALID, "null tgsw set");
    for (int j = 0; j < n_steps; j++)
        if (step_bit[j] < 0 || (step_bit[j] >> 4) >= n_sets || (step_bit[j] & 15) >= sets[step_bit[j] >> 4]->d)
            return thfhe_fail(THFHE_E_INVALID, "lhe_wfa: step_bit must name bit 0 .. d-1 of set 0 .. n_sets-1 (16 set + bit)");
    for (int i = 1; i < n_sets; i++)
        if (sets[i]->count != sets[0]->count || sets[i]->ctx != sets[0]->ctx)
            return thfhe_fail(THFHE_E_INVALID, "lhe_wfa: the sets must have one count and one context");
    THFHE_TRY(ctx_lhe_validate_range(sets[0], first, count, kLheRules.range_text));
    THFHE_TRY(ctx_lhe_validate_ctx(c, sets[0], kLheRules.ctx_text));
    if (count == 0) return THFHE_OK;
    DevLock lk(*c);
    if (lk.rc) return lk.rc;
    int cus = 0;
    THFHE_TRY(ctx_cus(c, &cus));
    // a slice: two layers of n_states TLWE samples per sample within the tree workspace's bound, at most tree_slice output records, one grid.y
    const size_t recs = (size_t)n_out * theta;
    const size_t S_max = std::min({count, (size_t)65535, std::max<size_t>(1, c->tree_slice / (2 * (size_t)n_states)), std::max<size_t>(1, c->tree_slice / recs)});
    const size_t words = c->p.n + 1, rec = keyswitch ? words : 1025, fin_bytes = (size_t)n_tables * n_states * 4096;
    const size_t layer_words = (size_t)n_states * 2048, tab_bytes = (n_trans + n_out) * sizeof(int32_t);
    int rc = c->d_tv.grow(fin_bytes);
    if (!rc && fin_a) rc = c->d_tva.grow(fin_bytes);
    if (!rc) rc = c->d_lhe_a.grow(S_max * layer_words * sizeof(int32_t));
    if (!rc) rc = c->d_lhe_b.grow(S_max * layer_words * sizeof(int32_t));
    if (!rc) rc = c->d_wfa_tab.grow(tab_bytes);
    if (!rc) rc = c->d_u.grow(S_max * recs * 1025 * sizeof(int32_t));
    if (!rc && keyswitch) rc = c->stage.grow(S_max * recs * words);
    if (!rc && table_index) rc = c->d_lut_idx.grow(S_max * sizeof(int32_t));
    if (rc) return rc;
    hipStream_t st = c->stream;
    THFHE_HIP(hipMemcpyAsync(c->d_tv.as<int32_t>(), fin_b, fin_bytes, hipMemcpyHostToDevice, st));
    if (fin_a) THFHE_HIP(hipMemcpyAsync(c->d_tva.as<int32_t>(), fin_a, fin_bytes, hipMemcpyHostToDevice, st));
    int32_t *const d_trans = c->d_wfa_tab.as<int32_t>(), *const d_start = d_trans + n_trans;
    THFHE_HIP(hipMemcpyAsync(d_trans, trans, n_trans * sizeof(int32_t), hipMemcpyHostToDevice, st));
    THFHE_HIP(hipMemcpyAsync(d_start, start, n_out * sizeof(int32_t), hipMemcpyHostToDevice, st));
    int32_t *const res = keyswitch ? c->stage.out_ptr() : c->d_u.as<int32_t>();
    for (size_t s0 = 0; s0 < count; s0 += S_max) {
        const size_t S = std::min(S_max, count - s0);
        if (table_index) THFHE_HIP(hipMemcpyAsync(c->d_lut_idx.as<int32_t>(), table_index + s0, S * sizeof(int32_t), hipMemcpyHostToDevice, st));
        THFHE_TRY(enqueue_lhe_wfa(c, sets, first + s0, S, n_steps, n_states, step_bit, d_trans, d_start, fin_a ? c->d_tva.as<int32_t>() : nullptr,
                                  c->d_tv.as<int32_t>(), table_index ? c->d_lut_idx.as<int32_t>() : nullptr, table_index ? (size_t)n_states * 1024 : 0, theta,
                                  n_out, cus, keyswitch ? c->stage.out_ptr() : nullptr, c->profiling && s0 == 0));
        THFHE_HIP(hipMemcpyAsync(out + s0 * recs * rec, res, S * recs * rec * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    }
    THFHE_HIP(hipStreamSynchronize(st));
    return THFHE_OK;
}

// ---- leveled scatter: demux trees that write at TGSW-encrypted addresses: thfhe_lhe_demux, thfhe_lhe_scatter --------------------------
constexpr int kScatterMaxVals = 1 << 24;

// arguments of sk_lhe_demux_kernel, grid (nodes, samples): child 1 of node (s, q) = C_(s,bit) (.) x(s, q), child 0 = x(s, q) - child 1.  Word offsets:
// x at index(s) * in_sample + q * in_node, index(s) = in_idx[s] or s; both children at s * out_sample + q * out_node of their own pointers.  A child
// may be written over x: the node is in LDS before the first store.  PUB: x_a is not read (zero).
struct LheDemuxArgs {
    const cplx *spec;   // spectra of the set, at the first sample of the launch
    const cplx *tw;
    const int32_t *x_a, *x_b;
    int32_t *out0_a, *out0_b, *out1_a, *out1_b;
    const int32_t *in_idx;   // [samples] or null
    size_t in_sample, in_node, out_sample, out_node;
    int d, bit, Bgbit;
};

// One external product, two outputs: sk_lhe_cmux_kernel with d0 = 0 and d1 = x, which then also stores x - product.
template <int L, bool PUB>
__global__ __launch_bounds__(512, 2) void sk_lhe_demux_kernel(LheDemuxArgs a) {
    constexpr int ROWS = 2 * L;
    __shared__ __attribute__((aligned(4096))) int32_t sAcc[2048];
    __shared__ int32_t sD1[2048];
    __shared__ cplx sSpec[ROWS][512];
    __shared__ cplx sX[8][kXbufSlots];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const W64 w64{a.tw[TwRing1k::T2 + 1 * 8 + (lane & 7)]};
    const LaneRoots roots{a.tw[TwRing1k::ROOTS + 2 * lane], a.tw[TwRing1k::ROOTS + 2 * lane + 1]};
    const size_t s = blockIdx.y, node = blockIdx.x;
    const size_t in = (a.in_idx ? (size_t)a.in_idx[s] : s) * a.in_sample + node * a.in_node;
    cplx B[L][8];
    lhe_load_spectra<L, PUB>(lane, wave, B, a.spec + (s * a.d + a.bit) * ((size_t)ROWS * 2048));
    for (int q = threadIdx.x; q < 1024; q += 512) {
        sAcc[q] = 0;
        sAcc[1024 + q] = 0;
        sD1[q] = PUB ? 0 : a.x_a[in + q];
        sD1[1024 + q] = a.x_b[in + q];
    }
    wg_barrier();   // x is read: from here on its slot may be written
    lhe_cmux_step<L, false, PUB, false>(lane, wave, sAcc, sD1, sSpec, sX, B, nullptr, nullptr, 0, a.Bgbit, roots, w64);
    const size_t o = s * a.out_sample + node * a.out_node;
    for (int q = threadIdx.x; q < 1024; q += 512) {
        const uint32_t pa = (uint32_t)sAcc[q], pb = (uint32_t)sAcc[1024 + q];
        a.out1_a[o + q] = (int32_t)pa;
        a.out1_b[o + q] = (int32_t)pb;
        a.out0_a[o + q] = (int32_t)((uint32_t)sD1[q] - pa);
        a.out0_b[o + q] = (int32_t)((uint32_t)sD1[1024 + q] - pb);
    }
}

// arguments of sk_lhe_scatter_rotate_kernel: sk_lhe_rotate_kernel's start (LheRotArgs: src_a, src_b, src_idx, src_stride), the POSITIVE rotations
// ACC += C_(s,i) (.) (X^(box 2^i) ACC - ACC) for i = 0 .. d_rot-1, and the whole accumulator (mask | body) to out + job * out_stride
struct LheScatterRotArgs {
    const cplx *spec;
    const cplx *tw;
    const int32_t *src_a, *src_b;
    const int32_t *src_idx;
    size_t src_stride;
    int32_t *out;
    size_t out_stride;   // words between the accumulators of consecutive jobs
    int d, d_rot, box, Bgbit;
};

// sk_lhe_rotate_kernel's loop, mirrored: the value moves UP to coefficient (addr mod 2^d_rot) box, where the lookup moves an entry down to 0.  The
// largest total shift is N - box, so nothing wraps.  Nothing is extracted: the accumulator is the root of the sample's demux tree.
template <int L>
__global__ __launch_bounds__(512, 2) void sk_lhe_scatter_rotate_kernel(LheScatterRotArgs a) {
    constexpr int ROWS = 2 * L;
    __shared__ __attribute__((aligned(4096))) int32_t sAcc[2048];
    __shared__ cplx sSpec[ROWS][512];
    __shared__ cplx sX[8][kXbufSlots];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const W64 w64{a.tw[TwRing1k::T2 + 1 * 8 + (lane & 7)]};
    const LaneRoots roots{a.tw[TwRing1k::ROOTS + 2 * lane], a.tw[TwRing1k::ROOTS + 2 * lane + 1]};
    const size_t job = blockIdx.x;
    const size_t bit_stride = (size_t)ROWS * 2048;
    const cplx *key = a.spec + job * a.d * bit_stride;
    if (wave == 0) {
        const size_t t = (a.src_idx ? (size_t)a.src_idx[job] : job) * a.src_stride;
        if (a.src_a) acc_init_tlwe16(lane, sAcc, sAcc + 1024, 0, a.src_a + t, a.src_b + t);
        else acc_init_tv16(lane, sAcc, sAcc + 1024, 0, a.src_b + t);
    }
    cplx B[L][8];
    lhe_load_spectra<L, false>(lane, wave, B, key);   // d_rot >= 1: the host does not launch this kernel otherwise
    wg_barrier();
    for (int i = 0; i < a.d_rot; i++) {
        const int a2n = a.box << i;   // <= N / 2
        const int inl = i + 1 < a.d_rot ? i + 1 : i;
        lhe_cmux_step<L, true, false, true>(lane, wave, sAcc, nullptr, sSpec, sX, B, key + i * bit_stride, key + inl * bit_stride, a2n, a.Bgbit, roots, w64);
    }
    int32_t *const o = a.out + job * a.out_stride;
    for (int q = threadIdx.x; q < 2048; q += 512) o[q] = sAcc[q];
}

// arguments of sk_lhe_scatter_sum_kernel, grid (leaves, samples): leaf P of sample s is added into polynomial P of table tab_idx[s] (null: table 0)
struct LheScatterSumArgs {
    const int32_t *leaves;    // [samples][n_leaves][mask | body]
    const int32_t *tab_idx;   // [samples] or null, validated on the host
    int32_t *tab;             // masks [n_tables][n_leaves][N], then the bodies tab_half words further
    size_t tab_half;
    int n_leaves;
};
// Samples of one table meet on the same words, so the sum is made of atomic adds in global memory; integer sums mod 2^32 do not depend on their order.
__global__ __launch_bounds__(256) void sk_lhe_scatter_sum_kernel(LheScatterSumArgs a) {
    const size_t s = blockIdx.y, P = blockIdx.x;
    const int32_t *const v = a.leaves + (s * a.n_leaves + P) * 2048;
    const size_t t = a.tab_idx ? (size_t)a.tab_idx[s] : 0;
    unsigned int *const dst = reinterpret_cast<unsigned int *>(a.tab) + (t * a.n_leaves + P) * 1024;
    for (int q = threadIdx.x; q < 1024; q += 256) {
        atomicAdd(dst + q, (unsigned int)v[q]);
        atomicAdd(dst + a.tab_half + q, (unsigned int)v[1024 + q]);
    }
}

template <int L>
void launch_lhe_demux_l(const LheDemuxArgs &a, size_t nodes, size_t samples, bool pub, hipStream_t s) {
    const dim3 grid((unsigned)nodes, (unsigned)samples);
    if (pub) hipLaunchKernelGGL((sk_lhe_demux_kernel<L, true>), grid, dim3(512), 0, s, a);
    else hipLaunchKernelGGL((sk_lhe_demux_kernel<L, false>), grid, dim3(512), 0, s, a);
}
int launch_lhe_demux(thfhe_ctx *c, const LheDemuxArgs &a, size_t nodes, size_t samples, bool pub) {
    THFHE_TRY(with_static_int<4>(c->p.l, kBadL, [&](auto l) { launch_lhe_demux_l<decltype(l)::value>(a, nodes, samples, pub, c->stream); }));
    THFHE_HIP(hipGetLastError());
    return THFHE_OK;
}
int launch_lhe_scatter_rotate(thfhe_ctx *c, const LheScatterRotArgs &a, size_t jobs) {
    const dim3 grid((unsigned)jobs), block(512);
    THFHE_TRY(with_static_int<4>(c->p.l, kBadL, [&](auto l) { hipLaunchKernelGGL(sk_lhe_scatter_rotate_kernel<decltype(l)::value>, grid, block, 0, c->stream, a); }));
    THFHE_HIP(hipGetLastError());
    return THFHE_OK;
}

// thfhe_lhe_demux: the flat form of one node per sample.  x goes up into d_lhe_a / d_lhe_b, the children come down from d_lhe_in[0 .. 3].
int lhe_demux(thfhe_ctx *c, const thfhe_tgsw_set *set, int bit, const int32_t *x_a, const int32_t *x_b, int32_t *out0_a, int32_t *out0_b, int32_t *out1_a,
              int32_t *out1_b, size_t count) {
    if (!x_b || !out0_a || !out0_b || !out1_a || !out1_b) return thfhe_fail(THFHE_E_INVALID, "null argument");
    if (bit < 0 || bit >= kLheMaxBits) return thfhe_fail(THFHE_E_INVALID, "lhe_demux: bit must be 0 .. d-1");
    if (!set) return thfhe_fail(THFHE_E_INVALID, "null tgsw set");
    if (bit >= set->d) return thfhe_fail(THFHE_E_INVALID, "lhe_demux: bit must be 0 .. d-1");
    THFHE_TRY(ctx_lhe_validate_range(set, 0, count, kLheRules.range_text));
    THFHE_TRY(ctx_lhe_validate_ctx(c, set, kLheRules.ctx_text));
    if (count == 0) return THFHE_OK;
    DevLock lk(*c);
    if (lk.rc) return lk.rc;
    const size_t S_max = std::min<size_t>(count, 32768), bytes = S_max * 4096;
    for (DevBuf &b : c->d_lhe_in) THFHE_TRY(b.grow(bytes));
    if (x_a) THFHE_TRY(c->d_lhe_a.grow(bytes));
    THFHE_TRY(c->d_lhe_b.grow(bytes));
    int32_t *const dst[4] = {out0_a, out0_b, out1_a, out1_b};
    for (size_t s0 = 0; s0 < count; s0 += S_max) {
        const size_t S = std::min(S_max, count - s0);
        if (x_a) THFHE_HIP(hipMemcpyAsync(c->d_lhe_a.as<int32_t>(), x_a + s0 * 1024, S * 4096, hipMemcpyHostToDevice, c->stream));
        THFHE_HIP(hipMemcpyAsync(c->d_lhe_b.as<int32_t>(), x_b + s0 * 1024, S * 4096, hipMemcpyHostToDevice, c->stream));
        LheDemuxArgs a{set->spec.as<cplx>() + s0 * lhe_sample_slots(c, set->d), c->d_tw.as<cplx>(), x_a ? c->d_lhe_a.as<int32_t>() : nullptr,
                       c->d_lhe_b.as<int32_t>(), c->d_lhe_in[0].as<int32_t>(), c->d_lhe_in[1].as<int32_t>(), c->d_lhe_in[2].as<int32_t>(),
                       c->d_lhe_in[3].as<int32_t>(), nullptr, 1024, 0, 1024, 0, set->d, bit, c->p.Bgbit};
        THFHE_TRY(launch_lhe_demux(c, a, 1, S, !x_a));
        for (int q = 0; q < 4; q++) THFHE_HIP(hipMemcpyAsync(dst[q] + s0 * 1024, c->d_lhe_in[q].as<int32_t>(), S * 4096, hipMemcpyDeviceToHost, c->stream));
    }
    THFHE_HIP(hipStreamSynchronize(c->stream));
    return THFHE_OK;
}

// thfhe_lhe_scatter: per slice of at most tree_slice / 2^d_tree samples (the workspace: 2^d_tree TLWE samples of 8 KiB per sample) the rotations into
// slot 0 of every sample, the demux tree in place -- the node at depth k, prefix q, lies in slot q 2^(d_tree-k), keeps child 0 there and writes child 1
// 2^(d_tree-k-1) slots further, so leaf P ends in slot P -- and the sum of the leaves into the tables, which stay on the device until the last slice.
int lhe_scatter(thfhe_ctx *c, const thfhe_tgsw_set *set, size_t first, size_t count, int d_tree, int d_rot, const int32_t *val_a, const int32_t *val_b,
                int n_vals, const int32_t *val_index, int n_tables, const int32_t *table_index, int32_t *tab_a, int32_t *tab_b) {
    // host checks, before the set or the context is looked at
    if (!val_b || !tab_a || !tab_b) return thfhe_fail(THFHE_E_INVALID, "null argument");
    if (d_tree < 0 || d_tree > kLheMaxTree) return thfhe_fail(THFHE_E_INVALID, "lhe_scatter: d_tree must be 0 .. 6");
    if (d_rot < 0 || d_rot > kLheMaxRot) return thfhe_fail(THFHE_E_INVALID, "lhe_scatter: d_rot must be 0 .. 10");
    if (n_tables < 1 || ((long)n_tables << d_tree) > kMaxEncLuts) return thfhe_fail(THFHE_E_INVALID, "lhe_scatter: n_tables 2^d_tree must be 1 .. 262144");
    if (n_vals < 1 || n_vals > kScatterMaxVals) return thfhe_fail(THFHE_E_INVALID, "lhe_scatter: n_vals must be 1 .. 2^24");
    if (count > (size_t)INT32_MAX / 16) return thfhe_fail(THFHE_E_INVALID, "count too large");
    if (val_index) {
        for (size_t g = 0; g < count; g++)
            if (val_index[g] < 0 || val_index[g] >= n_vals) return thfhe_fail(THFHE_E_INVALID, "val_index out of range (0 .. n_vals-1)");
    } else if (n_vals != 1 && (size_t)n_vals != count) {
        return thfhe_fail(THFHE_E_INVALID, "lhe_scatter: without val_index n_vals must be 1 or count");
    }
    THFHE_TRY(tree_validate_index(table_index, n_tables, count));
    if (!set) return thfhe_fail(THFHE_E_INVALID, "null tgsw set");
    if (d_tree + d_rot != set->d) return thfhe_fail(THFHE_E_INVALID, "lhe_scatter: d_tree + d_rot must equal the set's d");
    THFHE_TRY(ctx_lhe_validate_range(set, first, count, kLheRules.range_text));
    THFHE_TRY(ctx_lhe_validate_ctx(c, set, kLheRules.ctx_text));
    const size_t leaves = (size_t)1 << d_tree, tab_words = (size_t)n_tables * leaves * 1024;
    if (count == 0) {   // nothing is written anywhere: the tables are their starting value
        std::fill_n(tab_a, tab_words, 0);
        std::fill_n(tab_b, tab_words, 0);
        return THFHE_OK;
    }
    DevLock lk(*c);
    if (lk.rc) return lk.rc;
    const size_t S_max = std::min({count, (size_t)65535, std::max<size_t>(1, c->tree_slice / leaves)});
    const bool per_slice = !val_index && n_vals > 1;   // value s belongs to sample s: a slice's values go up with the slice
    const size_t val_bytes = (per_slice ? S_max : (size_t)n_vals) * 4096;
    int rc = c->d_sc_tab.grow(2 * tab_words * sizeof(int32_t));
    if (!rc) rc = c->d_lhe_a.grow(S_max * leaves * 2048 * sizeof(int32_t));
    if (!rc) rc = c->d_tv.grow(val_bytes);
    if (!rc && val_a) rc = c->d_tva.grow(val_bytes);
    if (!rc && (val_index || table_index)) rc = c->d_sc_idx.grow(2 * S_max * sizeof(int32_t));
    if (rc) return rc;
    hipStream_t st = c->stream;
    int32_t *const tab = c->d_sc_tab.as<int32_t>(), *const w = c->d_lhe_a.as<int32_t>();
    int32_t *const d_vidx = c->d_sc_idx.as<int32_t>(), *const d_tidx = d_vidx + S_max;
    const int32_t *const v_a = val_a ? c->d_tva.as<int32_t>() : nullptr, *const v_b = c->d_tv.as<int32_t>();
    THFHE_HIP(hipMemsetAsync(tab, 0, 2 * tab_words * sizeof(int32_t), st));
    if (!per_slice) {
        THFHE_HIP(hipMemcpyAsync(c->d_tv.as<int32_t>(), val_b, val_bytes, hipMemcpyHostToDevice, st));
        if (val_a) THFHE_HIP(hipMemcpyAsync(c->d_tva.as<int32_t>(), val_a, val_bytes, hipMemcpyHostToDevice, st));
    }
    const size_t val_stride = n_vals > 1 ? 1024 : 0, ws = leaves * 2048;   // ws: words of workspace per sample
    for (size_t s0 = 0; s0 < count; s0 += S_max) {
        const size_t S = std::min(S_max, count - s0);
        const cplx *spec = set->spec.as<cplx>() + (first + s0) * lhe_sample_slots(c, set->d);
        if (per_slice) {
            THFHE_HIP(hipMemcpyAsync(c->d_tv.as<int32_t>(), val_b + s0 * 1024, S * 4096, hipMemcpyHostToDevice, st));
            if (val_a) THFHE_HIP(hipMemcpyAsync(c->d_tva.as<int32_t>(), val_a + s0 * 1024, S * 4096, hipMemcpyHostToDevice, st));
        }
        if (val_index) THFHE_HIP(hipMemcpyAsync(d_vidx, val_index + s0, S * sizeof(int32_t), hipMemcpyHostToDevice, st));
        if (table_index) THFHE_HIP(hipMemcpyAsync(d_tidx, table_index + s0, S * sizeof(int32_t), hipMemcpyHostToDevice, st));
        if (c->profiling && s0 == 0) THFHE_HIP(hipEventRecord(c->ev[0], st));
        if (d_rot > 0) {
            LheScatterRotArgs r{spec, c->d_tw.as<cplx>(), v_a, v_b, val_index ? d_vidx : nullptr, val_stride, w, ws, set->d, d_rot, 1024 >> d_rot, c->p.Bgbit};
            THFHE_TRY(launch_lhe_scatter_rotate(c, r, S));
        }
        if (c->profiling && s0 == 0) THFHE_HIP(hipEventRecord(c->ev[1], st));
        for (int k = 0; k < d_tree; k++) {
            const size_t node = ws >> k, half = node / 2;   // words between the nodes of depth k; child 1 lies half a node further
            LheDemuxArgs a{spec, c->d_tw.as<cplx>(), w, w + 1024, w, w + 1024, w + half, w + half + 1024, nullptr, ws, node, ws, node, set->d, set->d - 1 - k, c->p.Bgbit};
            const bool from_values = k == 0 && d_rot == 0;   // no rotation ran: the root is the value itself, and a trivial value has a zero mask
            if (from_values) a.x_a = v_a, a.x_b = v_b, a.in_idx = val_index ? d_vidx : nullptr, a.in_sample = val_stride, a.in_node = 0;
            THFHE_TRY(launch_lhe_demux(c, a, (size_t)1 << k, S, from_values && !val_a));
        }
        if (c->profiling && s0 == 0) THFHE_HIP(hipEventRecord(c->ev[2], st));
        const LheScatterSumArgs x{w, table_index ? d_tidx : nullptr, tab, tab_words, (int)leaves};
        hipLaunchKernelGGL(sk_lhe_scatter_sum_kernel, dim3((unsigned)leaves, (unsigned)S), dim3(256), 0, st, x);
        THFHE_HIP(hipGetLastError());
        if (c->profiling && s0 == 0) {
            THFHE_HIP(hipEventRecord(c->ev[3], st));
            c->ev_valid = true;
        }
    }
    THFHE_HIP(hipMemcpyAsync(tab_a, tab, tab_words * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    THFHE_HIP(hipMemcpyAsync(tab_b, tab + tab_words, tab_words * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    THFHE_HIP(hipStreamSynchronize(st));
    return THFHE_OK;
}

#endif  // THFHE_LHE_H
