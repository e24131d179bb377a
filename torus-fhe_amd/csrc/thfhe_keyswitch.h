// thfhe_keyswitch.h -- the LWE key switch of every engine (single key: J/keyswitch.jl:45-80 with the MUX combine of J/gates.jl:172-176;
// multi key: J/mk_internals.jl:730-744, one key per party): the padded key (KsKey), one argument struct, and the kernels and launcher
// that all engines share.
//
//   ks_pad_kernel              key rows of n + 1 words -> rows of row_words (a multiple of 128), zero-padded
//   ks_plain_kernel            one workgroup per (sample, party, coordinate range); the output row in registers (small batches, other shapes)
//   ks_staged_kernel           32 samples per workgroup, the rows of a few (i, j) staged in LDS, the digit selecting an address (from 192 samples on)
//   sk_keyswitch_mfma_kernel   single key, 2-bit digits, t = 4 or 8: the key switch as an int8 GEMM on the matrix cores (from 512 samples on);
//   sk_ksk_planes_kernel       its key planes
//
// The LWE -> TLWE packing key switch (thfhe_threshold.hip) runs on the same kernels: its key rows are TLWE samples of 2N words, b lands
// at word N of the output record (KsArgs::b_col, ::out_rec), and its coordinates are padded to a multiple of 128 (KsKey::upload_pack).
//
// Every sample's output is the sum of per-(party, coordinate range) partial sums: integer adds commute, so atomics into a zeroed output
// are bit-exact.  ks_enqueue picks the kernel and zeroes the output where the kernel accumulates.
#ifndef THFHE_KEYSWITCH_H
#define THFHE_KEYSWITCH_H

#include <hip/hip_runtime.h>

#include "../../include/thfhe_hip.h"
#include "thfhe_common.h"
#include "thfhe_devctx.h"

namespace {
using namespace thfhe;

// One key switch of `samples` extracted samples into out[samples][parties * n + 1].  Sample g's input starts at u + g * rot_per_gate * u_rec:
// party p reads mask words [p * u_pstride, p * u_pstride + N), b is the last word of the record.  Single key: parties = 1, u_rec = N + 1,
// u_pstride = 0; rot_per_gate = 2 adds two records (the MUX combine: u1 + u2 and b1 + b2 + 2^29).  3-gen: ONE mask for all parties
// (u_rec = N + 1, u_pstride = 0); CCS, KMS: one mask per party (u_rec = P N + 1, u_pstride = N).
struct KsArgs {
    const int32_t *ksk;  // [P][N][t][base-1][row_words]
    const int32_t *u;
    int32_t *out;
    long samples;
    int n, t, basebit, parties, row_words;
    int N;  // ring degree = dimension of the extracted sample
    int u_rec, u_pstride;
    int rot_per_gate;
    int out_rec;  // words per output record: parties * n + 1; the packing key: 2N
    int b_col;    // output column that receives b: n (its own word after the parties' masks); the packing key: N (inside the row)
};

constexpr long kKsMfmaMinSamples = 512;    // batches from this size on run sk_keyswitch_mfma_kernel where its shape allows
constexpr long kKsStagedMinSamples = 192;  // ... ks_staged_kernel (measured, SK-128: 128 gates 0.146 ms plain / 0.184 staged, 256 gates 0.381 / 0.201)

__device__ __forceinline__ uint32_t ks_mask_word(const KsArgs &a, long g, int p, int i) {   // mask word i of party p of sample g
    const int32_t *u = a.u + (size_t)g * a.rot_per_gate * a.u_rec + (size_t)p * a.u_pstride + i;
    uint32_t v = (uint32_t)u[0];
    if (a.rot_per_gate == 2) v += (uint32_t)u[a.u_rec];
    return v;
}
__device__ __forceinline__ uint32_t ks_b(const KsArgs &a, long g) {   // b of sample g
    const int32_t *u = a.u + (size_t)g * a.rot_per_gate * a.u_rec + a.u_rec - 1;
    uint32_t b = (uint32_t)u[0];
    if (a.rot_per_gate == 2) b += (uint32_t)u[a.u_rec] + (1u << 29);
    return b;
}
// rounding offset of the digits: 2^(32 - (1 + basebit t)), 0 when the digits cover all 32 bits
__device__ __forceinline__ uint32_t ks_prec_offset(int bt) { return bt >= 32 ? 0u : 1u << (31 - bt); }
// word `col` of sample g's partial sum for party p into the zeroed output; the first coordinate range of party 0 adds b at column b_col
__device__ __forceinline__ void ks_emit(const KsArgs &a, long g, int p, bool first, int col, uint32_t v) {
    unsigned int *out = reinterpret_cast<unsigned int *>(a.out) + (size_t)g * a.out_rec;
    if (col == a.b_col && p == 0 && first) v += ks_b(a, g);
    if (col < a.n) {
        atomicAdd(out + (size_t)p * a.n + col, v);
    } else if (col == a.n) {
        atomicAdd(out + (size_t)a.parties * a.n, v);
    }
}

__global__ __launch_bounds__(256) void ks_pad_kernel(const int32_t *__restrict__ src, long rows, int n, int row_words, int32_t *__restrict__ dst) {
    const long r = blockIdx.x;
    if (r >= rows) return;
    for (int q = threadIdx.x; q < row_words; q += 256) dst[r * row_words + q] = q <= n ? src[r * (n + 1) + q] : 0;
}

// ------------------------------------------------------------------------------------------------------
// plain key switch.  grid = (samples, parties, nsplit): block (g, p, s) key-switches coordinates [s N / nsplit, (s + 1) N / nsplit) of
// sample g with party p's key.  Wave w takes coordinates i = w (mod 4); every lane keeps its 4 NX4 + 2 NX2 words of the padded output row
// in registers and issues NX4 16-byte and NX2 8-byte loads per row (n = 630: 640 words).
// ------------------------------------------------------------------------------------------------------
template <int NX4, int NX2>
__global__ __launch_bounds__(256) void ks_plain_kernel(KsArgs a, int nsplit) {
    constexpr int ROW = 64 * (4 * NX4 + 2 * NX2);
    __shared__ uint32_t sA[2048];   // this block's slice of the mask: N / nsplit <= 2048 words (N = 4096 is launched with nsplit >= 2)
    __shared__ uint32_t sRed[3][ROW];
    const long g = blockIdx.x;
    const int p = blockIdx.y;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const uint32_t prec_offset = ks_prec_offset(a.basebit * a.t);
    const int span = a.N / nsplit, i_lo = (int)blockIdx.z * span, i_hi = i_lo + span;
    for (int q = tid; q < span; q += 256) sA[q] = ks_mask_word(a, g, p, i_lo + q) + prec_offset;
    __syncthreads();
    const int base1 = (1 << a.basebit) - 1;
    const uint32_t mask = (uint32_t)base1;
    uint32_t r4[NX4 > 0 ? NX4 : 1][4];
    uint32_t r2[NX2 > 0 ? NX2 : 1][2];
#pragma unroll
    for (int c = 0; c < NX4; c++)
#pragma unroll
        for (int q = 0; q < 4; q++) r4[c][q] = 0;
    r2[0][0] = r2[0][1] = 0;
    const int32_t *kp = a.ksk + (size_t)p * a.N * a.t * base1 * ROW;
    for (int i = i_lo + wave; i < i_hi; i += 4) {
        const uint32_t ai = sA[i - i_lo];
        const int32_t *rowi = kp + (size_t)i * a.t * base1 * ROW;
        for (int j = 0; j < a.t; j++) {
            const uint32_t d = (ai >> (32 - (j + 1) * a.basebit)) & mask;
            if (d == 0) continue;  // wave-uniform
            const int32_t *row = rowi + ((size_t)j * base1 + (d - 1)) * ROW;
#pragma unroll
            for (int c = 0; c < NX4; c++) {
                const uint4 x = *reinterpret_cast<const uint4 *>(row + c * 256 + 4 * lane);
                r4[c][0] -= x.x; r4[c][1] -= x.y; r4[c][2] -= x.z; r4[c][3] -= x.w;
            }
            if (NX2 > 0) {
                const uint2 x = *reinterpret_cast<const uint2 *>(row + NX4 * 256 + 2 * lane);
                r2[0][0] -= x.x; r2[0][1] -= x.y;
            }
        }
    }
    if (wave > 0) {
        uint32_t *red = sRed[wave - 1];
#pragma unroll
        for (int c = 0; c < NX4; c++)
#pragma unroll
            for (int q = 0; q < 4; q++) red[c * 256 + 4 * lane + q] = r4[c][q];
        if (NX2 > 0) {
            red[NX4 * 256 + 2 * lane] = r2[0][0];
            red[NX4 * 256 + 2 * lane + 1] = r2[0][1];
        }
    }
    __syncthreads();
    if (wave == 0) {
        auto emit = [&](int q, uint32_t v) { ks_emit(a, g, p, blockIdx.z == 0, q, v + sRed[0][q] + sRed[1][q] + sRed[2][q]); };
#pragma unroll
        for (int c = 0; c < NX4; c++)
#pragma unroll
            for (int q = 0; q < 4; q++) emit(c * 256 + 4 * lane + q, r4[c][q]);
        if (NX2 > 0) {
            emit(NX4 * 256 + 2 * lane, r2[0][0]);
            emit(NX4 * 256 + 2 * lane + 1, r2[0][1]);
        }
    }
}

// ------------------------------------------------------------------------------------------------------
// staged key switch (from 192 samples on; rows of 512, 640, 768 or 1152 words, basebit 2 or 3, t basebit <= 16).  The plain kernel reads
// 0.75 .. 0.88 rows per sample and (i, j) out of L2 and selects them with branches.  Here a workgroup of eight waves takes 32 samples, one
// party and `span` coordinates; it copies the rows KS[p][i][j][1 .. base-1] of SJ consecutive (i, j) at a time into LDS -- contiguous in
// global memory, double buffered through registers -- and every lane reads its part of the row its sample's digit names (digit 0: a row of
// zeros) with ds_read_b128: the digit selects an address, not a branch, and base-1 rows per (i, j) leave L2 once for 32 samples.  A stage
// may straddle two coordinates, so any t works.  A wave takes FOUR samples, one per 16-lane group of the LDS hardware ({0-3,12-15,20-27},
// {4-11,16-19,28-31} and the same + 32 serve one ds_read_b128 cycle each): the 16 lanes of a group read 16 consecutive pieces of ONE row =
// all 64 banks once, whatever the four digits are.  Partial sums of the coordinate ranges and the parties' parts of b meet in the zeroed
// output with integer atomics.
// ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void ks_sub(uint32_t &r, uint32_t x) { asm("v_sub_u32 %0, %0, %1" : "+v"(r) : "v"(x)); }   // in place, never re-associated
template <int W, int R, int SJ>   // W: 16-byte pieces per lane (row_words = 64 W); R = 2^basebit - 1 rows per (i, j); SJ: (i, j) pairs per stage
__global__ __launch_bounds__(512) void ks_staged_kernel(KsArgs a, int span) {   // span: coordinates per workgroup, <= SPAN
    constexpr int ROW4 = 16 * W, Q = W, GW = 32;
    constexpr int SPAN = R == 3 ? 128 : 64;      // 64 with seven rows per (i, j): the digits of 128 would cost two workgroups per CU their LDS
    constexpr int STAGE4 = SJ * R * ROW4;
    constexpr int NLD = (STAGE4 + 511) / 512;
    constexpr int KS_CHUNK = 3;                  // reads in flight behind the ones being subtracted (measured: 3 <= 5 < 10)
    static_assert(NLD <= 5, "a stage is at most five rounds of 512 pieces");
    __shared__ uint4 sL[ROW4 + 2 * STAGE4];      // [row of zeros][stage 0][stage 1]
    __shared__ uint16_t sDig[GW][SPAN];          // top 16 bits of u + offset: all t digits of a coordinate
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int q5 = lane & 31;
    const int gl = 2 * (lane >> 5) + (int)((0xF00F0FF0u >> q5) & 1u);   // the lane's ds_read_b128 group = its sample within the wave
    const int c = q5 < 4 ? q5 : q5 < 12 ? q5 - 4 : q5 < 20 ? q5 - 8 : q5 < 28 ? q5 - 12 : q5 - 16;   // position in the group: 0 .. 15
    const long g0 = (long)blockIdx.x * GW;
    const int p = blockIdx.y;
    const int first = (int)blockIdx.z * span;
    const uint32_t prec_offset = 1u << (32 - (1 + a.basebit * a.t));
    for (int q = tid; q < GW * span; q += 512) {
        const int g = q / span, ii = q % span;
        uint32_t v = 0;
        if (g0 + g < a.samples) v = ks_mask_word(a, g0 + g, p, first + ii) + prec_offset;
        sDig[g][ii] = (uint16_t)(v >> 16);  // absent samples: all digits zero
    }
    for (int q = tid; q < ROW4; q += 512) sL[q] = uint4{0u, 0u, 0u, 0u};
    const uint4 *src = reinterpret_cast<const uint4 *>(a.ksk) + ((size_t)p * a.N + first) * a.t * R * ROW4;
    const int NS = span * a.t / SJ;
    // stage st of the key: SJ R contiguous rows; thread tid moves pieces tid + 512 k (a partial last round reads a clamped index and stores
    // nothing).  Named scalars: as arrays behind an unrolled loop the pieces stayed in scratch memory.
    uint4 pre0, pre1 = uint4{0u, 0u, 0u, 0u}, pre2 = pre1, pre3 = pre1, pre4 = pre1;
    const bool last_ok = 512 * NLD <= STAGE4 || tid + 512 * (NLD - 1) < STAGE4;
    const int last_idx = last_ok ? tid + 512 * (NLD - 1) : STAGE4 - 1;
#define KS_GLOAD(st)                                              \
    {                                                             \
        const uint4 *p_ = src + (size_t)(st) * STAGE4;            \
        pre0 = p_[NLD == 1 ? last_idx : tid];                     \
        if (NLD > 1) pre1 = p_[NLD == 2 ? last_idx : tid + 512];  \
        if (NLD > 2) pre2 = p_[NLD == 3 ? last_idx : tid + 1024]; \
        if (NLD > 3) pre3 = p_[NLD == 4 ? last_idx : tid + 1536]; \
        if (NLD > 4) pre4 = p_[last_idx];                         \
    }
#define KS_LSTORE(buf)                                            \
    {                                                             \
        uint4 *d_ = sL + ROW4 + (buf) * STAGE4 + tid;             \
        if (NLD > 1 || last_ok) d_[0] = pre0;                     \
        if (NLD > 2 || (NLD == 2 && last_ok)) d_[512] = pre1;     \
        if (NLD > 3 || (NLD == 3 && last_ok)) d_[1024] = pre2;    \
        if (NLD > 4 || (NLD == 4 && last_ok)) d_[1536] = pre3;    \
        if (NLD == 5 && last_ok) d_[2048] = pre4;                 \
    }
    KS_GLOAD(0)
    KS_LSTORE(0)
    __syncthreads();
    uint4 acc[Q];
#pragma unroll
    for (int k = 0; k < Q; k++) acc[k] = uint4{0u, 0u, 0u, 0u};
    const uint16_t *dig = sDig[wave * 4 + gl];
    const uint32_t dmask = (uint32_t)R;
    int ii0 = 0, j0 = 0;   // coordinate and level of the stage's first pair
    for (int st = 0; st < NS; st++) {
        if (st + 1 < NS) {
            KS_GLOAD(st + 1)
        }
        const uint4 *row[SJ];
#pragma unroll
        for (int pp = 0; pp < SJ; pp++) {
            int ii = ii0, j = j0 + pp;
            while (j >= a.t) j -= a.t, ii++;
            const uint32_t d = ((uint32_t)dig[ii] >> (16 - (j + 1) * a.basebit)) & dmask;
            row[pp] = sL + (d ? ROW4 + (st & 1) * STAGE4 + (pp * R + (int)d - 1) * ROW4 : 0) + c;
        }
        j0 += SJ;
        while (j0 >= a.t) j0 -= a.t, ii0++;
        // KS_CHUNK reads in flight behind the KS_CHUNK being subtracted -- not all of a stage: the memory fence stops the optimiser, the
        // scheduling barrier the instruction scheduler from clustering them
        constexpr int NCH = (Q + KS_CHUNK - 1) / KS_CHUNK;
        uint4 x[2][KS_CHUNK];
        auto reads = [&](int ch) {   // ch < SJ * NCH, compile-time after unrolling
            const uint4 *r = row[ch / NCH];
            const int k0 = (ch % NCH) * KS_CHUNK;
#pragma unroll
            for (int k = 0; k < KS_CHUNK; k++)
                if (k0 + k < Q) x[ch & 1][k] = r[16 * (k0 + k)];
        };
        reads(0);
#pragma unroll
        for (int ch = 0; ch < SJ * NCH; ch++) {
            if (ch + 1 < SJ * NCH) reads(ch + 1);
            asm volatile("" ::: "memory");
            __builtin_amdgcn_sched_barrier(0);
            const int k0 = (ch % NCH) * KS_CHUNK;
#pragma unroll
            for (int k = 0; k < KS_CHUNK; k++)
                if (k0 + k < Q) {
                    uint4 &t = acc[k0 + k];
                    const uint4 v = x[ch & 1][k];
                    ks_sub(t.x, v.x), ks_sub(t.y, v.y), ks_sub(t.z, v.z), ks_sub(t.w, v.w);
                }
            __builtin_amdgcn_sched_barrier(0);
        }
        if (st + 1 < NS) {
            KS_LSTORE((st + 1) & 1)
        }
        __syncthreads();
    }
#undef KS_GLOAD
#undef KS_LSTORE
    const long g = g0 + wave * 4 + gl;
    if (g < a.samples) {
#pragma unroll
        for (int k = 0; k < Q; k++) {
            const uint32_t v4[4] = {acc[k].x, acc[k].y, acc[k].z, acc[k].w};
#pragma unroll
            for (int e = 0; e < 4; e++) ks_emit(a, g, p, blockIdx.z == 0, 4 * (c + 16 * k) + e, v4[e]);
        }
    }
}

// ------------------------------------------------------------------------------------------------------
// key switch on the matrix cores (ks_basebit == 2, t = 4 or 8, large batches).  The key switch is an exact integer GEMM:
//   out[g] = (0, .., 0, b) - sum_k A[g][k] B[k],   k = (i, j, v): coordinate i < N, level j < t, digit value v < 4,
// A one-hot (A[g][(i, j, v)] = [digit j of coordinate i of gate g == v]) and B[(i, j, v)] = KS[i][j][v - 1], with a row of zeros for v = 0.
// Every 32-bit key word is split into four balanced signed bytes, w = sum_p beta_p 2^(8p) (mod 2^32), beta_p in [-128, 127], so B becomes four
// int8 planes and C_p = A B_p is a v_mfma_i32_32x32x32_i8 product: |C_p| <= N t 128 = 2^20, and out = b - sum_p C_p << 8p, all mod 2^32.
// Integer sums commute, so tiling, split-K and the atomics cannot change a bit.
//
// K chunks of 32 = 8 (i, j) slots x 4 values: slot s = 8 kc + 4 h + q of the chunk kc is held by the lanes of half h = lane >> 5 in the
// fragment dword q, value v in byte v.  A and B fragments use that one convention, and an MFMA pairs element e of lane half h of A with
// element e of the same lane half of B, so the product is the sum over the chunk whatever order the hardware gives the 32 k of a chunk.
// Planes: [word tile wt][chunk kc][plane p][lane][4 dwords], a 1 KB B fragment per (wt, kc, p); lane r + 32 h holds word 32 wt + r.
// ------------------------------------------------------------------------------------------------------
typedef int32_t ks_i32x4 __attribute__((ext_vector_type(4)));
typedef int32_t ks_i32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ uint32_t ks_balanced_byte(uint32_t w, int p) {   // beta_p of w, as a byte
    for (int k = 0; k < p; k++) w = (w - (uint32_t)(int32_t)(int8_t)(w & 0xFFu)) >> 8;
    return w & 0xFFu;
}

__global__ __launch_bounds__(256) void sk_ksk_planes_kernel(const int32_t *__restrict__ ksk, int row_words, int t, long kchunks, long total,
                                                             uint32_t *__restrict__ planes) {
    const long x = (long)blockIdx.x * 256 + threadIdx.x;   // one dword of the planes
    if (x >= total) return;
    const int q = (int)(x & 3), lane = (int)((x >> 2) & 63), p = (int)((x >> 8) & 3);
    const long kc = (x >> 10) % kchunks, wt = (x >> 10) / kchunks;
    const long s = 8 * kc + 4 * (lane >> 5) + q, i = s / t, j = s % t;
    const int32_t *row = ksk + ((i * t + j) * 3) * row_words + 32 * wt + (lane & 31);
    uint32_t dw = 0;
    for (int v = 1; v < 4; v++) dw |= ks_balanced_byte((uint32_t)row[(v - 1) * row_words], p) << (8 * v);
    planes[x] = dw;
}

struct KSMArgs {
    const ks_i32x4 *planes;   // [wtiles][kchunks][4][64]
    const int32_t *u;         // [jobs][u_rec]: N mask words, b last
    int32_t *out;             // [gates][out_rec]
    long gates;
    int u_rec, out_rec, b_col;   // KsArgs::u_rec, ::out_rec, ::b_col
    int rot_per_gate;         // 1, or 2 for MUX: input = (0, 2^29) + u1 + u2
    int n, t;
    int kchunks;              // N t / 8
    int wtiles;               // 32-word tiles of a padded row
    int gtiles;               // 256-gate tiles
    int nsplit;               // > 1: the chunks are cut in nsplit ranges whose partial sums meet in the zeroed output with atomics
};

// One workgroup: 256 gates (4 waves x 2 tiles of 32) x one 32-word tile (4 planes) x one chunk range.  The planes of KS_S chunks (32 KB) are
// staged in LDS per step (double buffered through registers) and read by all four waves; each wave builds its A fragments from the digits of
// its gates, and keeps 2 x 4 accumulators of 32 x 32 int32.
template <int T, int ROT>   // key-switch depth: 4 or 8; rotations per gate: 1, or 2 for MUX (a.rot_per_gate)
__global__ __launch_bounds__(256) void sk_keyswitch_mfma_kernel(KSMArgs a) {
    static_assert(T == 4 || T == 8, "a lane half's four slots are four levels of one coordinate");
    constexpr int S = 8;                  // chunks per stage
    constexpr int NLD = S * 4 * 64 / 256; // 16-byte pieces per thread and stage
    __shared__ ks_i32x4 sB[2][S * 4 * 64];
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int r = lane & 31, h = lane >> 5;
    // workgroups are dealt round-robin over the 8 XCDs: renumber them so that the gate tiles of one (word tile, chunk range) share an XCD's L2
    long L = blockIdx.x;
    const long nblk = gridDim.x;
    if (nblk % 8 == 0) L = (L % 8) * (nblk / 8) + L / 8;
    const int gt = (int)(L % a.gtiles), wt = (int)(L / a.gtiles % a.wtiles), sp = (int)(L / a.gtiles / a.wtiles);
    const int kper = a.kchunks / a.nsplit, kc0 = sp * kper, NS = kper / S;
    const ks_i32x4 *src = a.planes + ((size_t)wt * a.kchunks + kc0) * 256;
    const uint32_t prec_offset = 1u << (32 - (1 + 2 * T));
    // the lane's A rows: gates g0 + 32 m + r
    const long g0 = (long)gt * 256 + wave * 64;
    // (rows past the batch read the last gate's digits and store nothing: no branch around the loads, whose waits would serialise them)
    const int32_t *urow[2];
#pragma unroll
    for (int m = 0; m < 2; m++) {
        const long g = g0 + 32 * m + r;
        urow[m] = a.u + (size_t)(g < a.gates ? g : a.gates - 1) * ROT * a.u_rec;
    }
    // chunk kc: the lane's four slots 8 kc + 4 h + q are levels j0 .. j0 + 3 of one coordinate (t is a multiple of 4)
    auto coord = [&](int kc) { return T == 8 ? kc : 2 * kc + h; };
    const int j0 = T == 8 ? 4 * h : 0;
    ks_i32x4 pre[NLD];
    uint32_t uw[2][S], un[2][S];
    auto load = [&](int st) {
        const ks_i32x4 *p_ = src + (size_t)st * (S * 256) + tid;
#pragma unroll
        for (int k = 0; k < NLD; k++) pre[k] = p_[256 * k];
#pragma unroll
        for (int m = 0; m < 2; m++)
#pragma unroll
            for (int c = 0; c < S; c++) {
                const int i = coord(kc0 + st * S + c);
                un[m][c] = (uint32_t)urow[m][i];
                if (ROT == 2) un[m][c] += (uint32_t)urow[m][a.u_rec + i];
            }
    };
    auto store = [&](int buf) {
#pragma unroll
        for (int k = 0; k < NLD; k++) sB[buf][tid + 256 * k] = pre[k];
#pragma unroll
        for (int m = 0; m < 2; m++)
#pragma unroll
            for (int c = 0; c < S; c++) uw[m][c] = un[m][c] + prec_offset;   // (here, not in load(): the add would wait for the loads)
    };
    load(0);
    store(0);
    __syncthreads();
    ks_i32x16 acc[2][4];
#pragma unroll
    for (int m = 0; m < 2; m++)
#pragma unroll
        for (int p = 0; p < 4; p++) acc[m][p] = ks_i32x16{0};
    for (int st = 0; st < NS; st++) {
        if (st + 1 < NS) load(st + 1);
        const ks_i32x4 *b = sB[st & 1] + lane;
        ks_i32x4 bf[2][4];   // the B fragments of chunk c + 1 are read while chunk c's MFMAs run
#pragma unroll
        for (int p = 0; p < 4; p++) bf[0][p] = b[p * 64];
#pragma unroll
        for (int c = 0; c < S; c++) {
            if (c + 1 < S)
#pragma unroll
                for (int p = 0; p < 4; p++) bf[(c + 1) & 1][p] = b[((c + 1) * 4 + p) * 64];
            ks_i32x4 af[2];
#pragma unroll
            for (int m = 0; m < 2; m++)
#pragma unroll
                for (int q = 0; q < 4; q++) af[m][q] = (int32_t)(1u << (8 * ((uw[m][c] >> (30 - 2 * (j0 + q))) & 3u)));   // digit 0: the zero row
#pragma unroll
            for (int m = 0; m < 2; m++)
#pragma unroll
                for (int p = 0; p < 4; p++) acc[m][p] = __builtin_amdgcn_mfma_i32_32x32x32_i8(af[m], bf[c & 1][p], acc[m][p], 0, 0, 0);
        }
        if (st + 1 < NS) store((st + 1) & 1);
        __syncthreads();
    }
    // C/D: lane r + 32 h, register e holds row (e & 3) + 8 (e >> 2) + 4 h, column r
    const int col = 32 * wt + r;
    if (col >= a.out_rec) return;
#pragma unroll
    for (int m = 0; m < 2; m++)
#pragma unroll
        for (int e = 0; e < 16; e++) {
            const long g = g0 + 32 * m + (e & 3) + 8 * (e >> 2) + 4 * h;
            if (g >= a.gates) continue;
            uint32_t v = 0u - ((uint32_t)acc[m][0][e] + ((uint32_t)acc[m][1][e] << 8) + ((uint32_t)acc[m][2][e] << 16) + ((uint32_t)acc[m][3][e] << 24));
            if (col == a.b_col && sp == 0) {
                const int32_t *u1 = a.u + (size_t)g * ROT * a.u_rec;
                v += (uint32_t)u1[a.u_rec - 1];
                if (ROT == 2) v += (uint32_t)u1[2 * a.u_rec - 1] + (1u << 29);
            }
            unsigned int *o = reinterpret_cast<unsigned int *>(a.out) + (size_t)g * a.out_rec + col;
            if (a.nsplit == 1) *o = v;
            else atomicAdd(o, v);
        }
}

// ------------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------------

// The key-switching key of a context: rows KS[p][i][j][v - 1] of n + 1 words padded to row_words = the next multiple of 128 (whole 16-byte
// pieces, an even number of words per lane), and for a single-key context of the matrix-core shape also the int8 planes of
// sk_keyswitch_mfma_kernel (4 bytes per (word, coordinate, level, digit value): 80 MiB at n = 630, t = 8).
struct KsKey {
    DevBuf rows, planes;
    int n = 0, t = 0, basebit = 0, parties = 0, N = 0, row_words = 0;
    bool single = false;   // single-key engine: the matrix-core kernel and its coordinate span rule

    // upload `ksk` ([parties][N][t][base-1][n+1] words) and pad it; returns when the key is on the device
    int upload(const int32_t *ksk, int parties_, int N_, int n_, int t_, int basebit_, bool single_, hipStream_t s) {
        n = n_, t = t_, basebit = basebit_, parties = parties_, N = N_, single = single_;
        row_words = 128 * ((n + 1 + 127) / 128);
        const long nrows = (long)parties * N * t * ((1 << basebit) - 1);
        DevBuf raw;  // upload staging
        THFHE_TRY(raw.grow((size_t)nrows * (n + 1) * sizeof(int32_t)));
        THFHE_HIP(hipMemcpyAsync(raw.as<int32_t>(), ksk, (size_t)nrows * (n + 1) * sizeof(int32_t), hipMemcpyHostToDevice, s));
        THFHE_TRY(rows.grow((size_t)nrows * row_words * sizeof(int32_t)));
        hipLaunchKernelGGL(ks_pad_kernel, dim3((unsigned)nrows), dim3(256), 0, s, raw.as<int32_t>(), nrows, n, row_words, rows.as<int32_t>());
        THFHE_HIP(hipGetLastError());
        if (single && basebit == 2 && (t == 4 || t == 8) && N == 1024) THFHE_TRY(build_planes(s));   // the shapes sk_keyswitch_mfma_kernel takes
        THFHE_HIP(hipStreamSynchronize(s));   // before `raw` is freed
        return THFHE_OK;
    }

    // The LWE -> TLWE packing key ([n_lwe][t][base-1][2 N_ring] words: TLWE samples (alpha, beta)) as a single-key table: rows of
    // row_words = 2 N_ring, output "dimension" n = 2 N_ring (b is added at word N_ring: KsArgs::b_col), input coordinates padded with rows
    // of zeros to N = n_pad, a multiple of 128 -- the matrix-core kernel's chunking (and the plain kernel's coordinate ranges) need it, and a
    // zero mask word past n_lwe has only zero digits.  Planes for 2-bit digits, t = 4 or 8.  Replaces any earlier key; on failure the key
    // is left empty (n = 0).
    int upload_pack(const int32_t *pk, int n_lwe, int t_, int basebit_, int N_ring, hipStream_t s) {
        n = 0;
        planes = DevBuf();
        const int n_pad = 128 * ((n_lwe + 127) / 128);
        const size_t per_coord = (size_t)t_ * ((1 << basebit_) - 1) * 2 * N_ring;   // words of one coordinate's rows
        THFHE_TRY(rows.grow((size_t)n_pad * per_coord * sizeof(int32_t)));
        THFHE_HIP(hipMemcpyAsync(rows.as<int32_t>(), pk, (size_t)n_lwe * per_coord * sizeof(int32_t), hipMemcpyHostToDevice, s));
        if (n_pad > n_lwe)
            THFHE_HIP(hipMemsetAsync(rows.as<int32_t>() + (size_t)n_lwe * per_coord, 0, (size_t)(n_pad - n_lwe) * per_coord * sizeof(int32_t), s));
        t = t_, basebit = basebit_, parties = 1, N = n_pad, row_words = 2 * N_ring, single = true;
        if (basebit == 2 && (t == 4 || t == 8)) THFHE_TRY(build_planes(s));
        THFHE_HIP(hipStreamSynchronize(s));   // before the caller's host key may go
        n = 2 * N_ring;
        return THFHE_OK;
    }

    // the int8 planes of sk_keyswitch_mfma_kernel from the padded rows (N t / 8 chunks: a multiple of 64 for N = 1024 and for N % 128 == 0)
    int build_planes(hipStream_t s) {
        const long kchunks = (long)N * t / 8, total = (long)(row_words / 32) * kchunks * 4 * 64 * 4;
        THFHE_TRY(planes.grow((size_t)total * sizeof(uint32_t)));
        hipLaunchKernelGGL(sk_ksk_planes_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, rows.as<int32_t>(), row_words, t, kchunks,
                           total, planes.as<uint32_t>());
        THFHE_HIP(hipGetLastError());
        return THFHE_OK;
    }

    // the arguments of a key switch of `samples` records of N + 1 words, one rotation each; CCS / KMS layouts, the MUX combine and the
    // packing key set their fields
    KsArgs args(const int32_t *u, int32_t *out, long samples) const {
        return KsArgs{rows.as<int32_t>(), u, out, samples, n, t, basebit, parties, row_words, N, N + 1, 0, 1, parties * n + 1, n};
    }
};

// the key switch of a.samples samples into a.out: matrix cores where the key has planes (from mfma_min samples on), else the staged
// kernel where its shape allows, else the plain kernel with the coordinates cut into nsplit_plain ranges (N / nsplit_plain <= 2048).
// Zeroes a.out where the kernel accumulates into it.
inline int ks_enqueue(const KsKey &key, const KsArgs &a, int nsplit_plain, hipStream_t stream, long mfma_min = kKsMfmaMinSamples) {
    const size_t out_bytes = (size_t)a.samples * a.out_rec * sizeof(int32_t);
    if (key.planes.bytes() && a.samples >= mfma_min) {
        // 256-gate x 32-word tiles; the chunks are cut into nsplit ranges until the grid has at least 1 024 workgroups (4 096 gates, n = 630: 16 x 20 x 4)
        KSMArgs k{key.planes.as<ks_i32x4>(), a.u, a.out, a.samples, a.u_rec, a.out_rec, a.b_col, a.rot_per_gate, a.n, a.t, a.N * a.t / 8, a.row_words / 32,
                  (int)((a.samples + 255) / 256), 1};
        while (k.nsplit < 8 && (long)k.gtiles * k.wtiles * k.nsplit < 1024) k.nsplit *= 2;
        if (k.nsplit > 1) THFHE_HIP(hipMemsetAsync(a.out, 0, out_bytes, stream));
        const dim3 grid((unsigned)((long)k.gtiles * k.wtiles * k.nsplit)), block(256);
        if (a.t == 8) {
            if (a.rot_per_gate == 1) hipLaunchKernelGGL((sk_keyswitch_mfma_kernel<8, 1>), grid, block, 0, stream, k);
            else hipLaunchKernelGGL((sk_keyswitch_mfma_kernel<8, 2>), grid, block, 0, stream, k);
        } else {
            if (a.rot_per_gate == 1) hipLaunchKernelGGL((sk_keyswitch_mfma_kernel<4, 1>), grid, block, 0, stream, k);
            else hipLaunchKernelGGL((sk_keyswitch_mfma_kernel<4, 2>), grid, block, 0, stream, k);
        }
        THFHE_HIP(hipGetLastError());
        return THFHE_OK;
    }
    THFHE_HIP(hipMemsetAsync(a.out, 0, out_bytes, stream));
    // staged: ranges of 64 coordinates with 3-bit digits; with 2-bit digits the single key cuts its coordinates into 16 ranges (8 from
    // 2 048 gates on: measured), the multi key into ranges of 128
    const int span = a.basebit == 3 || (key.single && a.samples < 2048) ? 64 : 128;
    const bool staged = (a.row_words == 512 || a.row_words == 640 || a.row_words == 768 || (a.row_words == 1152 && a.basebit == 2)) &&
                        (a.basebit == 2 || a.basebit == 3) && a.t * a.basebit <= 16 && a.N % span == 0;
    if (staged && a.samples >= kKsStagedMinSamples) {
        // stage depth by LDS: two stages + the row of zeros + the digits stay under half a CU's LDS (two workgroups per CU)
        const dim3 grid((unsigned)((a.samples + 31) / 32), (unsigned)a.parties, (unsigned)(a.N / span)), block(512);
        const bool b2 = a.basebit == 2;
        if (a.row_words == 512) {
            if (b2) hipLaunchKernelGGL((ks_staged_kernel<8, 3, 4>), grid, block, 0, stream, a, span);
            else hipLaunchKernelGGL((ks_staged_kernel<8, 7, 2>), grid, block, 0, stream, a, span);
        } else if (a.row_words == 640) {
            if (b2) hipLaunchKernelGGL((ks_staged_kernel<10, 3, 4>), grid, block, 0, stream, a, span);
            else hipLaunchKernelGGL((ks_staged_kernel<10, 7, 2>), grid, block, 0, stream, a, span);
        } else if (a.row_words == 768) {
            if (b2) hipLaunchKernelGGL((ks_staged_kernel<12, 3, 2>), grid, block, 0, stream, a, span);
            else hipLaunchKernelGGL((ks_staged_kernel<12, 7, 1>), grid, block, 0, stream, a, span);
        } else {
            hipLaunchKernelGGL((ks_staged_kernel<18, 3, 2>), grid, block, 0, stream, a, span);
        }
        THFHE_HIP(hipGetLastError());
        return THFHE_OK;
    }
    if (a.N / nsplit_plain > 2048) return thfhe_fail(THFHE_E_UNSUPPORTED, "key switch: more than 2048 coordinates per workgroup");
    const dim3 grid((unsigned)a.samples, (unsigned)a.parties, (unsigned)nsplit_plain), block(256);
    switch (a.row_words / 64) {
#define THFHE_KS_CASE(W, X4, X2) \
    case W: hipLaunchKernelGGL((ks_plain_kernel<X4, X2>), grid, block, 0, stream, a, nsplit_plain); break;
        THFHE_KS_CASE(2, 0, 1) THFHE_KS_CASE(4, 1, 0) THFHE_KS_CASE(6, 1, 1) THFHE_KS_CASE(8, 2, 0) THFHE_KS_CASE(10, 2, 1)
        THFHE_KS_CASE(12, 3, 0) THFHE_KS_CASE(14, 3, 1) THFHE_KS_CASE(16, 4, 0) THFHE_KS_CASE(18, 4, 1) THFHE_KS_CASE(20, 5, 0)
        THFHE_KS_CASE(22, 5, 1) THFHE_KS_CASE(32, 8, 0)   // 32: the packing key's rows of 2N = 2048 words
#undef THFHE_KS_CASE
    default: return thfhe_fail(THFHE_E_UNSUPPORTED, "LWE dimension n too large for the key-switch kernel (n <= 1407)");
    }
    THFHE_HIP(hipGetLastError());
    return THFHE_OK;
}

}  // namespace

#endif  // THFHE_KEYSWITCH_H
