// thfhe_cb.h -- the private functional key switch of circuit bootstrapping: LWE samples under the level-2 ring key
// z2 (dimension D <= 2048) -> the TLWE rows of a TGSW sample under the level-1 ring key z (N = 1024).  Device-pointer level: the key
// (CbKey), the kernels and the launcher (cb_enqueue); the context-level calls are in thfhe_cb_host.h.
//
//   key    int32[2][D][t][2][N]: row (f, i, p) a TLWE encryption of zero under z, with z2[i] 2^(32 - (p+1) basebit) added to coefficient 0
//          of the body (f = 1) or of the mask (f = 0).  Rows are NOT tabulated per digit value: the signed digit multiplies the row.
//   input  g = sample * l + level: int32[D + 1] = (a, b)
//   output T_f(g) = e_f(b) - sum_(i, p) d_(i, p)(a_i) K[f][i][p],  e_1(b) = (0, b X^0), e_0(b) = (b X^0, 0); T_0 is row `level` and T_1 row
//          l + level of the sample's int32[2l][2][N]: the layout of thfhe_tgsw_set_create.
//   digits d_(i, p) in [-B/2, B/2), B = 2^basebit: the balanced base-B digits of a_i rounded to t basebit bits,
//          sum_p d_p 2^(32 - (p+1) basebit) = round(a_i) mod 2^32 (cb_digit; tests/cb_reference.py states the same rule with carries).
//
//   cb_pks_plain_kernel   one workgroup per (input, range of (i, p)): digits once into LDS, both functions in one pass, the 4096 output
//                         words in registers (16 per lane); reads 2 D t 8 KiB of key per input
//   cb_digits_kernel      the digits of a batch as an int8 matrix A[input][K], K = D t padded to a multiple of 128
//   cb_planes_kernel      the key as four balanced byte planes in MFMA B-fragment order (sk_keyswitch_mfma_kernel's split of a word)
//   cb_pks_mfma_kernel    out = e(b) - sum_plane (A B_plane) << 8 plane: the exact int8 GEMM of sk_keyswitch_mfma_kernel with a digit-valued A.
//                         256 inputs x 32 words per workgroup, so a key byte leaves memory once per 256 inputs.
//                         |C_plane| <= D t 2^(basebit-1) 128 <= 2^27 (D = 2048, t = 4, basebit = 8) < 2^31.
//   cb_extract_levels_kernel   stage A in one-rotation mode: the l records of a bit from ONE accumulator, its mask polynomial staged in LDS
//
// Integer sums commute: kernel, split and summation order cannot change a word.
#ifndef THFHE_CB_H
#define THFHE_CB_H

#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/thfhe_hip.h"
#include "thfhe_common.h"
#include "thfhe_devctx.h"
#include "thfhe_keyswitch.h"
#include "thfhe_lane.h"

namespace {
using namespace thfhe;

constexpr int kCbMaxD = 2048;           // input dimension: the level-2 ring degree, or less (tests)
constexpr int kCbRow = 2048;            // words of a key row: a TLWE sample of the N = 1024 ring (mask, body)
constexpr int kCbCols = 2 * kCbRow;     // output words per input: both functions
constexpr int kCbPlainSpan = 16384;     // (i, p) pairs per workgroup of the plain kernel at most: its digits live in LDS
constexpr int kCbStage = 128;           // (i, p) pairs per LDS stage of the MFMA kernel: 4 chunks of 32
constexpr long kCbBatchMinInputs = 3;   // inputs from which cb_enqueue takes the MFMA kernel (measured, D = 2048, t = 7: 3 inputs 0.141 ms plain / 0.089 MFMA, 192 inputs 3.06 / 0.149; fewer than 3 not measured)

// what is added to a mask word before its digits are cut: the rounding bit 2^(31 - t basebit) (nothing when the digits cover all 32 bits) and
// B/2 at every digit position, so that digit p is ((word + offset) >> (32 - (p+1) basebit) & (B - 1)) - B/2 with the carries already in place
__host__ __device__ inline uint32_t cb_digit_offset(int t, int basebit) {
    const int bt = t * basebit;
    uint32_t off = bt < 32 ? 1u << (31 - bt) : 0u;
    for (int p = 0; p < t; p++) off += 1u << (31 - p * basebit);
    return off;
}
__device__ __forceinline__ int cb_digit(uint32_t v, int p, int basebit) {   // v = mask word + cb_digit_offset
    return (int)((v >> (32 - (p + 1) * basebit)) & ((1u << basebit) - 1u)) - (1 << (basebit - 1));
}

struct CbArgs {
    const int32_t *key;   // [2][D][t][2048]
    const int32_t *in;    // [inputs][D + 1]
    int32_t *out;         // [inputs / l][2l][2048]
    long inputs;
    int D, t, basebit, l;
};
// first word of row T_f of input g
__device__ __forceinline__ size_t cb_out_row(long g, int f, int l) { return ((size_t)(g / l) * 2 * l + (size_t)f * l + (size_t)(g % l)) * kCbRow; }
// b lands on coefficient 0 of the body of T_1 and of the mask of T_0
__device__ __forceinline__ bool cb_b_word(int f, int w) { return f ? w == kCbRow / 2 : w == 0; }

// grid = (inputs, nsplit): workgroup (g, z) takes the pairs k = i t + p in [z kspan, (z + 1) kspan) of input g; lane `tid` holds words
// 4 tid .. 4 tid + 3 of the mask and of the body of both rows.  nsplit > 1: the partial sums meet in the zeroed output with atomics.
__global__ __launch_bounds__(256) void cb_pks_plain_kernel(CbArgs a, int kspan, int nsplit) {
    __shared__ int8_t sDig[kCbPlainSpan];
    const long g = blockIdx.x;
    const int z = blockIdx.y, tid = threadIdx.x;
    const int K = a.D * a.t, k0 = z * kspan, k1 = min(K, k0 + kspan);
    const uint32_t off = cb_digit_offset(a.t, a.basebit);
    const int32_t *in = a.in + (size_t)g * (a.D + 1);
    for (int k = k0 + tid; k < k1; k += 256) {
        const int i = k / a.t, p = k - i * a.t;
        sDig[k - k0] = (int8_t)cb_digit((uint32_t)in[i] + off, p, a.basebit);
    }
    __syncthreads();
    uint32_t acc[2][2][4];
#pragma unroll
    for (int f = 0; f < 2; f++)
#pragma unroll
        for (int c = 0; c < 2; c++)
#pragma unroll
            for (int e = 0; e < 4; e++) acc[f][c][e] = 0u;
    const int32_t *row0 = a.key + (size_t)k0 * kCbRow + 4 * tid;
    const size_t fstride = (size_t)K * kCbRow;
    for (int k = k0; k < k1; k++, row0 += kCbRow) {
        const int d = __builtin_amdgcn_readfirstlane((int)sDig[k - k0]);
        if (d == 0) continue;
        const uint32_t ud = (uint32_t)d;
#pragma unroll
        for (int f = 0; f < 2; f++)
#pragma unroll
            for (int c = 0; c < 2; c++) {
                const uint4 x = *reinterpret_cast<const uint4 *>(row0 + f * fstride + c * (kCbRow / 2));
                acc[f][c][0] -= ud * x.x, acc[f][c][1] -= ud * x.y, acc[f][c][2] -= ud * x.z, acc[f][c][3] -= ud * x.w;
            }
    }
    const uint32_t b = (uint32_t)in[a.D];
#pragma unroll
    for (int f = 0; f < 2; f++) {
        unsigned int *o = reinterpret_cast<unsigned int *>(a.out) + cb_out_row(g, f, a.l);
#pragma unroll
        for (int c = 0; c < 2; c++)
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const int w = c * (kCbRow / 2) + 4 * tid + e;
                uint32_t v = acc[f][c][e];
                if (z == 0 && cb_b_word(f, w)) v += b;
                if (nsplit == 1) o[w] = v;
                else atomicAdd(o + w, v);
            }
    }
}

// grid = (kpad / 256, inputs): dig[g][k] = digit p of mask word i of input g, k = i t + p; zero for k >= D t
__global__ __launch_bounds__(256) void cb_digits_kernel(const int32_t *__restrict__ in, int D, int t, int basebit, int kpad, int8_t *__restrict__ dig) {
    const long g = blockIdx.y;
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= kpad) return;
    int d = 0;
    if (k < D * t) {
        const int i = k / t, p = k - i * t;
        d = cb_digit((uint32_t)in[(size_t)g * (D + 1) + i] + cb_digit_offset(t, basebit), p, basebit);
    }
    dig[(size_t)g * kpad + k] = (int8_t)d;
}

// grid = (ceil((D + 1) / 256), records): the extracted record x[r] of gadget level `level` into its place lwe2[r][level], `add` on the body
// (stage A of circuit bootstrapping: +-mu_j becomes 0 or g_j)
__global__ __launch_bounds__(256) void cb_place_kernel(const int32_t *__restrict__ x, int D, int l, int level, uint32_t add, int32_t *__restrict__ lwe2) {
    const long r = blockIdx.y;
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q > D) return;
    uint32_t v = (uint32_t)x[(size_t)r * (D + 1) + q];
    if (q == D) v += add;
    lwe2[((size_t)r * l + level) * (D + 1) + q] = (int32_t)v;
}

// Stage A in one-rotation mode ("one rotation per bit"): grid = bits, one workgroup per bit.  acc int64[bits][2][D] holds the rotated
// accumulators of a test vector with mu_j at every coefficient q = j mod theta; record (bit, j), j < l, of lwe2[bits][l][D + 1] is
// mk_extract_at_kernel's extraction at coefficient j -- a'_i = t64tot32(a_{j-i}) for i <= j, t64tot32(-a_{D+j-i}) for i > j, negated mod 2^64
// before the conversion -- with `2^(31 - (j+1) Bgbit)` added to the body.  The mask polynomial is read once, 16 bytes per lane, into LDS (8 D
// bytes); the l records read it from there: lane i of a wave takes word (j - i) mod D, 64 consecutive 8-byte words in descending order, one bank
// row per half wave, conflict-free.  A record starts (bit l + j)(D + 1) words into lwe2, which is 4-byte aligned and no more: the stores are one
// dword per lane, 64 consecutive dwords per wave.  D is a power of two, 512 <= D <= kCbMaxD (cb_extract_levels checks it).
__global__ __launch_bounds__(256) void cb_extract_levels_kernel(const int64_t *__restrict__ acc, int D, int l, int Bgbit, int32_t *__restrict__ lwe2) {
    __shared__ __attribute__((aligned(16))) int64_t sMask[kCbMaxD];
    const long bit = blockIdx.x;
    const int tid = threadIdx.x;
    const int64_t *ap = acc + (size_t)bit * 2 * D;
    for (int q = 2 * tid; q < D; q += 512) *reinterpret_cast<longlong2 *>(sMask + q) = *reinterpret_cast<const longlong2 *>(ap + q);
    __syncthreads();
    for (int j = 0; j < l; j++) {
        uint32_t *o = reinterpret_cast<uint32_t *>(lwe2) + ((size_t)bit * l + j) * ((size_t)D + 1);
        for (int q = tid; q < D; q += 256) {
            const int64_t v = sMask[(j - q) & (D - 1)];
            o[q] = (uint32_t)t64tot32(q > j ? (int64_t)(0ull - (uint64_t)v) : v);
        }
        if (tid == 0) o[D] = (uint32_t)t64tot32(ap[D + j]) + (1u << (31 - (j + 1) * Bgbit));
    }
}

// Planes: [word tile wt < 128][stage st][chunk c < 4][plane < 4][lane][4 dwords]: a 1 KiB B fragment per (wt, st, c, plane).  Byte v of dword q of
// lane r + 32 h is plane byte `plane` of key word (k, column 32 wt + r), k = 128 st + 64 h + 16 c + 4 q + v -- a lane half's 64 pairs of a stage are
// contiguous in k, so a lane of the MFMA kernel reads its A fragments of a stage as 64 consecutive digit bytes.  Column = f 2048 + word of row.
__global__ __launch_bounds__(256) void cb_planes_kernel(const int32_t *__restrict__ key, int K, long nstages, long total, uint32_t *__restrict__ planes) {
    const long x = (long)blockIdx.x * 256 + threadIdx.x;   // one dword of the planes
    if (x >= total) return;
    const int q = (int)(x & 3), lane = (int)((x >> 2) & 63), plane = (int)((x >> 8) & 3), c = (int)((x >> 10) & 3);
    const long st = (x >> 12) % nstages, wt = (x >> 12) / nstages;
    const int col = 32 * (int)wt + (lane & 31), f = col / kCbRow, w = col % kCbRow;
    uint32_t dw = 0;
    for (int v = 0; v < 4; v++) {
        const long k = kCbStage * st + 64 * (lane >> 5) + 16 * c + 4 * q + v;
        if (k < K) dw |= ks_balanced_byte((uint32_t)key[((size_t)f * K + k) * kCbRow + w], plane) << (8 * v);
    }
    planes[x] = dw;
}

struct CbmArgs {
    const ks_i32x4 *planes;   // [128][nstages][4][4][64]
    const int8_t *dig;        // [inputs][kpad]
    const int32_t *in;        // [inputs][D + 1]: b is read
    int32_t *out;
    long inputs;
    int D, l, kpad;
    int nstages;              // kpad / 128
    int gtiles;               // 256-input tiles
    int nsplit;               // > 1: the stages are cut in nsplit ranges whose partial sums meet in the zeroed output with atomics
};

// One workgroup: 256 inputs (4 waves x 2 tiles of 32) x one 32-word tile (4 planes) x one range of stages.  The planes of a stage (16 KiB) are staged
// in LDS (double buffered through registers) and read by all four waves; a wave's A fragments are its inputs' digit bytes as they lie in memory,
// and it keeps 2 x 4 accumulators of 32 x 32 int32.
__global__ __launch_bounds__(256) void cb_pks_mfma_kernel(CbmArgs a) {
    constexpr int S = 4;                  // chunks of 32 pairs per stage
    constexpr int NLD = S * 4 * 64 / 256; // 16-byte pieces per thread and stage
    __shared__ ks_i32x4 sB[2][S * 4 * 64];
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int r = lane & 31, h = lane >> 5;
    const long L = blockIdx.x;
    const int gt = (int)(L % a.gtiles), wt = (int)(L / a.gtiles % (kCbCols / 32)), sp = (int)(L / a.gtiles / (kCbCols / 32));
    const int per = (a.nstages + a.nsplit - 1) / a.nsplit, st0 = sp * per, st1 = min(a.nstages, st0 + per);
    if (st0 >= st1) return;   // the whole workgroup: an empty last range
    const ks_i32x4 *src = a.planes + ((size_t)wt * a.nstages + st0) * (S * 4 * 64);
    // the lane's A rows: inputs g0 + 32 m + r (rows past the batch read the last input's digits and store nothing)
    const long g0 = (long)gt * 256 + wave * 64;
    const ks_i32x4 *arow[2];
#pragma unroll
    for (int m = 0; m < 2; m++) {
        const long g = g0 + 32 * m + r;
        arow[m] = reinterpret_cast<const ks_i32x4 *>(a.dig + (size_t)(g < a.inputs ? g : a.inputs - 1) * a.kpad + (size_t)st0 * kCbStage + 64 * h);
    }
    ks_i32x4 pre[NLD], an[2][S], aw[2][S];
    auto load = [&](int s) {   // s: stage within the range
        const ks_i32x4 *p_ = src + (size_t)s * (S * 4 * 64) + tid;
#pragma unroll
        for (int k = 0; k < NLD; k++) pre[k] = p_[256 * k];
#pragma unroll
        for (int m = 0; m < 2; m++)
#pragma unroll
            for (int c = 0; c < S; c++) an[m][c] = arow[m][(size_t)s * (kCbStage / 16) + c];
    };
    auto store = [&](int buf) {
#pragma unroll
        for (int k = 0; k < NLD; k++) sB[buf][tid + 256 * k] = pre[k];
#pragma unroll
        for (int m = 0; m < 2; m++)
#pragma unroll
            for (int c = 0; c < S; c++) aw[m][c] = an[m][c];
    };
    load(0);
    store(0);
    __syncthreads();
    ks_i32x16 acc[2][4];
#pragma unroll
    for (int m = 0; m < 2; m++)
#pragma unroll
        for (int p = 0; p < 4; p++) acc[m][p] = ks_i32x16{0};
    const int NS = st1 - st0;
    for (int s = 0; s < NS; s++) {
        if (s + 1 < NS) load(s + 1);
        const ks_i32x4 *b = sB[s & 1] + lane;
        ks_i32x4 bf[2][4];   // the B fragments of chunk c + 1 are read while chunk c's MFMAs run
#pragma unroll
        for (int p = 0; p < 4; p++) bf[0][p] = b[p * 64];
#pragma unroll
        for (int c = 0; c < S; c++) {
            if (c + 1 < S)
#pragma unroll
                for (int p = 0; p < 4; p++) bf[(c + 1) & 1][p] = b[((c + 1) * 4 + p) * 64];
#pragma unroll
            for (int m = 0; m < 2; m++)
#pragma unroll
                for (int p = 0; p < 4; p++) acc[m][p] = __builtin_amdgcn_mfma_i32_32x32x32_i8(aw[m][c], bf[c & 1][p], acc[m][p], 0, 0, 0);
        }
        if (s + 1 < NS) store((s + 1) & 1);
        __syncthreads();
    }
    // C/D: lane r + 32 h, register e holds row (e & 3) + 8 (e >> 2) + 4 h, column r
    const int col = 32 * wt + r, f = col / kCbRow, w = col % kCbRow;
    const bool add_b = sp == 0 && cb_b_word(f, w);
#pragma unroll
    for (int m = 0; m < 2; m++)
#pragma unroll
        for (int e = 0; e < 16; e++) {
            const long g = g0 + 32 * m + (e & 3) + 8 * (e >> 2) + 4 * h;
            if (g >= a.inputs) continue;
            uint32_t v = 0u - ((uint32_t)acc[m][0][e] + ((uint32_t)acc[m][1][e] << 8) + ((uint32_t)acc[m][2][e] << 16) + ((uint32_t)acc[m][3][e] << 24));
            if (add_b) v += (uint32_t)a.in[(size_t)g * (a.D + 1) + a.D];
            unsigned int *o = reinterpret_cast<unsigned int *>(a.out) + cb_out_row(g, f, a.l) + w;
            if (a.nsplit == 1) *o = v;
            else atomicAdd(o, v);
        }
}

// ------------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------------

// The private key-switching key of a context: the rows as uploaded (the plain kernel), their byte planes (the MFMA kernel) and the digit matrix
// of the batch in flight (grow-only).  D = 0: no key.
struct CbKey {
    DevBuf rows, planes, dig;
    int D = 0, t = 0, basebit = 0, nstages = 0;
    long batch_min = kCbBatchMinInputs;   // inputs from which the MFMA kernel runs

    size_t row_bytes(int D_, int t_) const { return (size_t)2 * D_ * t_ * kCbRow * sizeof(int32_t); }
    static int stages(int D_, int t_) { return (D_ * t_ + kCbStage - 1) / kCbStage; }
    size_t plane_bytes(int D_, int t_) const { return (size_t)(kCbCols / 32) * stages(D_, t_) * 4 * 4 * 64 * 16; }

    // upload `pks` and build the planes; the sizes are checked against the free device memory first.  Replaces any earlier key; on failure no
    // key is set.  Returns when the key is on the device.
    int upload(const int32_t *pks, int D_, int t_, int basebit_, hipStream_t s) {
        D = 0;
        rows = DevBuf();
        planes = DevBuf();
        size_t free_b = 0, total_b = 0;
        THFHE_HIP(hipMemGetInfo(&free_b, &total_b));
        if (row_bytes(D_, t_) + plane_bytes(D_, t_) > free_b)
            return thfhe_fail(THFHE_E_NOMEM, "circuit-bootstrap key: 2 x 2 D t 8 KiB (rows and byte planes) exceed the free device memory");
        THFHE_TRY(rows.grow(row_bytes(D_, t_)));
        THFHE_TRY(planes.grow(plane_bytes(D_, t_)));
        THFHE_HIP(hipMemcpyAsync(rows.as<int32_t>(), pks, row_bytes(D_, t_), hipMemcpyHostToDevice, s));
        const long ns = stages(D_, t_), total = (long)(plane_bytes(D_, t_) / sizeof(uint32_t));
        hipLaunchKernelGGL(cb_planes_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, rows.as<int32_t>(), D_ * t_, ns, total, planes.as<uint32_t>());
        THFHE_HIP(hipGetLastError());
        THFHE_HIP(hipStreamSynchronize(s));   // before the caller's host key may go
        D = D_, t = t_, basebit = basebit_, nstages = (int)ns;
        return THFHE_OK;
    }
};

constexpr long kCbMaxLaunchInputs = 4096;   // inputs per launch: bounds the digit matrix (4096 x 20 KiB at D = 2048, t = 10)

// The private key switch of `inputs` = samples * l records d_in[inputs][D + 1] into d_out[samples][2l][2048], enqueued on `stream`.
// kernel: 0 = by batch size (key.batch_min), 1 = plain, 2 = MFMA.
inline int cb_enqueue(CbKey &key, const int32_t *d_in, long inputs, int l, int32_t *d_out, hipStream_t stream, int kernel = 0) {
    const int K = key.D * key.t;
    const bool mfma = kernel == 2 || (kernel == 0 && inputs >= key.batch_min);
    const long slice = kCbMaxLaunchInputs / l * l;   // whole samples
    if (mfma) THFHE_TRY(key.dig.grow((size_t)std::min(inputs, slice) * key.nstages * kCbStage));
    for (long g0 = 0; g0 < inputs; g0 += slice) {
        const long G = std::min(slice, inputs - g0);
        const int32_t *in = d_in + (size_t)g0 * (key.D + 1);
        int32_t *out = d_out + (size_t)(g0 / l) * 2 * l * kCbRow;
        const size_t out_bytes = (size_t)G * kCbCols * sizeof(int32_t);
        if (mfma) {
            const int kpad = key.nstages * kCbStage;
            hipLaunchKernelGGL(cb_digits_kernel, dim3((unsigned)((kpad + 255) / 256), (unsigned)G), dim3(256), 0, stream, in, key.D, key.t, key.basebit, kpad,
                               key.dig.as<int8_t>());
            CbmArgs k{key.planes.as<ks_i32x4>(), key.dig.as<int8_t>(), in, out, G, key.D, l, kpad, key.nstages, (int)((G + 255) / 256), 1};
            // the stages are cut into ranges until the grid has at least 1 024 workgroups (256 inputs: 1 x 128 x 8)
            while (k.nsplit < 16 && 2 * k.nsplit <= k.nstages && (long)k.gtiles * (kCbCols / 32) * k.nsplit < 1024) k.nsplit *= 2;
            if (k.nsplit > 1) THFHE_HIP(hipMemsetAsync(out, 0, out_bytes, stream));
            hipLaunchKernelGGL(cb_pks_mfma_kernel, dim3((unsigned)((long)k.gtiles * (kCbCols / 32) * k.nsplit)), dim3(256), 0, stream, k);
        } else {
            // ranges of (i, p): enough workgroups to fill the device at small batches, at most kCbPlainSpan pairs each
            int nsplit = (int)std::min<long>(64, (1024 + G - 1) / G);
            nsplit = std::max(nsplit, (K + kCbPlainSpan - 1) / kCbPlainSpan);
            nsplit = std::min(nsplit, K);
            const int kspan = (K + nsplit - 1) / nsplit;
            nsplit = (K + kspan - 1) / kspan;   // no empty range
            if (nsplit > 1) THFHE_HIP(hipMemsetAsync(out, 0, out_bytes, stream));
            const CbArgs a{key.rows.as<int32_t>(), in, out, G, key.D, key.t, key.basebit, l};
            hipLaunchKernelGGL(cb_pks_plain_kernel, dim3((unsigned)G, (unsigned)nsplit), dim3(256), 0, stream, a, kspan, nsplit);
        }
        THFHE_HIP(hipGetLastError());
    }
    return THFHE_OK;
}

}  // namespace

#endif  // THFHE_CB_H
