// thfhe_mk_pack.h -- the multi-key packing key switch of the 3-gen engine: LWE-shaped Torus32 records -> Torus64 RLWE samples under
// the summed ring key Z = sum_q z_q, and the box packing of p of them into one encrypted test vector.  Included by thfhe_mk.hip.
//
// The pure digit and index arithmetic (mkp_*) is host-callable: tests/emu/mk_pack_emu.cpp replays it against the numpy model without a GPU.
//   mk_pack_rows_kernel       T_i = (0, b_i 2^32 on X^0) - sum_{j, p: d != 0} PK[j][p][d - 1] mod 2^64, both polynomials: the hot path, a stream of
//                             64-bit integer adds over key rows of 2N words
//   mk_pack_rows_wide_kernel  the same sums for large batches: 32 records per workgroup, a key row tile fetched once per digit value
//   mk_pack_boxes_kernel<NN>  output g = U(X) sum_{i < p} X^(i N/p) T_(g p + i): the Torus64 twin of pack_boxes_kernel (thfhe_threshold.hip)
#ifndef THFHE_MK_PACK_H
#define THFHE_MK_PACK_H

#include <stddef.h>
#include <stdint.h>

#include "thfhe_lane.h"

namespace thfhe {

// ---- what the host emulation shares with the kernels -----------------------------------------------------------------------------------------
// A mask word with the LWE key switch's rounding offset (ks_prec_offset, thfhe_keyswitch.h): half a unit of the last digit, nothing when the t
// digits of basebit bits cover the whole word.  The sum wraps mod 2^32: 0xFFFFFFFF rounds up to the all-zero digits.
THFHE_FN uint32_t mkp_round_word(int32_t a, int t, int basebit) {
    const int bt = t * basebit;
    return (uint32_t)a + (bt >= 32 ? 0u : 1u << (31 - bt));
}
// digit p (0 = most significant) of a rounded word: 0 .. 2^basebit - 1; digit d != 0 names key row d - 1
THFHE_FN int mkp_digit(uint32_t abar, int p, int basebit) { return (int)((abar >> (32 - (p + 1) * basebit)) & ((1u << basebit) - 1u)); }
// coefficient c of X^(i B) f mod X^N + 1 is f[c - i B] for c >= i B and -f[c - i B + N] below: the source index, *neg = the sign
THFHE_FN int mkp_box_src(int c, int i, int B, int N, bool *neg) {
    const int e = c - i * B;   // in (-N, N)
    *neg = e < 0;
    return e & (N - 1);
}
// Prefix sum up to j, -N <= j < 2N, of the negacyclic extension E of S (E[j + N] = -E[j]) from the inclusive prefix sums pre[] of S[0 .. N) and
// tot = pre[N - 1]: pre[j] inside [0, N), tot - pre[j mod N] one period below or above (j = -1 gives 0).
THFHE_FN uint64_t mkp_ext_prefix(const uint64_t *pre, uint64_t tot, int j, int N) { return (j >= 0 && j < N) ? pre[j] : tot - pre[j & (N - 1)]; }
// (U S)[c], U = X^(-B/2) (1 + X + ... + X^(B-1)): the sum of E[j] over c - B/2 < j <= c + B/2, a difference of two prefixes
THFHE_FN uint64_t mkp_window(const uint64_t *pre, uint64_t tot, int c, int B, int N) {
    return mkp_ext_prefix(pre, tot, c + B / 2, N) - mkp_ext_prefix(pre, tot, c - B / 2, N);
}

// whether digit p of a rounded word has the value v (1 .. 2^basebit - 1): one record's bit of the membership mask mk_pack_rows_wide_kernel builds
// for (j, p, v) over its record group -- bit g of the mask is mkp_digit_is of record g's word j
THFHE_FN bool mkp_digit_is(uint32_t abar, int p, int basebit, int v) { return mkp_digit(abar, p, basebit) == v; }

constexpr int kMkPackGroup = 4;     // records per workgroup of mk_pack_rows_kernel: their partial sums live in registers
constexpr int kMkPackTile = 512;    // int64 words of the 2N-word row a workgroup owns: 256 lanes x 16 B
constexpr int kMkPackWideGroup = 32;   // records per workgroup of mk_pack_rows_wide_kernel: one bit each of a 32-bit membership mask
constexpr int kMkPackWideTile = 256;   // int64 words of the row a wide workgroup owns: 256 lanes x 8 B, so that 32 sums fit the register file
// records from which mk_pack_enqueue takes the wide kernel (thfhe_mk_set_pack_wide_threshold): the smallest size at which its median lay below the
// direct kernel's minimum on every measured key (tools/mk_pack_bench.py, profiles/mk_pack_wide_bench.json)
constexpr size_t kMkPackWideDefault = 4096;

}  // namespace thfhe

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

namespace {
using namespace thfhe;

struct MkPackArgs {
    const int32_t *recs;   // [count][D + 1]
    const int64_t *pk;     // [D][t][R][2][N]
    int64_t *T;            // [count][2][N]
    long count;
    int D, t, basebit, N;
};

// grid = (ceil(count / kMkPackGroup), 2N / kMkPackTile): workgroup (x, y) owns words [512 y, 512 y + 512) of the 2N-word sums of records
// [4 x, 4 x + 4) and walks all D t digits with the four partial sums in registers -- no two workgroups add into the same output word, no atomics.
// The mask words travel through LDS 256 at a time with the rounding offset applied; a digit is made wave-uniform (readfirstlane), so a zero digit
// is a scalar branch around the 16-byte-per-lane load of its key row.  Integer adds mod 2^64: the order of the rows does not matter.
__global__ __launch_bounds__(256) void mk_pack_rows_kernel(MkPackArgs a) {
    constexpr int G = kMkPackGroup;
    __shared__ uint32_t sA[G][256];
    const int tid = threadIdx.x;
    const long g0 = (long)blockIdx.x * G;   // < count: the grid covers the records exactly
    const int ng = (int)(a.count - g0 < G ? a.count - g0 : G);
    const int col = (int)blockIdx.y * kMkPackTile + 2 * tid;   // < 2N: the grid covers the row exactly
    const size_t row = 2 * (size_t)a.N, rec = (size_t)a.D + 1;
    const int R = (1 << a.basebit) - 1;
    unsigned long long s0[G], s1[G];
#pragma unroll
    for (int g = 0; g < G; g++) s0[g] = s1[g] = 0;
    for (int j0 = 0; j0 < a.D; j0 += 256) {
        const int jn = a.D - j0 < 256 ? a.D - j0 : 256;
        __syncthreads();   // the words of the chunk before are consumed
#pragma unroll
        for (int g = 0; g < G; g++) sA[g][tid] = mkp_round_word(g < ng && tid < jn ? a.recs[(size_t)(g0 + g) * rec + j0 + tid] : 0, a.t, a.basebit);
        __syncthreads();
        for (int jj = 0; jj < jn; jj++) {
            const int64_t *rows = a.pk + (size_t)(j0 + jj) * a.t * R * row + col;
#pragma unroll
            for (int g = 0; g < G; g++) {
                const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane((int)sA[g][jj]);
                for (int p = 0; p < a.t; p++) {
                    const int d = mkp_digit(w, p, a.basebit);
                    if (d == 0) continue;
                    const ulonglong2 v = *reinterpret_cast<const ulonglong2 *>(rows + ((size_t)p * R + (d - 1)) * row);
                    s0[g] -= v.x;
                    s1[g] -= v.y;
                }
            }
        }
    }
#pragma unroll
    for (int g = 0; g < G; g++) {
        if (g >= ng) break;
        if (col == a.N) s0[g] += (unsigned long long)(int64_t)a.recs[(size_t)(g0 + g) * rec + a.D] << 32;   // (0, b 2^32 on X^0)
        *reinterpret_cast<ulonglong2 *>(a.T + (size_t)(g0 + g) * row + col) = ulonglong2{s0[g], s1[g]};
    }
}

// The same sums with the key row fetched once per workgroup: grid = (ceil(count / 32), 2N / 256), workgroup (x, y) owns words
// [256 y, 256 y + 256) of the sums of records [32 x, 32 x + 32), one 8-byte word per lane and 32 partial sums in registers.  It walks (j, p, v), v the
// digit VALUE 1 .. R: lane L holds the rounded word j of record L mod 32 (LDS, [j][record] with a padded row: conflict-free both ways), a ballot
// of mkp_digit_is over the wave is the wave-uniform membership mask of v, and row tile (j, p, v - 1) is loaded once when the mask is not empty and
// subtracted from exactly the sums whose bit is set (a scalar all-ones / zero word ANDed into the tile: no divergence).  Records past the batch's end
// enter as zero words, whose digits are all zero.  No atomics, no two workgroups write one word; the sums are the direct kernel's word for word.
__global__ __launch_bounds__(256) void mk_pack_rows_wide_kernel(MkPackArgs a) {
    constexpr int G = kMkPackWideGroup;
    __shared__ uint32_t sA[256][G + 1];
    const int tid = threadIdx.x, lg = tid & (G - 1);
    const long g0 = (long)blockIdx.x * G;   // < count: the grid covers the records exactly
    const int ng = (int)(a.count - g0 < G ? a.count - g0 : G);
    const int col = (int)blockIdx.y * kMkPackWideTile + tid;   // < 2N: the grid covers the row exactly
    const size_t row = 2 * (size_t)a.N, rec = (size_t)a.D + 1;
    const int R = (1 << a.basebit) - 1;
    unsigned long long s[G];
#pragma unroll
    for (int g = 0; g < G; g++) s[g] = 0;
    for (int j0 = 0; j0 < a.D; j0 += 256) {
        const int jn = a.D - j0 < 256 ? a.D - j0 : 256;
        __syncthreads();   // the words of the chunk before are consumed
#pragma unroll 4
        for (int g = 0; g < G; g++) sA[tid][g] = mkp_round_word(g < ng && tid < jn ? a.recs[(size_t)(g0 + g) * rec + j0 + tid] : 0, a.t, a.basebit);
        __syncthreads();
        for (int jj = 0; jj < jn; jj++) {
            const int64_t *rows = a.pk + (size_t)(j0 + jj) * a.t * R * row + col;
            const uint32_t w = sA[jj][lg];
            for (int p = 0; p < a.t; p++) {
                for (int v = 1; v <= R; v++) {
                    const uint32_t m = (uint32_t)__ballot(mkp_digit_is(w, p, a.basebit, v));   // lanes 32 .. 63 repeat lanes 0 .. 31
                    if (m == 0) continue;
                    const unsigned long long x = *reinterpret_cast<const unsigned long long *>(rows + ((size_t)p * R + (v - 1)) * row);
#pragma unroll
                    for (int g = 0; g < G; g++) {
                        const uint32_t sel = 0u - ((m >> g) & 1u);
                        s[g] -= x & (((unsigned long long)sel << 32) | sel);
                    }
                }
            }
        }
    }
#pragma unroll
    for (int g = 0; g < G; g++) {
        if (g < ng) {
            unsigned long long v = s[g];
            if (col == a.N) v += (unsigned long long)(int64_t)a.recs[(size_t)(g0 + g) * rec + a.D] << 32;   // (0, b 2^32 on X^0)
            a.T[(size_t)(g0 + g) * row + col] = (int64_t)v;
        }
    }
}

// Box packing over Torus64: output g = U(X) * sum_{i < p} X^(i B) T_(g p + i) mod X^NN + 1, B = NN / p, U = X^(-B/2) (1 + X + ... + X^(B-1)).
// grid = (outputs, 2): block (g, poly) owns one polynomial of the 2 NN-word sums T; thread tid owns coefficients tid + 1024 m.
//   strided rotate-sum   S[c] = sum_i (X^(i B) T_i)[c] (mkp_box_src): every word of the p records is read once
//   window sum           (U S)[c] as a difference of two prefixes of the negacyclic extension of S (mkp_window), from the inclusive prefix sums of
//                        S: a Hillis-Steele scan in place in NN x 8 B of LDS (8 / 16 / 32 KiB), a barrier between its reads and its writes
// Integer sums mod 2^64, no atomics; 64-bit offsets into T.
template <int NN>
__global__ __launch_bounds__(1024) void mk_pack_boxes_kernel(const int64_t *__restrict__ T, int p, int64_t *__restrict__ out_a, int64_t *__restrict__ out_b) {
    constexpr int M = NN / 1024;
    __shared__ uint64_t sPre[NN];
    const size_t g = blockIdx.x;
    const int poly = blockIdx.y, tid = threadIdx.x;
    const int B = NN / p;
    const uint64_t *src = reinterpret_cast<const uint64_t *>(T) + g * p * 2 * NN + (size_t)poly * NN;
#pragma unroll
    for (int m = 0; m < M; m++) {
        const int c = tid + 1024 * m;
        uint64_t acc = 0;
#pragma unroll 4
        for (int i = 0; i < p; i++) {
            bool neg;
            const int e = mkp_box_src(c, i, B, NN, &neg);
            const uint64_t v = src[(size_t)i * 2 * NN + e];
            acc += neg ? 0ull - v : v;
        }
        sPre[c] = acc;
    }
    __syncthreads();
    for (int d = 1; d < NN; d <<= 1) {
        uint64_t v[M];
#pragma unroll
        for (int m = 0; m < M; m++) {
            const int c = tid + 1024 * m;
            v[m] = sPre[c] + (c >= d ? sPre[c - d] : 0ull);
        }
        __syncthreads();
#pragma unroll
        for (int m = 0; m < M; m++) sPre[tid + 1024 * m] = v[m];
        __syncthreads();
    }
    const uint64_t tot = sPre[NN - 1];
    int64_t *out = (poly ? out_b : out_a) + g * NN;
#pragma unroll
    for (int m = 0; m < M; m++) {
        const int c = tid + 1024 * m;
        out[c] = (int64_t)mkp_window(sPre, tot, c, B, NN);
    }
}

// accumulator start of a rotation on an ENCRYPTED table: acc[job] = (X^{-barb} tv_a[t], X^{-barb} tv_b[t]), t = lut_idx[job] (null: table 0).  The
// index (q + barb) mod 2N and the sign from its bit N of mk_lut_acc_init_kernel, on both polynomials.
__global__ __launch_bounds__(256) void mk_lut_acc_init_enc_kernel(const int32_t *__restrict__ barb, const int64_t *__restrict__ tv_a,
                                                                   const int64_t *__restrict__ tv_b, const int32_t *__restrict__ lut_idx, long jobs, int N,
                                                                   int64_t *__restrict__ acc) {
    const long job = blockIdx.x;
    if (job >= jobs) return;
    const int b = barb[job];
    const size_t t = lut_idx ? (size_t)lut_idx[job] * N : 0;
    int64_t *ap = acc + job * 2 * N;
    for (int q = threadIdx.x; q < N; q += 256) {
        const int e = (q + b) & (2 * N - 1);
        const int64_t va = tv_a[t + (e & (N - 1))], vb = tv_b[t + (e & (N - 1))];
        ap[q] = (e & N) ? (int64_t)(0ull - (uint64_t)va) : va;
        ap[N + q] = (e & N) ? (int64_t)(0ull - (uint64_t)vb) : vb;
    }
}

}  // namespace
#endif  // __HIPCC__

#endif  // THFHE_MK_PACK_H
