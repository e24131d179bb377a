// thfhe_lut_prologue.h -- the front half of every programmable bootstrap, shared by the single-key and the 3-gen multi-key
// engines: one arithmetic, one kernel, and the two places a job's operands can live (contiguous arrays, the gate-DAG wire table).
#ifndef THFHE_LUT_PROLOGUE_H
#define THFHE_LUT_PROLOGUE_H

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/thfhe_hip.h"
#include "thfhe_lane.h"

namespace {
using namespace thfhe;

// One word of a job: x = w0 x0 [+ w1 x1] [+ w2 x2] (+ bias on the body word) mod 2^32, rounded to a multiple of theta in Z_2N:
// bar = modswitch_{2N/theta}(x) * theta (theta = 1: the gates' plain mod-switch).  x1 / x2 are read only if the spec names them.
__device__ inline int32_t lut_prologue_word(const thfhe_lut_spec &sp, const int32_t *x0, const int32_t *x1, const int32_t *x2, bool body, int log2_2n) {
    uint32_t v = (uint32_t)sp.weights[0] * (uint32_t)*x0;
    if (sp.n_inputs > 1) v += (uint32_t)sp.weights[1] * (uint32_t)*x1;
    if (sp.n_inputs > 2) v += (uint32_t)sp.weights[2] * (uint32_t)*x2;
    if (body) v += (uint32_t)sp.bias;
    const int log2_theta = sp.theta >> 1;   // theta is 1, 2 or 4 (lut_spec_check)
    return (int32_t)((uint32_t)modswitch2n((int32_t)v, log2_2n - log2_theta) << log2_theta);
}

// What a source writes to lut_idx[job]: nothing (the caller brings the rotation's index array, or every job uses table 0), an index from the
// source's table column, or the job number (every job rotates a table of its own: the packed tables of a tree's selection level).
enum class LutIdx { none, table, job };

// Flat source: record s of the contiguous arrays in0 .. in2 ([records][n + 1] words) serves the `reps` jobs s reps + r, one spec for all.
// LutIdx::table: job s reps + r looks up row table_index[s] reps + r (table_index null: table 0 for every record).
template <LutIdx Idx>
struct LutFlatSrc {
    static constexpr LutIdx kIdx = Idx;
    const int32_t *in0, *in1, *in2;
    thfhe_lut_spec sp;
    int reps;
    const int32_t *table_index;
    __device__ const thfhe_lut_spec &spec(long) const { return sp; }
    __device__ void operands(long j, int n, const int32_t *x[3]) const {
        const size_t off = (size_t)(j / reps) * ((size_t)n + 1);
        x[0] = in0 + off, x[1] = in1 + off, x[2] = in2 + off;
    }
    __device__ int32_t index(long j) const {
        if (Idx == LutIdx::job) return (int32_t)j;
        const long s = j / reps;
        return (int32_t)((table_index ? table_index[s] : 0) * (long)reps + (j - s * reps));
    }
};

// Where a wire-table job's spec comes from: one for the whole launch, or node g's entry of the run's spec array.
struct LutSpecByValue {
    thfhe_lut_spec sp;
    __device__ const thfhe_lut_spec &of(long) const { return sp; }
};
struct LutSpecPerNode {
    const thfhe_lut_spec *specs;
    const int32_t *t_spec;
    __device__ const thfhe_lut_spec &of(long g) const { return specs[t_spec[g]]; }
};

// Wire-table source (gate-DAG launch groups, thfhe_dag.h): node s = j / reps of the slice is node g of instance q (first + s = q cnt + g); its
// operands are the wires t0[g], t1[g], t2[g] of instance q's [n_wires][n + 1] table, read in place.  LutIdx::table: job s reps + r looks up
// row t_idx[g] + r (a LUT node's table, a TREE node's row0 + r).
template <typename Spec, LutIdx Idx>
struct LutWireSrc {
    static constexpr LutIdx kIdx = Idx;
    const int32_t *wires, *t0, *t1, *t2;
    Spec sp;
    const int32_t *t_idx;
    long first, cnt;
    size_t n_wires;
    int reps;
    __device__ long node(long j) const { return (first + j / reps) % cnt; }
    __device__ const thfhe_lut_spec &spec(long j) const { return sp.of(node(j)); }
    __device__ void operands(long j, int n, const int32_t *x[3]) const {
        const long g = node(j);
        const size_t words = (size_t)n + 1;
        const int32_t *rec = wires + (size_t)((first + j / reps) / cnt) * n_wires * words;
        x[0] = rec + (size_t)t0[g] * words, x[1] = rec + (size_t)t1[g] * words, x[2] = rec + (size_t)t2[g] * words;
    }
    __device__ int32_t index(long j) const { return Idx == LutIdx::job ? (int32_t)j : t_idx[node(j)] + (int32_t)(j % reps); }
};

// bara[j][0 .. n) / barb[j] (and lut_idx[j]) of jobs 0 .. jobs-1 of `src`.  n = mask words of a record (n, or P n on the 3-gen scheme), pad = row
// stride of bara.  One thread per word; grid.y strides over the jobs (lut_prologue_launch caps it at 65 535).
template <typename Src>
__global__ __launch_bounds__(256) void lut_prologue_kernel(Src src, long jobs, int n, int pad, int log2_2n, int32_t *__restrict__ bara,
                                                           int32_t *__restrict__ barb, int32_t *__restrict__ lut_idx) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i > n) return;
    for (long j = blockIdx.y; j < jobs; j += gridDim.y) {
        const thfhe_lut_spec sp = src.spec(j);
        const int32_t *x[3];
        src.operands(j, n, x);
        const int32_t bar = lut_prologue_word(sp, x[0] + i, x[1] + i, x[2] + i, i == n, log2_2n);
        if (i == n) {
            barb[j] = bar;
            if (Src::kIdx != LutIdx::none) lut_idx[j] = src.index(j);
        } else {
            bara[(size_t)j * pad + i] = bar;
        }
    }
}

template <typename Src>
void lut_prologue_launch(const Src &src, size_t jobs, int n, int pad, int log2_2n, int32_t *bara, int32_t *barb, int32_t *lut_idx, hipStream_t stream) {
    const dim3 grid((unsigned)((n + 1 + 255) / 256), (unsigned)(jobs < 65535 ? jobs : 65535));
    hipLaunchKernelGGL(lut_prologue_kernel<Src>, grid, dim3(256), 0, stream, src, (long)jobs, n, pad, log2_2n, bara, barb, lut_idx);
}

}  // namespace

#endif  // THFHE_LUT_PROLOGUE_H
