// thfhe_linear.h -- the dense layer in front of a programmable bootstrap, shared by the single-key and the 3-gen multi-key
// engines: an integer matrix times a vector of LWE records, word-wise mod 2^32.  One kernel for both record widths (n + 1, P n + 1 words), the
// device buffers a context keeps for it, and the host checks of the entries.
#ifndef THFHE_LINEAR_H
#define THFHE_LINEAR_H

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/thfhe_hip.h"
#include "thfhe_common.h"
#include "thfhe_devctx.h"
#include "thfhe_linear_plan.h"

namespace {
using namespace thfhe;

constexpr int kLinTileM = 16;   // outputs a workgroup accumulates per lane
constexpr int kLinTileK = 16;   // weights of one output staged in the LDS at a time: kLinTileM x kLinTileK = one weight per thread
constexpr int kLinMaxDim = 65536;
static_assert(kLinTileM * kLinTileK == 256, "the weight tile is loaded one word per thread");

// Where the K operand records of a sample live.  LinFlatSrc: the contiguous [S][K][rec] array of a flat call, operand k of sample s = record
// s K + k.  LinWireSrc (DENSE launch groups of the gate DAG, thfhe_dag.h): sample j of the slice is node g of instance q (first + j = q cnt + g);
// its operand k is the record of wire pool[t_off[g] + k] in instance q's [n_wires][rec] table, read in place.
struct LinFlatSrc {
    static constexpr bool kWire = false;
    const int32_t *in;
    __device__ const int32_t *sample(long s, int K, int rec) const { return in + (size_t)s * K * rec; }
    __device__ const int32_t *ids(long) const { return nullptr; }
};
struct LinWireSrc {
    static constexpr bool kWire = true;
    const int32_t *wires, *pool, *t_off;
    long first, cnt;
    size_t n_wires;
    __device__ const int32_t *sample(long s, int, int rec) const { return wires + (size_t)((first + s) / cnt) * n_wires * rec; }
    __device__ const int32_t *ids(long s) const { return pool + t_off[(first + s) % cnt]; }
};

// x[s][m][i] = sum_k W[m][k] in[s][k][i] (+ bias[m] on the body word i = rec - 1) mod 2^32, for the S samples of a slice.
// in: the K records per sample of `src`, W: [M][K], bias: [M] or null, x: [S][M][rec].  A workgroup owns kLinTileM outputs x 256 consecutive words
// of one sample: each lane keeps kLinTileM accumulators and reads its word of every input record once (rows of 1 KiB, coalesced); the weights of the
// tile go through the LDS kLinTileK columns at a time and are read back wave-uniformly.  A wire source stages the kLinTileK wire ids of the k-tile
// next to the weights, between the same two barriers, so the record reads of a tile take their row from the LDS and none waits on an index load
// from memory.  grid.x: the 256-word blocks of a record; grid.y strides over the S x ceil(M / kLinTileM) tiles (lwe_linear_launch caps it at
// 65 535).  Lanes past the record's end stay for the barriers and touch no memory.
template <typename Src>
__global__ __launch_bounds__(256) void lwe_linear_kernel(Src src, const int32_t *__restrict__ W, const int32_t *__restrict__ bias,
                                                         int32_t *__restrict__ x, long S, int M, int K, int rec) {
    __shared__ uint32_t w[kLinTileK][kLinTileM];
    int32_t *wid = nullptr;
    if constexpr (Src::kWire) {
        __shared__ int32_t wire_ids[kLinTileK];
        wid = wire_ids;
    }
    const int i = blockIdx.x * 256 + threadIdx.x;
    const bool live = i < rec;
    const int wk = threadIdx.x % kLinTileK, wm = threadIdx.x / kLinTileK;   // the weight this thread stages: consecutive threads, consecutive k
    const int m_tiles = (M + kLinTileM - 1) / kLinTileM;
    const long tiles = S * m_tiles;
    for (long t = blockIdx.y; t < tiles; t += gridDim.y) {
        const long s = t / m_tiles;
        const int m0 = (int)(t - s * m_tiles) * kLinTileM;
        const int32_t *col = src.sample(s, K, rec) + i;
        const int32_t *ids = src.ids(s);
        uint32_t acc[kLinTileM];
#pragma unroll
        for (int m = 0; m < kLinTileM; m++) acc[m] = 0;
        for (int k0 = 0; k0 < K; k0 += kLinTileK) {
            __syncthreads();   // the previous tile's weights have been read
            w[wk][wm] = (m0 + wm < M && k0 + wk < K) ? (uint32_t)W[(size_t)(m0 + wm) * K + k0 + wk] : 0u;
            if constexpr (Src::kWire)
                if (wm == 0) wid[wk] = k0 + wk < K ? ids[k0 + wk] : 0;
            __syncthreads();
            const int kn = K - k0 < kLinTileK ? K - k0 : kLinTileK;
            if (live) {
#pragma unroll 4
                for (int k = 0; k < kn; k++) {
                    uint32_t v;
                    if constexpr (Src::kWire) v = (uint32_t)col[(size_t)wid[k] * rec];
                    else v = (uint32_t)col[(size_t)(k0 + k) * rec];
#pragma unroll
                    for (int m = 0; m < kLinTileM; m++) acc[m] += w[k][m] * v;
                }
            }
        }
        if (live) {
#pragma unroll
            for (int m = 0; m < kLinTileM; m++) {
                if (m0 + m < M) {
                    uint32_t r = acc[m];
                    if (bias && i == rec - 1) r += (uint32_t)bias[m0 + m];
                    x[((size_t)s * M + m0 + m) * rec + i] = (int32_t)r;
                }
            }
        }
    }
}

template <typename Src>
void lwe_linear_launch(const Src &src, const int32_t *W, const int32_t *bias, int32_t *x, size_t S, int M, int K, int rec, hipStream_t stream) {
    const size_t tiles = S * (size_t)((M + kLinTileM - 1) / kLinTileM);
    const dim3 grid((unsigned)((rec + 255) / 256), (unsigned)(tiles < 65535 ? tiles : 65535));
    hipLaunchKernelGGL(lwe_linear_kernel<Src>, grid, dim3(256), 0, stream, src, W, bias, x, (long)S, M, K, rec);
}

// idx[j] = lut[j mod M] for the jobs of one slice of a DENSE launch group: the table of every output, in the job order of the PBS stage
__global__ __launch_bounds__(256) void dense_lut_idx_kernel(const int32_t *__restrict__ lut, int32_t *__restrict__ idx, long jobs, int M) {
    for (long j = (long)blockIdx.x * 256 + threadIdx.x; j < jobs; j += (long)gridDim.x * 256) idx[j] = lut[j % M];
}

// What a context keeps for the dense layer (grow-only): the weights and the bias, a slice's input records and its sums x, and the most PBS jobs
// (samples x outputs) of one slice (thfhe_set_linear_slice).
struct LinBufs {
    DevBuf w, bias, in, x;
    DevBuf dag_words, dag_wires;   // a gate-DAG run's dense families (thfhe_dag_run_dense_batch): the word pool and the operand wire ids
    size_t slice = 4096;
    // profiling (thfhe_linear_last_timings): events around the last slice's input upload and kernel, made by the first profiled call
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    bool ev_valid = false, ev_whole = false;   // ev_whole: the call went on to a timed key switch (the context's ev[3])
    LinBufs() = default;
    LinBufs(const LinBufs &) = delete;
    LinBufs &operator=(const LinBufs &) = delete;
    ~LinBufs() {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
    int events() {
        for (hipEvent_t &e : ev)
            if (!e) THFHE_HIP(hipEventCreate(&e));
        return THFHE_OK;
    }
};

// Host checks of a dense-layer call, before a context or a device is touched.  fused: the call bootstraps x (tv, theta, n_luts, lut_index are its
// arguments); lut_index holds one entry per OUTPUT.
inline int linear_validate(const int32_t *W, int M, int K, const int32_t *in, const int32_t *out, size_t count, bool fused, const void *tv, int theta,
                           int n_luts, const int32_t *lut_index) {
    if (!W || !in || !out || (fused && !tv)) return thfhe_fail(THFHE_E_INVALID, "null argument");
    if (M < 1 || M > kLinMaxDim || K < 1 || K > kLinMaxDim) return thfhe_fail(THFHE_E_INVALID, "linear: M and K must be 1 .. 65536");
    if (fused) {
        if (theta != 1 && theta != 2 && theta != 4) return thfhe_fail(THFHE_E_INVALID, "lut spec: theta must be 1, 2 or 4");
        if (n_luts < 1 || n_luts > 1024) return thfhe_fail(THFHE_E_INVALID, "n_luts must be 1 .. 1024");
        if (lut_index)
            for (int m = 0; m < M; m++)
                if (lut_index[m] < 0 || lut_index[m] >= n_luts) return thfhe_fail(THFHE_E_INVALID, "lut_index out of range (0 .. n_luts-1)");
    }
    if (count > (size_t)INT32_MAX / 16 / (size_t)M) return thfhe_fail(THFHE_E_INVALID, "count too large");
    return THFHE_OK;
}

template <typename Ctx>
int ctx_set_linear_slice(Ctx *c, size_t jobs) {
    if (!c || jobs < 1 || jobs > ((size_t)1 << 20)) return thfhe_fail(THFHE_E_INVALID, "slice must be 1 .. 2^20 jobs");
    std::lock_guard<std::mutex> g(c->mu);
    c->lin.slice = jobs;
    return THFHE_OK;
}

// ms = {input upload, lwe_linear_kernel, upload start .. end of the key switch} of the last slice of the last profiled dense-layer call; a call
// without a key switch ends ms[2] at the kernel's end
template <typename Ctx>
int ctx_linear_last_timings(Ctx *c, float ms[3]) {
    if (!c || !ms) return thfhe_fail(THFHE_E_INVALID, "null argument");
    std::lock_guard<std::mutex> g(c->mu);
    if (!c->lin.ev_valid) return thfhe_fail(THFHE_E_INVALID, "no profiled call recorded");
    hipEvent_t end = c->lin.ev_whole && c->ev_valid ? c->ev[3] : c->lin.ev[2];
    THFHE_HIP(hipEventSynchronize(end));
    THFHE_HIP(hipEventElapsedTime(&ms[0], c->lin.ev[0], c->lin.ev[1]));
    THFHE_HIP(hipEventElapsedTime(&ms[1], c->lin.ev[1], c->lin.ev[2]));
    THFHE_HIP(hipEventElapsedTime(&ms[2], c->lin.ev[0], end));
    return THFHE_OK;
}

inline int linear_tile(int *tile_m, int *tile_k) {
    if (!tile_m || !tile_k) return thfhe_fail(THFHE_E_INVALID, "null argument");
    *tile_m = kLinTileM, *tile_k = kLinTileK;
    return THFHE_OK;
}

}  // namespace

#endif  // THFHE_LINEAR_H
