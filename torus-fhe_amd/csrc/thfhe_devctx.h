// thfhe_devctx.h -- host plumbing shared by the engine contexts of libthfhe_hip.so: grow-only device buffers (DevBuf), the device /
// stream / event core every context derives from (DevCtx), its destroy, and the C ABI bodies the single-key (thfhe_sk.hip) and 3-gen
// multi-key (thfhe_mk.hip) engines have in common.  Host code only: no kernels.
#ifndef THFHE_DEVCTX_H
#define THFHE_DEVCTX_H

#include <hip/hip_runtime.h>

#include <mutex>
#include <vector>

#include "thfhe_common.h"

// Host-side C++ of the library stays out of its dynamic symbol table: only the C ABI of include/thfhe_hip.h is exported.  The engine
// context structs (thfhe_ctx, ...) are marked THFHE_INTERNAL where they are defined.
#define THFHE_INTERNAL __attribute__((visibility("hidden")))
#pragma GCC visibility push(hidden)

namespace thfhe {

// return a non-zero THFHE_* code of `expr` (DevBuf::grow, DevCtx::open) to the caller
#define THFHE_TRY(expr)                       \
    do {                                      \
        const int thfhe_rc_ = (expr);         \
        if (thfhe_rc_) return thfhe_rc_;      \
    } while (0)

// One device allocation that only grows: grow(bytes) keeps an allocation of at least `bytes`, else frees it and allocates exactly
// `bytes` (the contents are not kept).  Freed by the destructor; movable, not copyable.
class DevBuf {
public:
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p_(o.p_), bytes_(o.bytes_) { o.p_ = nullptr, o.bytes_ = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept {
        if (this != &o) {
            if (p_) (void)hipFree(p_);
            p_ = o.p_, bytes_ = o.bytes_;
            o.p_ = nullptr, o.bytes_ = 0;
        }
        return *this;
    }
    ~DevBuf() {
        if (p_) (void)hipFree(p_);
    }
    int grow(size_t bytes) {
        if (bytes <= bytes_) return THFHE_OK;
        if (p_) (void)hipFree(p_);
        p_ = nullptr, bytes_ = 0;
        THFHE_HIP(hipMalloc(&p_, bytes));
        bytes_ = bytes;
        return THFHE_OK;
    }
    size_t bytes() const { return bytes_; }
    template <typename T>
    T *as() const { return static_cast<T *>(p_); }

private:
    void *p_ = nullptr;
    size_t bytes_ = 0;
};

// Staging buffers of the host-buffer calls: three inputs and one output of `words` int32 each.
struct Stage {
    DevBuf in[3], out;
    int grow(size_t words) {
        for (DevBuf &b : in) {
            const int rc = b.grow(words * sizeof(int32_t));
            if (rc) return rc;
        }
        return out.grow(words * sizeof(int32_t));
    }
    int32_t *in_ptr(int q) const { return in[q].as<int32_t>(); }
    int32_t *out_ptr() const { return out.as<int32_t>(); }
};

// What every engine context holds: its device, its stream (created non-blocking by open()), the profiling events, the mutex that
// serialises calls on the context and the twiddle table of its ring degree.  `stream` is where calls enqueue; it differs from
// `own_stream` only after an engine's set_stream.
struct DevCtx {
    int device = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    bool profiling = false, ev_valid = false;
    std::mutex mu;
    DevBuf d_tw;   // make_twiddle_table(N) (thfhe_lane.h), filled by upload_twiddles

    DevCtx() = default;
    DevCtx(const DevCtx &) = delete;
    DevCtx &operator=(const DevCtx &) = delete;
    ~DevCtx() {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
        if (own_stream) (void)hipStreamDestroy(own_stream);
    }
    int open(int dev, bool with_events) {
        int n = 0;
        if (hipGetDeviceCount(&n) != hipSuccess || dev < 0 || dev >= n)
            return thfhe_fail(THFHE_E_NO_DEVICE, "no usable HIP device (this library has no CPU fallback)");
        THFHE_HIP(hipSetDevice(dev));
        device = dev;
        THFHE_HIP(hipStreamCreateWithFlags(&own_stream, hipStreamNonBlocking));
        stream = own_stream;
        if (with_events)
            for (hipEvent_t &e : ev) THFHE_HIP(hipEventCreate(&e));
        return THFHE_OK;
    }
    // build the twiddle table of ring degree N and copy it to d_tw; returns when the copy is done
    int upload_twiddles(int N) {
        const std::vector<cplx> tw = make_twiddle_table(N);
        THFHE_TRY(d_tw.grow(tw.size() * sizeof(cplx)));
        THFHE_HIP(hipMemcpyAsync(d_tw.as<cplx>(), tw.data(), tw.size() * sizeof(cplx), hipMemcpyHostToDevice, stream));
        THFHE_HIP(hipStreamSynchronize(stream));
        return THFHE_OK;
    }
};

inline int set_device(int device) {
    THFHE_HIP(hipSetDevice(device));
    return THFHE_OK;
}
// The prologue of a call that enqueues work: lock the context, then make its device current (rc: THFHE_OK or the hipSetDevice failure).
struct DevLock {
    std::lock_guard<std::mutex> g;
    const int rc;
    explicit DevLock(DevCtx &c) : g(c.mu), rc(set_device(c.device)) {}
};

// Every *_ctx_destroy: a call still running on another thread finishes first, the context's own stream is drained, then the members
// free their device memory and ~DevCtx destroys the events and the stream.
template <typename Ctx>
void ctx_destroy(Ctx *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    {
        std::lock_guard<std::mutex> g(c->mu);
        if (c->own_stream) (void)hipStreamSynchronize(c->own_stream);
    }
    delete c;
}

// ---- C ABI bodies shared by the single-key and multi-key engines (thfhe_* and thfhe_mk_*) ------------------------------------------

inline void *ctx_dev_alloc(DevCtx *c, size_t bytes) {
    if (!c) return nullptr;
    void *p = nullptr;
    if (hipSetDevice(c->device) != hipSuccess || hipMalloc(&p, bytes) != hipSuccess) return nullptr;
    return p;
}
inline void ctx_dev_free(DevCtx *c, void *p) {
    if (c) (void)hipSetDevice(c->device);
    (void)hipFree(p);
}
inline int ctx_copy(DevCtx *c, void *dst, const void *src, size_t bytes, hipMemcpyKind kind) {
    if (!c) return thfhe_fail(THFHE_E_INVALID, "null ctx");
    THFHE_HIP(hipSetDevice(c->device));
    THFHE_HIP(hipMemcpyAsync(dst, src, bytes, kind, c->stream));
    THFHE_HIP(hipStreamSynchronize(c->stream));
    return THFHE_OK;
}
inline int ctx_sync(DevCtx *c) {
    if (!c) return thfhe_fail(THFHE_E_INVALID, "null ctx");
    THFHE_HIP(hipStreamSynchronize(c->stream));
    return THFHE_OK;
}
inline int ctx_set_profiling(DevCtx *c, int enabled) {
    if (!c) return thfhe_fail(THFHE_E_INVALID, "null ctx");
    std::lock_guard<std::mutex> g(c->mu);
    c->profiling = enabled != 0;
    c->ev_valid = false;
    return THFHE_OK;
}
// ms = {prologue, blind rotation, key switch, whole call} of the last profiled call
inline int ctx_last_timings(DevCtx *c, float ms[4]) {
    if (!c || !ms) return thfhe_fail(THFHE_E_INVALID, "null argument");
    std::lock_guard<std::mutex> g(c->mu);
    if (!c->ev_valid) return thfhe_fail(THFHE_E_INVALID, "no profiled call recorded");
    THFHE_HIP(hipEventSynchronize(c->ev[3]));
    THFHE_HIP(hipEventElapsedTime(&ms[0], c->ev[0], c->ev[1]));
    THFHE_HIP(hipEventElapsedTime(&ms[1], c->ev[1], c->ev[2]));
    THFHE_HIP(hipEventElapsedTime(&ms[2], c->ev[2], c->ev[3]));
    THFHE_HIP(hipEventElapsedTime(&ms[3], c->ev[0], c->ev[3]));
    return THFHE_OK;
}
template <typename Ctx>
int ctx_set_dag_slice(Ctx *c, size_t max_gates) {
    if (!c || max_gates < 1 || max_gates > 32767) return thfhe_fail(THFHE_E_INVALID, "slice must be 1 .. 32767 gates");
    std::lock_guard<std::mutex> g(c->mu);
    c->dag_slice = max_gates;
    return THFHE_OK;
}
// The host-buffer form of a call (gates, gates_mixed, bootstrap): lock, device current, staging grown to `words` words, src[q] uploaded
// into stage.in[q] (bytes[q]; null sources skipped), run() enqueued, then `out_bytes` copied from `res` to `out` after all uploads
// (so `out` may alias an input) and the stream drained.
template <typename Ctx, typename Run>
int ctx_staged(Ctx *c, size_t words, const void *const (&src)[3], const size_t (&bytes)[3], Run run, const DevBuf &res, void *out, size_t out_bytes) {
    DevLock lk(*c);
    if (lk.rc) return lk.rc;
    int rc = c->stage.grow(words);
    if (rc) return rc;
    for (int q = 0; q < 3; q++)
        if (src[q]) THFHE_HIP(hipMemcpyAsync(c->stage.in_ptr(q), src[q], bytes[q], hipMemcpyHostToDevice, c->stream));
    rc = run();
    if (rc) return rc;
    THFHE_HIP(hipMemcpyAsync(out, res.as<void>(), out_bytes, hipMemcpyDeviceToHost, c->stream));
    THFHE_HIP(hipStreamSynchronize(c->stream));
    return THFHE_OK;
}
// ... and of a call that goes up and down in slices of at most S_max samples (the multi-value bootstraps and the trees, thfhe_pbs_host.h), the
// caller having locked the context and sized every buffer for S_max: per slice the operand records in[q] (null sources skipped) into stage.in[q] and, with `index`, the slice's
// per-sample indices into d_index; run(s0, S, last) enqueued (s0: the slice's first sample); then the slice's S records of out_words words copied
// from `res` to their place in `out`.  The stream is drained once, after the last slice.
template <typename Ctx, typename Run>
int ctx_sliced(Ctx *c, size_t count, size_t S_max, const int32_t *const (&in)[3], const int32_t *index, int32_t *d_index, Run run, const int32_t *res,
               int32_t *out, size_t out_words) {
    const size_t words = c->rec_words();
    for (size_t s0 = 0; s0 < count; s0 += S_max) {
        const size_t S = count - s0 < S_max ? count - s0 : S_max;
        for (int q = 0; q < 3; q++)
            if (in[q]) THFHE_HIP(hipMemcpyAsync(c->stage.in_ptr(q), in[q] + s0 * words, S * words * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
        if (index) THFHE_HIP(hipMemcpyAsync(d_index, index + s0, S * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
        THFHE_TRY(run(s0, S, s0 + S == count));
        THFHE_HIP(hipMemcpyAsync(out + s0 * out_words, res, S * out_words * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    }
    THFHE_HIP(hipStreamSynchronize(c->stream));
    return THFHE_OK;
}

// thfhe_gates / thfhe_mk_gates: one gate on host buffers; gates(d0, d1, d2, dout, count) is the engine's gates_dev body on the staging arrays
template <typename Ctx, typename Gates>
int ctx_gates(Ctx *c, const int32_t *in0, const int32_t *in1, const int32_t *in2, int32_t *out, size_t count, Gates gates) {
    if (!c || !in0 || !out) return thfhe_fail(THFHE_E_INVALID, "null argument");
    if (count == 0) return THFHE_OK;
    const size_t words = count * c->rec_words(), bytes = words * sizeof(int32_t);
    return ctx_staged(c, words, {in0, in1, in2}, {bytes, bytes, bytes}, [&] {
        return gates(c->stage.in_ptr(0), in1 ? c->stage.in_ptr(1) : nullptr, in2 ? c->stage.in_ptr(2) : nullptr, c->stage.out_ptr(), count);
    }, c->stage.out, out, bytes);
}
// thfhe_gates_mixed / thfhe_mk_gates_mixed after the entry's own checks (the opcodes an engine admits differ): two-input gates with per-gate
// opcodes, which travel in staging buffer 2; run(d0, d1, d_ops, dout) enqueues the engine's bootstraps of the `count` gates
template <typename Ctx, typename Run>
int ctx_gates_mixed(Ctx *c, const int32_t *ops, const int32_t *in0, const int32_t *in1, int32_t *out, size_t count, Run run) {
    const size_t words = count * c->rec_words(), bytes = words * sizeof(int32_t);
    return ctx_staged(c, words, {in0, in1, ops}, {bytes, bytes, count * sizeof(int32_t)}, [&] {
        return run(c->stage.in_ptr(0), c->stage.in_ptr(1), c->stage.in_ptr(2), c->stage.out_ptr());
    }, c->stage.out, out, bytes);
}

}  // namespace thfhe

#pragma GCC visibility pop

#endif  // THFHE_DEVCTX_H
