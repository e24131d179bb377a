// thfhe_linear_plan.h -- how a dense-layer call (thfhe_lwe_linear, thfhe_linear_lut_bootstrap and their thfhe_mk_ forms) is cut
// into slices: which samples go in which slice and where a slice's inputs and records lie in the host arrays.  Pure host arithmetic, no HIP,
// so that it can be tested on its own (tests/cpp/linear_plan_test.cpp).
#ifndef THFHE_LINEAR_PLAN_H
#define THFHE_LINEAR_PLAN_H

#include <cstddef>

namespace thfhe {
namespace linear_plan {

// A slice holds whole samples: as many as keep its PBS jobs (samples x M outputs) within `cap`, at least one (a sample with M > cap runs alone
// and exceeds it), never more than the call has.  count >= 1, M >= 1.
inline size_t samples_per_slice(size_t count, size_t M, size_t cap) {
    const size_t fit = cap / M;
    const size_t S = fit < 1 ? 1 : fit;
    return S < count ? S : count;
}

inline size_t n_slices(size_t count, size_t S_max) { return (count + S_max - 1) / S_max; }

// Slice i of a call: samples [s0, s0 + S), its S M jobs, and the word offsets of its part of in[count][K][rec] and of out[count][M][theta][out_rec]
// (out_rec: the words of an output record; a linear-only call has theta = 1).
struct Slice {
    size_t s0, S, jobs, in_off, out_off;
};
inline Slice slice_at(size_t i, size_t count, size_t S_max, size_t M, size_t K, size_t theta, size_t rec, size_t out_rec) {
    Slice s;
    s.s0 = i * S_max;
    s.S = count - s.s0 < S_max ? count - s.s0 : S_max;
    s.jobs = s.S * M;
    s.in_off = s.s0 * K * rec;
    s.out_off = s.s0 * M * theta * out_rec;
    return s;
}

}  // namespace linear_plan
}  // namespace thfhe

#endif  // THFHE_LINEAR_PLAN_H
