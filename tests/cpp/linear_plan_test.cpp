// Host check of the dense-layer slice planner (torus-fhe_amd/csrc/thfhe_linear_plan.h), the header ctx_linear cuts its calls with.
// For a grid of (count, M, K, theta, cap, rec, out_rec): the slices cover samples 0 .. count exactly once and in order, hold whole samples (at
// least one), keep S M within the cap unless one sample alone exceeds it (then the slice holds exactly that sample), take as many samples as the
// cap admits (only the last slice may be shorter), and their input / output word offsets are those of the first sample they hold -- at count = 1
// and with M theta above the cap too.  One JSON line on stdout.  CPU only; built with -fsanitize=address,undefined.
#include <cstddef>
#include <cstdio>
#include <vector>

#include "../../torus-fhe_amd/csrc/thfhe_linear_plan.h"

namespace LP = thfhe::linear_plan;

static long errors = 0, plans = 0;
#define CHECK(cond, ...)                                    \
    do {                                                    \
        if (!(cond)) {                                      \
            if (errors++ < 20) {                            \
                std::fprintf(stderr, "FAILED %s: ", #cond); \
                std::fprintf(stderr, __VA_ARGS__);          \
                std::fprintf(stderr, "\n");                 \
            }                                               \
        }                                                   \
    } while (0)

static void check(size_t count, size_t M, size_t K, size_t theta, size_t cap, size_t rec, size_t out_rec) {
    plans++;
    const size_t S_max = LP::samples_per_slice(count, M, cap);
    CHECK(S_max >= 1 && S_max <= count, "count %zu M %zu cap %zu: S_max %zu", count, M, cap, S_max);
    if (S_max < 1) return;
    if (M > cap) CHECK(S_max == 1, "count %zu M %zu cap %zu: a sample above the cap must run alone, S_max %zu", count, M, cap, S_max);
    else CHECK(S_max * M <= cap && (S_max == count || (S_max + 1) * M > cap), "count %zu M %zu cap %zu: S_max %zu is not the most the cap admits", count, M, cap, S_max);
    const size_t n = LP::n_slices(count, S_max);
    std::vector<unsigned char> seen(count, 0);   // the sanitizer watches every index the plan produces
    size_t next = 0;
    for (size_t i = 0; i < n; i++) {
        const LP::Slice s = LP::slice_at(i, count, S_max, M, K, theta, rec, out_rec);
        CHECK(s.s0 == next && s.S >= 1 && s.s0 + s.S <= count, "count %zu M %zu cap %zu: slice %zu is [%zu, +%zu), expected to start at %zu", count, M, cap, i, s.s0, s.S, next);
        if (s.s0 != next || s.S < 1 || s.s0 + s.S > count) return;
        CHECK(i + 1 == n || s.S == S_max, "count %zu M %zu cap %zu: slice %zu of %zu is short (%zu of %zu samples)", count, M, cap, i, n, s.S, S_max);
        CHECK(s.jobs == s.S * M && (s.jobs <= cap || s.S == 1), "count %zu M %zu cap %zu: slice %zu holds %zu jobs", count, M, cap, i, s.jobs);
        CHECK(s.in_off == s.s0 * K * rec, "count %zu K %zu rec %zu: slice %zu reads from word %zu", count, K, rec, i, s.in_off);
        CHECK(s.out_off == s.s0 * M * theta * out_rec, "count %zu M %zu theta %zu: slice %zu writes at word %zu", count, M, theta, i, s.out_off);
        for (size_t q = 0; q < s.S; q++) seen[s.s0 + q]++;
        next = s.s0 + s.S;
    }
    CHECK(next == count, "count %zu M %zu cap %zu: the slices end at sample %zu", count, M, cap, next);
    for (size_t q = 0; q < count; q++) CHECK(seen[q] == 1, "count %zu M %zu cap %zu: sample %zu is in %d slices", count, M, cap, q, (int)seen[q]);
}

int main() {
    const size_t counts[] = {1, 2, 3, 4, 5, 7, 11, 32, 33, 100, 4097};
    const size_t Ms[] = {1, 2, 3, 5, 16, 17, 128, 65536};
    const size_t thetas[] = {1, 2, 4};
    for (size_t count : counts)
        for (size_t M : Ms)
            for (size_t theta : thetas) {
                const size_t mt = M * theta;
                const size_t caps[] = {1, M > 1 ? M - 1 : 1, M, M + 1, 2 * M, 2 * M + 1, mt > 1 ? mt - 1 : 1, mt, 2 * mt + 1, 4096, (size_t)1 << 20};
                for (size_t cap : caps) {
                    check(count, M, 4, theta, cap, 631, 631);
                    check(count, M, 784, theta, cap, 17, 1025);
                }
            }
    // the cases the contract names: one sample, and M theta above the cap (the sample still runs, alone, at offset 0)
    {
        const LP::Slice s = LP::slice_at(0, 1, LP::samples_per_slice(1, 5, 3), 5, 7, 4, 38, 38);
        CHECK(s.s0 == 0 && s.S == 1 && s.jobs == 5 && s.in_off == 0 && s.out_off == 0, "count 1: [%zu, +%zu) jobs %zu in %zu out %zu", s.s0, s.S, s.jobs, s.in_off, s.out_off);
        const size_t S_max = LP::samples_per_slice(3, 5, 19);   // M theta = 20 > 19 >= M: three samples a slice by jobs, so one slice
        const LP::Slice t = LP::slice_at(0, 3, S_max, 5, 7, 4, 38, 1025);
        CHECK(S_max == 3 && t.S == 3 && t.jobs == 15, "cap 19 on M 5: S_max %zu", S_max);
        const LP::Slice u = LP::slice_at(2, 3, LP::samples_per_slice(3, 5, 4), 5, 7, 4, 38, 1025);   // M = 5 > 4: one sample a slice
        CHECK(u.s0 == 2 && u.S == 1 && u.in_off == 2 * 7 * 38 && u.out_off == (size_t)2 * 5 * 4 * 1025, "third slice: s0 %zu in %zu out %zu", u.s0, u.in_off, u.out_off);
    }
    std::printf("{\"plans\": %ld, \"errors\": %ld}\n", plans, errors);
    return errors ? 1 : 0;
}
