// Host check of the rotation-kernel rules (torus-fhe_amd/csrc/thfhe_launch_plan.h), the header the launchers and the
// thfhe_*_rotation_kernel_name calls share.  Usage: launch_plan_test NAMES_FILE [N:l:Bgbit ...]
//   single key   l = 1 .. 4, jobs = 0 .. 6200 (three rounds plus every remainder), nine (coop_max, ring4_max) pairs: the pieces are at most 3,
//                contiguous, disjoint and cover [0, jobs) exactly; every ring8 piece but a trailing one is a multiple of 2048; a coop piece
//                that follows a ring4 piece holds at most min(coop_max, 256) jobs
//   3-gen        every N:l:Bgbit given, parts / batched from mk_digit_parts, rotations x pair thresholds
//   KMS, CCS     the same grid; five (parties, l) shapes
// Every name goes to NAMES_FILE, one case per line, for tests/test_launch_plan.py to compare with its frozen copy of the rules this header
// replaced; one JSON line on stdout.  CPU only; built with -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../torus-fhe_amd/csrc/thfhe_launch_plan.h"

namespace LP = thfhe::launch_plan;

static long errors = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            if (errors++ < 20) {                          \
                std::fprintf(stderr, "FAILED %s: ", #cond); \
                std::fprintf(stderr, __VA_ARGS__);        \
                std::fprintf(stderr, "\n");               \
            }                                             \
        }                                                 \
    } while (0)

static void check_plan(long jobs, int coop, int ring4) {
    LP::SkPiece pc[LP::kMaxPieces];
    const int n = LP::sk_rotation_plan(jobs, coop, ring4, pc);
    CHECK(n >= 0 && n <= 3, "jobs %ld coop %d ring4 %d: %d pieces", jobs, coop, ring4, n);
    long next = 0;
    for (int i = 0; i < n && i < LP::kMaxPieces; i++) {
        CHECK(pc[i].first == next && pc[i].count > 0, "jobs %ld coop %d ring4 %d: piece %d is [%ld, +%ld), expected to start at %ld", jobs, coop, ring4, i,
              pc[i].first, pc[i].count, next);
        next = pc[i].first + pc[i].count;
        if (pc[i].shape == LP::kRing8 && i + 1 < n) CHECK(pc[i].count % 2048 == 0, "jobs %ld coop %d ring4 %d: ring8 piece %d of %ld jobs is not whole rounds", jobs, coop, ring4, i, pc[i].count);
        if (pc[i].shape == LP::kCoop && i > 0 && pc[i - 1].shape == LP::kRing4)
            CHECK(pc[i].count <= (coop < 256 ? coop : 256), "jobs %ld coop %d ring4 %d: %ld coop jobs after a ring4 piece", jobs, coop, ring4, pc[i].count);
    }
    CHECK(next == jobs, "jobs %ld coop %d ring4 %d: pieces cover [0, %ld)", jobs, coop, ring4, next);
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    std::FILE *out = std::fopen(argv[1], "w");
    if (!out) return 2;
    char name[64], tiny[8];
    long names = 0, plans = 0;

    const int sk_thresholds[9][2] = {{768, 1024}, {0, 0}, {0, 1024}, {768, 0}, {1 << 20, 1024}, {6, 6}, {100, 6}, {200, 1024}, {300, 1024}};
    for (const auto &t : sk_thresholds)
        for (long jobs = 0; jobs <= 6200; jobs++) {
            check_plan(jobs, t[0], t[1]), plans++;
            for (int l = 1; l <= 4; l++) {
                const int need = LP::sk_kernel_name(l, jobs, t[0], t[1], name, sizeof name);
                CHECK(need > 0 && need < (int)sizeof name && (int)std::strlen(name) == need, "sk name length %d", need);
                std::fprintf(out, "sk %d %d %d %ld %s\n", l, t[0], t[1], jobs, name), names++;
            }
        }
    // a buffer too short is reported by the return value and never overrun (the sanitizer watches `tiny`)
    CHECK(LP::sk_kernel_name(2, 5, 768, 1024, tiny, sizeof tiny) >= (int)sizeof tiny && std::strlen(tiny) == sizeof tiny - 1, "short buffer");
    CHECK(LP::ccs_kernel_name(true, tiny, sizeof tiny) >= (int)sizeof tiny, "short buffer");

    const long rotations[4] = {1, 256, 257, 5000}, thresholds[3] = {0, 256, 1L << 20};
    for (int i = 2; i < argc; i++) {
        int N, l, Bgbit;
        if (std::sscanf(argv[i], "%d:%d:%d", &N, &l, &Bgbit) != 3) return 2;
        const LP::MkDigitParts d = LP::mk_digit_parts(N, l, Bgbit);
        CHECK(d.parts >= 1 && (d.parts == 1) == (d.pw == 0) && d.parts * (d.parts > 1 ? d.pw : Bgbit) >= Bgbit, "%s: parts %d of %d bits", argv[i], d.parts, d.pw);
        for (long thr : thresholds)
            for (long rot : rotations) {
                const int need = LP::mk_kernel_name(N, l, d.parts, d.batched, rot, thr, name, sizeof name);
                CHECK(need > 0 && need < (int)sizeof name, "mk name length %d", need);
                std::fprintf(out, "mk %d %d %d %ld %ld %s\n", N, l, Bgbit, thr, rot, name), names++;
            }
    }
    for (long thr : thresholds)
        for (long rot : rotations) {
            CHECK(LP::kms_kernel_name(rot, thr, name, sizeof name) < (int)sizeof name, "kms name length");
            std::fprintf(out, "kms %ld %ld %s\n", thr, rot, name), names++;
        }
    const int ccs_shapes[5][2] = {{2, 3}, {8, 8}, {9, 3}, {16, 3}, {4, 9}};
    for (const auto &s : ccs_shapes) {
        CHECK(LP::ccs_kernel_name(LP::ccs_wide(s[0], s[1]), name, sizeof name) < (int)sizeof name, "ccs name length");
        std::fprintf(out, "ccs %d %d %s\n", s[0], s[1], name), names++;
    }
    if (std::fclose(out) != 0) return 2;
    std::printf("{\"errors\": %ld, \"sk_plans\": %ld, \"names\": %ld}\n", errors, plans, names);
    return errors ? 1 : 0;
}
