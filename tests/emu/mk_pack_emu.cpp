// mk_pack_emu.cpp -- TEST INFRASTRUCTURE ONLY (never linked into libthfhe_hip.so).  Host replay of the multi-key packing key switch of the 3-gen
// engine (torus-fhe_amd/csrc/thfhe_mk_pack.h): the digit with its rounding offset, the box source index and sign, and the prefix rule of the
// negacyclic extension -- the functions mk_pack_rows_kernel and mk_pack_boxes_kernel call -- looping over the kernels' threads, so that they are
// checked against numpy in the `-m "not gpu"` suite.  tests/test_mk_pack_lane_emu.py compiles it.
#include <cstdint>
#include <vector>

#include "../../torus-fhe_amd/csrc/thfhe_mk_pack.h"

using namespace thfhe;

extern "C" {
// d[count][t]: the digits of every word, most significant first
void mk_pack_emu_digits(const int32_t *a, long count, int t, int basebit, int32_t *d) {
    for (long i = 0; i < count; i++) {
        const uint32_t w = mkp_round_word(a[i], t, basebit);
        for (int p = 0; p < t; p++) d[i * t + p] = mkp_digit(w, p, basebit);
    }
}

// mk_pack_rows_kernel: T[count][2N] from recs[count][D + 1] and pk[D][t][R][2N], workgroup by workgroup (record group, column tile), lane by lane
void mk_pack_emu_rows(const int32_t *recs, long count, const int64_t *pk, int D, int t, int basebit, int N, int64_t *T) {
    const int R = (1 << basebit) - 1;
    const size_t row = 2 * (size_t)N, rec = (size_t)D + 1;
    for (long g0 = 0; g0 < count; g0 += kMkPackGroup)
        for (int tile = 0; tile < 2 * N / kMkPackTile; tile++)
            for (int tid = 0; tid < 256; tid++) {
                const int col = tile * kMkPackTile + 2 * tid;
                for (int g = 0; g < kMkPackGroup && g0 + g < count; g++) {
                    uint64_t s0 = 0, s1 = 0;
                    for (int j = 0; j < D; j++) {
                        const uint32_t w = mkp_round_word(recs[(size_t)(g0 + g) * rec + j], t, basebit);
                        for (int p = 0; p < t; p++) {
                            const int d = mkp_digit(w, p, basebit);
                            if (d == 0) continue;
                            const int64_t *v = pk + (((size_t)j * t + p) * R + (d - 1)) * row + col;
                            s0 -= (uint64_t)v[0], s1 -= (uint64_t)v[1];
                        }
                    }
                    if (col == N) s0 += (uint64_t)(int64_t)recs[(size_t)(g0 + g) * rec + D] << 32;
                    T[(size_t)(g0 + g) * row + col] = (int64_t)s0, T[(size_t)(g0 + g) * row + col + 1] = (int64_t)s1;
                }
            }
}

// mk_pack_boxes_kernel of one output: T[p][2][N] -> out_a[N], out_b[N]; the scan is a plain running sum (its result is what the kernel's
// Hillis-Steele scan leaves in LDS).  0 on a ring degree the kernel is not instantiated for.
int mk_pack_emu_boxes(int N, const int64_t *T, int p, int64_t *out_a, int64_t *out_b) {
    if (N != 1024 && N != 2048 && N != 4096) return 0;
    const int B = N / p;
    std::vector<uint64_t> pre(N);
    for (int poly = 0; poly < 2; poly++) {
        const uint64_t *src = reinterpret_cast<const uint64_t *>(T) + (size_t)poly * N;
        for (int c = 0; c < N; c++) {
            uint64_t acc = 0;
            for (int i = 0; i < p; i++) {
                bool neg;
                const int e = mkp_box_src(c, i, B, N, &neg);
                const uint64_t v = src[(size_t)i * 2 * N + e];
                acc += neg ? 0ull - v : v;
            }
            pre[c] = acc + (c ? pre[c - 1] : 0);
        }
        const uint64_t tot = pre[N - 1];
        for (int c = 0; c < N; c++) (poly ? out_b : out_a)[c] = (int64_t)mkp_window(pre.data(), tot, c, B, N);
    }
    return 1;
}
}
