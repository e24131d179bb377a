// mk_pack_wide_emu.cpp -- TEST INFRASTRUCTURE ONLY (never linked into libthfhe_hip.so).  Host replay of mk_pack_rows_wide_kernel
// (torus-fhe_amd/csrc/thfhe_mk_pack.h): workgroup by workgroup (record group of 32, column tile of 256 words), chunk by chunk of 256
// mask words, the walk over (j, p, v) with the membership mask of digit value v built from mkp_round_word / mkp_digit_is as the wave's ballot
// builds it (lane L votes for record L mod 32, the low 32 bits are kept), the row tile (j, p, v - 1) touched only when the mask is not empty and
// subtracted under the all-ones / zero word of each record's bit.  tests/test_mk_pack_wide_emu.py compiles it and compares with the numpy model.
#include <algorithm>
#include <cstdint>
#include <vector>

#include "../../torus-fhe_amd/csrc/thfhe_mk_pack.h"

using namespace thfhe;

extern "C" {
// T[count][2N] from recs[count][D + 1] and pk[D][t][R][2N].  loads: the row tiles fetched, summed over the workgroups (one per non-empty mask)
void mk_pack_wide_emu_rows(const int32_t *recs, long count, const int64_t *pk, int D, int t, int basebit, int N, int64_t *T, long *loads) {
    constexpr int G = kMkPackWideGroup;
    const int R = (1 << basebit) - 1;
    const size_t row = 2 * (size_t)N, rec = (size_t)D + 1;
    long n_loads = 0;
    std::vector<uint32_t> sA(256 * (G + 1));
    std::vector<uint64_t> s(256 * G);
    for (long g0 = 0; g0 < count; g0 += G) {
        const int ng = (int)(count - g0 < G ? count - g0 : G);
        for (int tile = 0; tile < 2 * N / kMkPackWideTile; tile++) {
            std::fill(s.begin(), s.end(), 0);
            for (int j0 = 0; j0 < D; j0 += 256) {
                const int jn = D - j0 < 256 ? D - j0 : 256;
                for (int tid = 0; tid < 256; tid++)
                    for (int g = 0; g < G; g++)
                        sA[tid * (G + 1) + g] = mkp_round_word(g < ng && tid < jn ? recs[(size_t)(g0 + g) * rec + j0 + tid] : 0, t, basebit);
                for (int jj = 0; jj < jn; jj++)
                    for (int p = 0; p < t; p++)
                        for (int v = 1; v <= R; v++) {
                            uint64_t ballot = 0;   // of one wave: every wave of the workgroup builds the same one
                            for (int lane = 0; lane < 64; lane++)
                                ballot |= (uint64_t)mkp_digit_is(sA[jj * (G + 1) + (lane & (G - 1))], p, basebit, v) << lane;
                            const uint32_t m = (uint32_t)ballot;
                            if (m == 0) continue;
                            n_loads++;
                            for (int tid = 0; tid < 256; tid++) {
                                const uint64_t x = (uint64_t)pk[(((size_t)(j0 + jj) * t + p) * R + (v - 1)) * row + tile * kMkPackWideTile + tid];
                                for (int g = 0; g < G; g++) {
                                    const uint32_t sel = 0u - ((m >> g) & 1u);
                                    s[tid * G + g] -= x & (((uint64_t)sel << 32) | sel);
                                }
                            }
                        }
            }
            for (int tid = 0; tid < 256; tid++) {
                const int col = tile * kMkPackWideTile + tid;
                for (int g = 0; g < ng; g++) {
                    uint64_t v = s[tid * G + g];
                    if (col == N) v += (uint64_t)(int64_t)recs[(size_t)(g0 + g) * rec + D] << 32;
                    T[(size_t)(g0 + g) * row + col] = (int64_t)v;
                }
            }
        }
    }
    if (loads) *loads = n_loads;
}

int mk_pack_wide_emu_group() { return kMkPackWideGroup; }
int mk_pack_wide_emu_tile() { return kMkPackWideTile; }
}
