// mv_emu.cpp -- TEST INFRASTRUCTURE ONLY (never linked into libthfhe_hip.so).  Host replay of the multi-value epilogue of the blind-rotate
// kernels (torus-fhe_amd/csrc/thfhe_lane.h: acc_init_tv16, extract_mv16), looping over the 64 lanes of a wavefront, so that its index and
// sign maps are checked against numpy in the `-m "not gpu"` suite.  tests/test_mv_lane_emu.py compiles it.
#include <cstdint>

#include "../../torus-fhe_amd/csrc/thfhe_lane.h"

using namespace thfhe;

extern "C" {
// acc = (0, X^{-barb} tv0), int32[2][1024]
void mv_emu_init(int32_t *acc, int barb, const int32_t *tv0) {
    for (int lane = 0; lane < 64; lane++) acc_init_tv16(lane, acc, acc + 1024, barb, tv0);
}
// out[q][1025]: the q outputs of one accumulator, taps c[q][p]; the loop over j is the ring kernels' (one wave), the cooperative kernel's
// eight waves take j = wave, wave + 8, ... of the same calls
void mv_emu_extract(const int32_t *acc, const int32_t *c, int p, int q, int32_t *out) {
    for (int j = 0; j < q; j++)
        for (int lane = 0; lane < 64; lane++) extract_mv16(lane, acc, acc + 1024, c + j * p, p, 1024 / p, out + j * 1025);
}
}
