// mk_mv_emu.cpp -- TEST INFRASTRUCTURE ONLY (never linked into libthfhe_hip.so).  Host replay of the multi-value epilogue of the 3-gen multi-key
// engine (torus-fhe_amd/csrc/thfhe_lane.h: extract_mv64, the body of mk_extract_mv_kernel in thfhe_mk.hip), looping over the 256 threads of its
// workgroup, so that its index and sign maps and the order "combine in Torus64, then convert" are checked against numpy in the `-m "not gpu"`
// suite.  tests/test_mk_mv_lane_emu.py compiles it.
#include <cstdint>

#include "../../torus-fhe_amd/csrc/thfhe_lane.h"

using namespace thfhe;

namespace {
// the kernel's staging and its loop over the outputs: the mask polynomial and the p body words the taps meet, then q calls per thread
template <int NN>
void extract(const int64_t *acc, const int32_t *c, int p, int q, int64_t out_bias, int32_t *out) {
    int64_t body[64];
    const int box = NN / p;
    for (int k = 0; k < p; k++) body[k] = acc[NN + NN - (box >> 1) - k * box];
    for (int j = 0; j < q; j++)
        for (int tid = 0; tid < 256; tid++) extract_mv64<NN>(tid, acc, body, c + j * p, p, out_bias, out + (long)j * (NN + 1));
}
}  // namespace

extern "C" {
// out[q][N+1]: the q outputs of one accumulator int64[2][N], taps c[q][p]; 0 on a ring degree the kernel is not instantiated for
int mk_mv_emu_extract(int N, const int64_t *acc, const int32_t *c, int p, int q, int64_t out_bias, int32_t *out) {
    switch (N) {
    case 1024: extract<1024>(acc, c, p, q, out_bias, out); return 1;
    case 2048: extract<2048>(acc, c, p, q, out_bias, out); return 1;
    case 4096: extract<4096>(acc, c, p, q, out_bias, out); return 1;
    default: return 0;
    }
}
}
