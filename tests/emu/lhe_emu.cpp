// Test-only host replay of the leveled CMux's digit helper (torus-fhe_amd/csrc/thfhe_lane.h: diff_digits_z), lane by lane over a wavefront
// (tests/test_lhe_lane_emu.py).  Never linked into libthfhe_hip.so.
#include "../../torus-fhe_amd/csrc/thfhe_lane.h"

using namespace thfhe;

// digits[(level - 1) * 1024 + q] = digit `level` of (p1 - p0)[q], q < 1024, from the folded values the 64 lanes produce
extern "C" void lhe_emu_diff_digits(const int32_t *p1, const int32_t *p0, int l, int Bgbit, int32_t *digits) {
    for (int level = 1; level <= l; level++)
        for (int lane = 0; lane < kLanes; lane++) {
            cplx z[8];
            diff_digits_z(lane, p1, p0, level, l, Bgbit, z);
            for (int m = 0; m < 8; m++) {
                digits[(level - 1) * 1024 + lane + 64 * m] = (int32_t)z[m].re;
                digits[(level - 1) * 1024 + lane + 64 * m + 512] = (int32_t)z[m].im;
            }
        }
}
