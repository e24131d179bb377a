// thfhe_mk_shared.h -- kernels shared by the multi-key schemes (3-gen: thfhe_mk.hip, CCS: thfhe_ccs.hip): the gate's linear
// prologue + mod-switch on (n, P) mask matrices.  The per-party key switch is in thfhe_keyswitch.h.
#ifndef THFHE_MK_SHARED_H
#define THFHE_MK_SHARED_H

#include <hip/hip_runtime.h>

#include "../../include/thfhe_hip.h"
#include "thfhe_common.h"
#include "thfhe_keyswitch.h"
#include "thfhe_lane.h"

namespace {
using namespace thfhe;

// ------------------------------------------------------------------------------------------------------
// prologue: tmp = (0, cb) + cx x + cy y + cz z ; bara[job][P*n], barb[job]
// ------------------------------------------------------------------------------------------------------
struct MKLin {
    int32_t cb, cx, cy, cz;
};
__host__ __device__ inline bool mk_gate_lin(int op, int which, MKLin &L) {
    const int32_t E8 = 1 << 29, E4 = 1 << 30;
    switch (op) {
    case THFHE_NAND: L = MKLin{E8, -1, -1, 0}; return true;   // J/3gen_mk_gates.jl:8-14
    case THFHE_OR: L = MKLin{E8, 1, 1, 0}; return true;       // :24-30
    case THFHE_AND: L = MKLin{-E8, 1, 1, 0}; return true;     // :40-46
    case THFHE_XOR: L = MKLin{E4, 2, 2, 0}; return true;      // :68-74
    case THFHE_AND3: L = MKLin{-E4, 1, 1, 1}; return true;    // :55-64
    case THFHE_MUX: L = which == 0 ? MKLin{-E8, 1, 1, 0} : MKLin{-E8, -1, 0, 1}; return true;  // :133-150 (two ANDs)
    case kOpIdentity: L = MKLin{0, 1, 0, 0}; return true;
    default: return false;
    }
}
__global__ __launch_bounds__(256) void mk_prologue_kernel(const int32_t *__restrict__ in0, const int32_t *__restrict__ in1,
                                                           const int32_t *__restrict__ in2, MKLin L0, MKLin L1, const int32_t *__restrict__ ops,
                                                           int rot_per_gate, int words, int w_pad, int log2_2n, long jobs,
                                                           int32_t *__restrict__ bara, int32_t *__restrict__ barb) {
    const long job = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (job >= jobs || i > words) return;
    const long gate = job / rot_per_gate;
    MKLin L = (job % rot_per_gate) == 0 ? L0 : L1;
    if (ops) mk_gate_lin(ops[gate], 0, L);  // per-gate opcodes of a mixed DAG level (validated on the host)
    const size_t off = (size_t)gate * (words + 1) + i;
    uint32_t v = (uint32_t)L.cx * (uint32_t)in0[off];
    if (L.cy != 0) v += (uint32_t)L.cy * (uint32_t)in1[off];
    if (L.cz != 0) v += (uint32_t)L.cz * (uint32_t)in2[off];
    if (i == words) {
        v += (uint32_t)L.cb;
        barb[job] = modswitch2n((int32_t)v, log2_2n);
    } else {
        bara[job * w_pad + i] = modswitch2n((int32_t)v, log2_2n);
    }
}

}  // namespace

#endif  // THFHE_MK_SHARED_H
