// thfhe_common.h -- shared host/device helpers of libthfhe_hip.so (error plumbing, wave-level transform drivers).
#ifndef THFHE_COMMON_H
#define THFHE_COMMON_H

#include <hip/hip_runtime.h>

#include <type_traits>

#include "../../include/thfhe_hip.h"
#include "thfhe_lane.h"

namespace thfhe {

constexpr int kOpIdentity = 100;  // internal opcode: tmp = x (plain bootstrap of a sample)

int thfhe_fail(int code, const char *msg);
int thfhe_fail_hip(hipError_t e, const char *what);

inline int ilog2(int x) {
    int l = 0;
    while ((1 << l) < x) l++;
    return l;
}

// Host-side checks of a programmable-bootstrap call, before any device work: null pointers first (no context needed), then the spec and
// every lut_index entry (the kernel cannot report an index out of range).  Shared by thfhe_lut_bootstrap (tv int32) and
// thfhe_mk_lut_bootstrap (tv int64); thfhe_lut_bootstrap_enc raises the table cap (max_luts).
inline int lut_validate(const thfhe_lut_spec *sp, const void *tv, int n_luts, const int32_t *lut_index, const int32_t *in0, const int32_t *in1,
                        const int32_t *in2, const int32_t *out, size_t count, int max_luts = 1024) {
    if (!sp || !tv || !in0 || !out) return thfhe_fail(THFHE_E_INVALID, "null argument");
    if (sp->n_inputs < 1 || sp->n_inputs > 3) return thfhe_fail(THFHE_E_INVALID, "lut spec: n_inputs must be 1, 2 or 3");
    if ((sp->n_inputs > 1 && !in1) || (sp->n_inputs > 2 && !in2)) return thfhe_fail(THFHE_E_INVALID, "null operand: the spec names more inputs");
    if (sp->theta != 1 && sp->theta != 2 && sp->theta != 4) return thfhe_fail(THFHE_E_INVALID, "lut spec: theta must be 1, 2 or 4");
    if (n_luts < 1 || n_luts > max_luts) return thfhe_fail(THFHE_E_INVALID, max_luts == 1024 ? "n_luts must be 1 .. 1024" : "n_luts must be 1 .. 262144");
    if (count > (size_t)INT32_MAX / 16) return thfhe_fail(THFHE_E_INVALID, "count too large");
    if (lut_index)
        for (size_t g = 0; g < count; g++)
            if (lut_index[g] < 0 || lut_index[g] >= n_luts) return thfhe_fail(THFHE_E_INVALID, "lut_index out of range (0 .. n_luts-1)");
    return THFHE_OK;
}

// The spec rules of lut_validate on their own (the gate-DAG LUT nodes, thfhe_dag.h): n_inputs 1 .. 3, theta 1, 2 or 4.
inline int lut_spec_check(const thfhe_lut_spec &sp) {
    if (sp.n_inputs < 1 || sp.n_inputs > 3) return thfhe_fail(THFHE_E_INVALID, "lut spec: n_inputs must be 1, 2 or 3");
    if (sp.theta != 1 && sp.theta != 2 && sp.theta != 4) return thfhe_fail(THFHE_E_INVALID, "lut spec: theta must be 1, 2 or 4");
    return THFHE_OK;
}

#define THFHE_HIP(expr)                                                    \
    do {                                                                   \
        hipError_t thfhe_e_ = (expr);                                      \
        if (thfhe_e_ != hipSuccess) return ::thfhe::thfhe_fail_hip(thfhe_e_, #expr); \
    } while (0)

// A runtime template argument: calls f(std::integral_constant<int, v>{}) for v in 1 .. Max, so that f can launch kernel<v>; kernel<1> ..
// kernel<Max> are instantiated and no other.  Any other v fails with `unsupported`.
template <int Max, int V = 1, class F>
int with_static_int(int v, const char *unsupported, F &&f) {
    if constexpr (V > Max) return thfhe_fail(THFHE_E_UNSUPPORTED, unsupported);
    else if (v == V) {
        f(std::integral_constant<int, V>{});
        return THFHE_OK;
    } else return with_static_int<Max, V + 1>(v, unsupported, f);
}
constexpr const char *kBadL = "decomposition length l must be 1..4";

// the end of a thfhe_*_rotation_kernel_name call: `need` is what the name writer of thfhe_launch_plan.h returned (the name's length)
inline int kernel_name_result(int len, int need) {
    return need < len ? THFHE_OK : thfhe_fail(THFHE_E_INVALID, "buffer too short for the kernel name");
}

#if defined(__HIPCC__)
#ifdef THFHE_STAMPS
// Diagnostic build only (make stamps -> torus-fhe_amd/lib/libthfhe_hip_stamps.so, never shipped): per-wave cycle totals of the phases of
// the ring kernel's CMux loop, s_memtime deltas summed over all CMuxes; read back with thfhe_debug_read_stamps.
#define THFHE_STAMP_STORAGE __device__ unsigned long long g_stamps[8 * 2048 * 8];
#define STAMP_DECL unsigned long long st_acc[6] = {0, 0, 0, 0, 0, 0}, st_t = __builtin_amdgcn_s_memtime()
#define STAMP(slot)                                              \
    do {                                                         \
        unsigned long long now_ = __builtin_amdgcn_s_memtime();  \
        st_acc[slot] += now_ - st_t;                             \
        st_t = now_;                                             \
    } while (0)
#define STAMP_FLUSH(wg, wave)                                                                                  \
    do {                                                                                                       \
        if (lane == 0 && (wg) < 2048)                                                                          \
            for (int q_ = 0; q_ < 6; q_++) g_stamps[(((size_t)(wg)) * 8 + (wave)) * 8 + q_] = st_acc[q_];       \
    } while (0)
#else
#define THFHE_STAMP_STORAGE
#define STAMP_DECL
#define STAMP(slot)
#define STAMP_FLUSH(wg, wave)
#endif


// Wave-level ordering point between two LDS segments.  One wavefront's DS instructions execute in issue order,
// so no hardware barrier is needed -- this only stops the compiler from moving LDS accesses across the exchange.
// The fences are scoped to the LDS address space so that global (bootstrapping-key) loads may be scheduled across them.
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront", "local");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront", "local");
}

// The lane index behind an empty asm: everything derived from it (the XOR-swizzled LDS slot maps: ~25 addresses of 1-3 integer
// instructions each) is recomputed where it is used.  Without it the compiler hoists those addresses out of the CMux loop as
// loop invariants and, being at the VGPR limit, spills them to scratch.
__device__ __forceinline__ int opaque_lane(int lane) {
    asm volatile("" : "+v"(lane));
    return lane;
}
// Wave-uniform words that no kernel of the launch writes (the mod-switched mask words a rotation walks: written by the prologue kernel before it):
// read through the constant address space, i.e. with s_load_dword into an SGPR.  As plain global loads they were global_load_dword + s_waitcnt vmcnt(0)
// at the top of every CMux -- a vector-memory round trip on the sequential chain, and a vmcnt(0) that also waits for whatever the wave has in flight.
typedef const int32_t __attribute__((address_space(4))) *uniform_i32_ptr;
__device__ __forceinline__ uniform_i32_ptr as_uniform(const int32_t *p) { return (uniform_i32_ptr)(size_t)p; }

// ---- LDS key ring (shared by the single-key and multi-key ring kernels) --------------------------------------------
// One LDS-DMA of this wave's 1 KiB slice of a key chunk: lane l fetches 16 B at gptr_lane into LDS at lds_byte_off + 16 l.
// Inline asm on purpose: the compiler then neither waits vmcnt(0) before every ring read nor reorders the hand-off.  The LDS base
// travels in m0 as a register-constrained INPUT ("{m0}"): the compiler itself materialises the value in m0 and knows it is live there,
// so nothing is clobbered behind its back (round 3 wrote m0 inside the asm and listed it as a clobber, which LLVM calls undefined
// for a reserved register).  s_nop 0 = the one wait state gfx9 wants between an SALU write of m0 and an LDS-DMA.
// The address is in the scalar-base form: a wave-uniform 64-bit base in an SGPR pair (the stream position: advanced with scalar adds, no vector
// instruction per issue) plus the lane's 32-bit byte offset in ONE loop-invariant VGPR.  IMM is the instruction's immediate offset; the hardware adds
// it to the global address AND to the LDS address, which is what a wave's second slice of a chunk (four-wave shape: + 1 KiB on both sides) wants.
template <int IMM = 0>
__device__ __forceinline__ void ring_dma(uint64_t gbase_uniform, uint32_t lane_byte_off, uint32_t lds_byte_off) {
    static_assert(IMM >= 0 && IMM < 4096, "immediate offset of a global instruction");
    asm volatile("s_nop 0\n\tglobal_load_lds_dwordx4 %0, %1 offset:%3" ::"v"(lane_byte_off), "s"(gbase_uniform), "{m0}"(lds_byte_off), "n"(IMM) : "memory");
}
// Hand-off barrier of the ring: this wave's own slice of the chunk has landed (at most VM younger DMAs in flight), every LDS read it issued
// has returned, then the workgroup barrier.  The wait sits inside the asm: the compiler's wait-count pass then puts a conservative lgkmcnt(0) in front
// of the first multiply after the barrier, harmless in this order, where no read is pending there.  The form with the s_waitcnt and s_barrier builtins
// times the same (profiles/r04_ring_multiply_phase.md); the asm form is the one every round measured.
template <int VM>
__device__ __forceinline__ void ring_barrier() {
    asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" ::"n"(VM) : "memory");
}
__device__ __forceinline__ void wave_fft_fwd_s(int lane, cplx (&z)[8], cplx *xb, const cplx *T1, const W64 &w) {
    wave_sync();
    fwds_seg1(lane, z, xb, T1);
    wave_sync();
    fwds_seg2_ld(lane, z, xb);
    fwds_seg2_st(lane, z, xb, w);
    wave_sync();
    fwds_seg3(lane, z, xb);
}
__device__ __forceinline__ void wave_fft_inv_s(int lane, cplx (&z)[8], cplx *xb, const cplx *T1, const W64 &w) {
    wave_sync();
    invs_seg1(lane, z, xb, w);
    wave_sync();
    invs_seg2_ld(lane, z, xb);
    invs_seg2_st(lane, z, xb);
    wave_sync();
    invs_seg3(lane, z, xb, T1);
}
// variant "q" (padded buffer, pass-1 twiddles from per-lane roots: thfhe_lane.h): first transpose in registers.  Exchange of the register index (bits 2,1,0) with lane bits (5,4,3):
//   stage A  z[r] (r < 4) of the upper half-wave <-> z[r + 4] of the lower half-wave      v_permlane32_swap
//   stage B  z[r] (bit 1 clear) of the odd 16-lane rows <-> z[r + 2] of the even rows      v_permlane16_swap
//   stage C  lanes with bit 3 clear take z[r] (r even) of lane ^ 8 into z[r + 1], lanes with bit 3 set take z[r + 1] into z[r]
//            (row_ror:8 DPP moves, bank masks 0x3 / 0xC)
// The exchange is its own inverse.
// KEEP64 (the ring kernel's transforms): stage C is a swap, its first move overwrites what the second one reads, so one side is kept -- by the compiler
// as one v_mov_b32 per dword; with KEEP64 per DOUBLE, behind an empty asm on the 64-bit pair: one v_mov_b64 (gfx950 has no DPP move on a 64-bit
// register, so the two moves themselves stay per dword).  Same lanes, same values; 64 fewer vector instructions per CMux and wave there.  Not the
// default: the multi-key rotation kernels, at their register limit, spill with it.
template <bool KEEP64 = false>
__device__ __forceinline__ void wave_transpose_hi3(cplx (&z)[8]) {
    uint32_t w[8][4];
#pragma unroll
    for (int r = 0; r < 8; r++) __builtin_memcpy(w[r], &z[r], 16);
#pragma unroll
    for (int d = 0; d < 4; d++) {
#pragma unroll
        for (int r = 0; r < 4; r++) {
            auto q = __builtin_amdgcn_permlane32_swap(w[r][d], w[r + 4][d], false, false);
            w[r][d] = q[0];
            w[r + 4][d] = q[1];
        }
#pragma unroll
        for (int r = 0; r < 8; r++) {
            if (r & 2) continue;
            auto q = __builtin_amdgcn_permlane16_swap(w[r][d], w[r + 2][d], false, false);
            w[r][d] = q[0];
            w[r + 2][d] = q[1];
        }
        if constexpr (!KEEP64) {
#pragma unroll
            for (int r = 0; r < 8; r += 2) {
                const uint32_t a = w[r][d], b = w[r + 1][d];
                w[r + 1][d] = __builtin_amdgcn_update_dpp(b, a, 0x128, 0xF, 0x3, false);
                w[r][d] = __builtin_amdgcn_update_dpp(a, b, 0x128, 0xF, 0xC, false);
            }
        }
    }
    if constexpr (KEEP64) {
#pragma unroll
        for (int r = 0; r < 8; r += 2) {
#pragma unroll
            for (int k = 0; k < 2; k++) {
                uint64_t keep = (uint64_t)w[r + 1][2 * k] | (uint64_t)w[r + 1][2 * k + 1] << 32;
                asm("" : "+v"(keep));
#pragma unroll
                for (int h = 0; h < 2; h++) {
                    const int d = 2 * k + h;
                    const uint32_t a = w[r][d], b = w[r + 1][d], kept = (uint32_t)(keep >> (32 * h));
                    w[r + 1][d] = __builtin_amdgcn_update_dpp(b, a, 0x128, 0xF, 0x3, false);
                    w[r][d] = __builtin_amdgcn_update_dpp(a, kept, 0x128, 0xF, 0xC, false);
                }
            }
        }
    }
#pragma unroll
    for (int r = 0; r < 8; r++) __builtin_memcpy(&z[r], w[r], 16);
}
// forward "q"; the inverse (invr_seg1 | inv_seg2_ld, dft8<-1> | wave_transpose_hi3, invq_seg3) is written out where it is used, with key requests
// between its stages (sk_blind_rotate_coop_kernel, thfhe_lhe.h)
__device__ __forceinline__ void wave_fft_fwd_q(int lane, cplx (&z)[8], cplx *xb, const LaneRoots &r, const W64 &w) {
    fwdq_seg1(z, r);
    wave_transpose_hi3(z);
    wave_sync();
    fwdr_seg2_st(lane, z, xb, w);
    wave_sync();
    fwd_seg3(lane, z, xb);
}
// variant "x" (the ring kernel; thfhe_lane.h): the exchange of register bits (2, 1, 0) with lane bits (3, 5, 4).  Its own inverse.  The two swap
// stages are the expensive ones: a lane swap holds the vector pipe about twice as long as a DPP move (tools/probes/issue_probe.hip: 9.25 against
// 5.0 cycles per instruction for a wave alone, 13.0 against 8.9 beside an FP64 wave), and there is one per dword pair either way.
//   lane bit 3 <-> register bit 2   one unmasked row_ror:8 move per dword of registers 4 .. 7 (16 instructions): an exchange because the lanes with
//                                   bit 3 set hold the pairs (r, r + 4) the other way round, before and after (variants "x" and "p" in
//                                   thfhe_lane.h say who produces and who consumes the flipped names).  With natural names on every lane the stage
//                                   is two masked moves and a kept 64-bit copy per double, 40 instructions (tests/emu/exchange_emu.cpp keeps it)
//   lane bit 5 <-> register bit 1   v_permlane32_swap
//   lane bit 4 <-> register bit 0   v_permlane16_swap
__device__ __forceinline__ void wave_transpose_x3(cplx (&z)[8]) {
    uint32_t w[8][4];
#pragma unroll
    for (int r = 0; r < 8; r++) __builtin_memcpy(w[r], &z[r], 16);
#pragma unroll
    for (int r = 4; r < 8; r++)
#pragma unroll
        for (int d = 0; d < 4; d++) w[r][d] = __builtin_amdgcn_update_dpp(w[r][d], w[r][d], 0x128, 0xF, 0xF, false);
#pragma unroll
    for (int d = 0; d < 4; d++) {
#pragma unroll
        for (int r = 0; r < 8; r++) {
            if (r & 2) continue;
            auto q = __builtin_amdgcn_permlane32_swap(w[r][d], w[r + 2][d], false, false);
            w[r][d] = q[0];
            w[r + 2][d] = q[1];
        }
#pragma unroll
        for (int r = 0; r < 8; r += 2) {
            auto q = __builtin_amdgcn_permlane16_swap(w[r][d], w[r + 1][d], false, false);
            w[r][d] = q[0];
            w[r + 1][d] = q[1];
        }
    }
#pragma unroll
    for (int r = 0; r < 8; r++) __builtin_memcpy(&z[r], w[r], 16);
}
// Forward of the ring kernel: variant "p" (thfhe_lane.h), the unmasked exchange.  z = the coefficients nu + 64 m of nu = lane_nu(lane), r = the forward
// roots of nu, flip = lane_flip_x(lane); spectra come out at lane nu, register k2 -- times rho^(-32) on the lanes with bit 3 set, which the PHASED key
// copy (thfhe_ctx::d_bk_ring) undoes in the product.  Not for a kernel that multiplies with the plain key.
__device__ __forceinline__ void wave_fft_fwd_x(int lane, cplx (&z)[8], cplx *xb, const LaneRootsF &r, uint32_t flip) {
    fwdp_seg1(z, flip);
    wave_transpose_x3(z);
    wave_sync();
    fwdp_seg2_st(lane, z, xb, r, flip);
    wave_sync();
    fwdf_seg3(lane, z, xb, r);
}
// w = lane_w64_x, r = lane_roots_x, bc = make_untwist_x(r.b, flip); outputs: the coefficients nu + 64 m of lane nu = lane_nu(lane)
template <bool LEAN>
__device__ __forceinline__ void wave_fft_inv_x(int lane, cplx (&z)[8], cplx *xb, W64 &w, LaneRoots &r, uint32_t flip, const cplx (&bc)[4]) {
    if (LEAN) opaque_in_place(w.w1), opaque_in_place(r.s);
    wave_sync();
    invf_seg1(lane, z, xb);
    wave_sync();
    inv_seg2_ld(lane, z, xb);
    invf_seg2(z, w);
    wave_transpose_x3(z);
    invx_seg3_ring(z, r, flip, bc);
}
// variant "qs" (multi-key kernels, whose LDS has no room for padded buffers): first transpose in registers, pass-1 twiddles from the
// per-lane roots, second transpose through the XOR-swizzled 512-slot buffer -- one LDS crossing and no T1 table reads per transform
__device__ __forceinline__ void wave_fft_fwd_qs(int lane, cplx (&z)[8], cplx *xb, const LaneRoots &r, const W64 &w) {
    fwdq_seg1(z, r);
    wave_transpose_hi3(z);
    wave_sync();
    fwds_seg2_st(lane, z, xb, w);
    wave_sync();
    fwds_seg3(lane, z, xb);
}
__device__ __forceinline__ void wave_fft_inv_qs(int lane, cplx (&z)[8], cplx *xb, const LaneRoots &r, const W64 &w) {
    wave_sync();
    invs_seg1(lane, z, xb, w);
    wave_sync();
    invs_seg2_ld(lane, z, xb);
    dft8<-1>(z);
    wave_transpose_hi3(z);
    invq_seg3(z, r);
}
// N = 2048 halves: twisted 512-point transforms (thfhe_lane.h, "N = 2048" section); T1t = the table of twist T
template <int T>
__device__ __forceinline__ void wave_fft_fwd_t(int lane, cplx (&z)[8], cplx *xb, const cplx *T1t, const W64 &w) {
    wave_sync();
    fwdt_seg1<T>(lane, z, xb, T1t);
    wave_sync();
    fwds_seg2_ld(lane, z, xb);
    fwds_seg2_st(lane, z, xb, w);
    wave_sync();
    fwds_seg3(lane, z, xb);
}
template <int T>
__device__ __forceinline__ void wave_fft_inv_t(int lane, cplx (&z)[8], cplx *xb, const cplx *T1t, const W64 &w) {
    wave_sync();
    invs_seg1(lane, z, xb, w);
    wave_sync();
    invs_seg2_ld(lane, z, xb);
    invs_seg2_st(lane, z, xb);
    wave_sync();
    invt_seg3<T>(lane, z, xb, T1t);
}
// "qs" form of the twisted halves: first transpose in registers, pass-1 twiddles from per-lane roots (no T1 table), one LDS crossing
template <int T, int DEN = 32>
__device__ __forceinline__ void wave_fft_fwd_tq(int lane, cplx (&z)[8], cplx *xb, const LaneRoots &r, const W64 &w) {
    fwdtq_seg1<T, DEN>(z, r);
    wave_transpose_hi3(z);
    wave_sync();
    fwds_seg2_st(lane, z, xb, w);
    wave_sync();
    fwds_seg3(lane, z, xb);
}
template <int T, int DEN = 32>
__device__ __forceinline__ void wave_fft_inv_tq(int lane, cplx (&z)[8], cplx *xb, const LaneRoots &r, const W64 &w) {
    wave_sync();
    invs_seg1(lane, z, xb, w);
    wave_sync();
    invs_seg2_ld(lane, z, xb);
    dft8<-1>(z);
    wave_transpose_hi3(z);
    invtq_seg3<T, DEN>(z, r);
}

// Two transforms of one wave side by side.  A wavefront's DS instructions execute in issue order, so the second transform's arithmetic covers
// the first one's LDS round trip (and the other way round); the inverse pair shares ONE transpose buffer: the second one's stores may follow
// the first one's loads without a wait.
template <int TA, int TB, int DEN = 32>
__device__ __forceinline__ void wave_fft_fwd_tq_two(int lane, cplx (&za)[8], cplx (&zb)[8], cplx *xa, cplx *xb, const LaneRoots &ra, const LaneRoots &rb,
                                                    const W64 &w) {
    fwdtq_seg1<TA, DEN>(za, ra);
    fwdtq_seg1<TB, DEN>(zb, rb);
    wave_transpose_hi3(za);
    wave_transpose_hi3(zb);
    wave_sync();
    fwds_seg2_st(lane, za, xa, w);
    fwds_seg2_st(lane, zb, xb, w);
    wave_sync();
    fwds_seg3(lane, za, xa);
    fwds_seg3(lane, zb, xb);
}
template <int TA, int TB, int DEN = 32>
__device__ __forceinline__ void wave_fft_inv_tq_two(int lane, cplx (&za)[8], cplx (&zb)[8], cplx *xb, const LaneRoots &ra, const LaneRoots &rb, const W64 &w) {
    wave_sync();
    invs_seg1(lane, za, xb, w);
    wave_sync();
    invs_seg2_ld(lane, za, xb);
    wave_sync();
    invs_seg1(lane, zb, xb, w);
    wave_sync();
    dft8<-1>(za);
    wave_transpose_hi3(za);
    invs_seg2_ld(lane, zb, xb);
    invtq_seg3<TA, DEN>(za, ra);
    dft8<-1>(zb);
    wave_transpose_hi3(zb);
    invtq_seg3<TB, DEN>(zb, rb);
}

#endif

}  // namespace thfhe
#endif
