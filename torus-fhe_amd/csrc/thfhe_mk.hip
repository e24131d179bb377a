// thfhe_mk.hip -- 3-gen multi-key (Torus64 ring) gate bootstrapping on gfx950: kernels + C ABI.
//
// Reference path: mk_gate_*_3gen (J/3gen_mk_gates.jl:8-150) -> mk_bootstrap_3gen (J/3gen_mk_internals.jl:112-116)
//   = mk_bootstrap_wo_keyswitch_3gen (:99-109): P*n sequential CMuxes on ONE Torus64 accumulator, party-major
//     (mk_blind_rotate_3gen :78-84, mk_mux_rotate_3gen :59-62, tgsw_extern_mul_3gen J/tgsw_3gen.jl:102-113),
//     rlwe_extract_sample_64 (J/rlwe.jl:70-74)
//   + mk_keyswitch_3gen (J/mk_internals.jl:730-744): one key switch per party, b = b' + sum of the parts' b.
//
// Kernels:
//   torus_transform_kernel    TransformedBootstrapKeyPart_3gen (J/3gen_mk_internals.jl:45-56): int64 coefficient
//   (thfhe_transform.h)       polynomials -> four balanced 16-bit limbs -> FP64 spectra in streaming order
//   mk_prologue_kernel        gate linear part + mod-switch of the (n, P) mask matrix and of b
//   mk_blind_rotate_coop_kernel / _pair_kernel   one 512-thread workgroup per gate / per two gates: the eight (output polynomial, limb) spectra on
//                             eight waves; _coop2k / _pair2k on the ring of degree 2048 (two twisted half transforms per polynomial);
//                             thfhe_rot2k.h (any number of digit row parts, N = 2048) and thfhe_rot4k.h (N = 4096) for the large-party sets
//   ks_plain_kernel / ks_staged_kernel (thfhe_keyswitch.h)   P key switches of the extracted sample + the cross-party combine of b:
//                             one workgroup per (sample, party, range), or from 192 samples on the rows staged in LDS for 32 samples
//   lut_prologue_kernel (thfhe_lut_prologue.h, shared with thfhe_sk.hip) / mk_lut_acc_init_kernel / mk_extract_at_kernel   programmable bootstrap
//                             (thfhe_mk_lut_bootstrap): weighted sum + mod-switch to multiples of theta, accumulator X^{-barb} * tv in
//                             global memory, the rotation kernels above through acc_in / acc_out, extraction of theta coefficients; with the
//                             prologue reading the wire table they run the LUT nodes of the gate DAG (thfhe_mk_dag_run_lut_batch)
//   mk_extract_mv_kernel      multi-value bootstrap (thfhe_mk_mv_lut_bootstrap): q outputs of ONE rotation, each the integer combination of p
//                             extractions of the Torus64 accumulator staged in LDS (extract_mv64, thfhe_lane.h), converted once; with the prologue on the
//                             wire table the MV nodes of the gate DAG (thfhe_mk_dag_run_mv_batch)
//   mk_pack_rows_kernel / mk_pack_boxes_kernel / mk_lut_acc_init_enc_kernel (thfhe_mk_pack.h)   the multi-key packing key switch, encrypted tables and
//                             the two-digit tree (thfhe_mk_pack_boxes, thfhe_mk_lut_bootstrap_enc, thfhe_mk_tree_lut_bootstrap): records ->
//                             Torus64 RLWE sums under Z = sum_q z_q, box packing of p of them, accumulator start on both polynomials
//   mk_pack_rows_wide_kernel (thfhe_mk_pack.h)   the row sums of large packings, a key row fetched once per 32 records; with
//                             mk_extract_mv_kernel as level 1 the multi-value tree thfhe_mk_tree_lut_bootstrap_mvk: 1 + k rotations for k functions
//   lwe_linear_kernel (thfhe_linear.h, shared with thfhe_sk.hip)   dense layer (thfhe_mk_lwe_linear, thfhe_mk_linear_lut_bootstrap): integer
//                             matrix x vector of P n + 1-word records mod 2^32, the sums staying on the device for the PBS of the same call
//                             ; on the wire-table source the DENSE nodes of the gate DAG (thfhe_mk_dag_run_dense_batch)
//   mk_lhe_cmux2k_kernel / mk_lhe_rotate2k_kernel (thfhe_mk_lhe.h)   leveled CMux and table lookup on TGSW samples the caller brings (thfhe_mk_lhe_cmux,
//                             thfhe_mk_lhe_lookup): the batched N = 2048 step with a key base per job, on d1 - ACC or on public rotation amounts
#include <hip/hip_runtime.h>

#include <type_traits>
#include <memory>
#include <mutex>
#include <new>
#include <vector>

#include "../../include/thfhe_hip.h"
#include "thfhe_common.h"
#include "thfhe_dag.h"
#include "thfhe_lane.h"
#include "thfhe_launch_plan.h"
#include "thfhe_mk_shared.h"
#include "thfhe_mk_pack.h"
#include "thfhe_pbs_host.h"
#include "thfhe_lhe_host.h"   // builds on thfhe_pbs_host.h

using namespace thfhe;

namespace {

#include "thfhe_transform.h"

// torus_transform_kernel on the resident key tables (N = 1024 / 2048): polynomial p = (pi, row r, output o) is part_{mk_part_index(j, o)}[level]
// of row r = j l + level of key pi; its limb spectra go to the chunks of the streaming order (mk_chunk_index)
struct MkResidentMap {
    int l;
    __device__ long src(long p) const {
        const int rows = 2 * l, o = (int)(p & 1), r = (int)((p >> 1) % rows);
        return (((p >> 1) / rows) * 4 + mk_part_index(r / l, o)) * l + r % l;
    }
    __device__ size_t dst(long p, int h, int) const {
        const int rows = 2 * l;
        return mk_chunk_index((p >> 1) / rows, (int)((p >> 1) % rows), h, (int)(p & 1), rows);
    }
};

// wide gadget base: src [poly = (pi, part_q, level)][2048] -> dst [(pi, part_q, level * parts + w)][2048] = src << (pw w)
__global__ __launch_bounds__(256) void mk_expand_parts_kernel(const int64_t *__restrict__ src, int64_t *__restrict__ dst, int l, int parts, int pw) {
    const long poly = blockIdx.x;   // (pi * 4 + q) * l + level
    const int w = blockIdx.y;
    const long head = poly / l, level = poly % l;
    const int64_t *s = src + poly * 2048;
    int64_t *d = dst + ((head * l + level) * parts + w) * 2048;
    for (int t = threadIdx.x; t < 2048; t += 256) d[t] = (int64_t)((uint64_t)s[t] << (pw * w));
}

// ------------------------------------------------------------------------------------------------------
// blind rotate + extract
// ------------------------------------------------------------------------------------------------------
struct MKBRArgs {
    const cplx *bk;
    const cplx *tw;
    const int32_t *bara;  // [jobs][w_pad]
    const int32_t *barb;
    int32_t *out;         // [jobs][N+1]
    long jobs;
    int pn;               // parties * n : number of CMuxes
    int w_pad, Bgbit;
    int64_t mu;
    // party-sharded mode (one rank per party): the accumulator enters from / leaves to global memory instead of being
    // initialised / extracted here.  acc_in == nullptr: start from X^{-barb} * mu; acc_out == nullptr: extract into `out`.
    const int64_t *acc_in = nullptr;
    int64_t *acc_out = nullptr;
    // N = 2048, wide gadget base (the 16+-party sets: l = 1, Bgbit 24 .. 26): every digit is cut into `parts` balanced parts of `pw` bits,
    // d = sum_w d_w 2^(pw w); part w multiplies the key row shifted left by pw w bits (a second / third copy in the key table)
    int parts = 1, pw = 0;
};

// ------------------------------------------------------------------------------------------------------
// blind rotate + extract: one 512-thread workgroup = ONE gate.  The eight (output, limb)
// spectra of a 3-gen external product map onto the eight waves:
//   phase 1  waves 0 .. 2l-1: wave r rotates / decomposes / transforms digit row r and publishes the spectrum in LDS;
//            then every wave requests its key chunks (2l x 8 loads of 16 B per lane, into registers);
//   phase 2  all waves, (o, h) = (wave >> 2, wave & 3): S = sum_r spectrum_r * key(r, h, o); inverse transform;
//            round(S) << 16h is added into accumulator polynomial o with 64-bit LDS atomics (integer adds commute: bit-exact).
// Two workgroup barriers per CMux and no redundant forward transforms.  (An LDS-ring variant in the style of
// sk_blind_rotate_ring_kernel -- 4 gates x 2 output waves per workgroup -- was built and measured 1.3x slower at 1024 gates
// and 3.5x slower for a handful: 9 barriers per digit row, redundant forward transforms; see git history / DESIGN.md 4.3.)
// LDS: T1 8 + acc 16 + spectra 2l x 8 + 8 transpose buffers x 8 KiB (l = 3: 136 KiB).
// ------------------------------------------------------------------------------------------------------
template <int L>
__global__ __launch_bounds__(512, 2) void mk_blind_rotate_coop_kernel(MKBRArgs a) {
    constexpr int ROWS = 2 * L;
    __shared__ cplx sT1[512];
    __shared__ int64_t sAcc[2048];
    __shared__ cplx sSpec[ROWS][512];
    __shared__ cplx sX[8][512];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    sT1[threadIdx.x] = a.tw[threadIdx.x];
    const W64 w64{a.tw[TwRing1k::T2 + 1 * 8 + (lane & 7)]};
    const long job = blockIdx.x;
    const int32_t *bara = a.bara + job * a.w_pad;
    const int Bgbit = a.Bgbit;
    const uint64_t offset = decomp_offset64(L, Bgbit);
    if (a.acc_in) {
        for (int q = threadIdx.x; q < 2048; q += 512) sAcc[q] = a.acc_in[job * 2048 + q];
    } else if (wave == 0) {
        acc_init16_64(lane, sAcc, sAcc + 1024, a.barb[job], a.mu);
    }
    __syncthreads();
    const int o = wave >> 2, h = wave & 3;
    unsigned long long *accu = reinterpret_cast<unsigned long long *>(sAcc) + o * 1024;

    for (int i = 0; i < a.pn; i++) {  // party-major, key index inner: J/3gen_mk_internals.jl:66-84
        const int ai = bara[i];       // uniform over the workgroup
        if (ai == 0) continue;
        const int a2n = ai & 2047;
        if (wave < ROWS) {
            uint32_t t[16];
            cplx z[8];
            load_rotated16_hi(lane, sAcc + (wave / L) * 1024, a2n, offset, t);
            digits_to_z(t, (wave % L) + 1, Bgbit, z);
            wave_fft_fwd_s(opaque_lane(lane), z, sX[wave], sT1, w64);
#pragma unroll
            for (int m = 0; m < 8; m++) sSpec[wave][m * 64 + lane] = z[m];
        }
        // key rows in registers: all 2l of them up to l = 3 (192 VGPRs); from l = 4 on (the 8-party set: 8 rows = 256 VGPRs, which
        // spilled 332 B/lane) a window of PRE rows, refilled as the multiply walks the rows
        constexpr int PRE = ROWS <= 6 ? ROWS : 4;
        cplx B[PRE][8];
#pragma unroll
        for (int r = 0; r < PRE; r++) load8(lane, B[r], a.bk + mk_chunk_index(i, r, h, o, ROWS) * 512);
        __syncthreads();  // spectra published; every rotated read of the accumulator is done
        cplx S[8];
#pragma unroll
        for (int m = 0; m < 8; m++) S[m] = cplx{0.0, 0.0};
#pragma unroll
        for (int r = 0; r < ROWS; r++) {
            cplx z[8];
#pragma unroll
            for (int m = 0; m < 8; m++) z[m] = sSpec[r][m * 64 + lane];
            mac8r(S, z, B[r % PRE]);
            if (r + PRE < ROWS) load8(lane, B[r % PRE], a.bk + mk_chunk_index(i, r + PRE, h, o, ROWS) * 512);
        }
        wave_fft_inv_s(opaque_lane(lane), S, sX[wave], sT1, w64);
#pragma unroll
        for (int m = 0; m < 8; m++) {
            const int q = lane + 64 * m;
            atomicAdd(accu + q, (unsigned long long)round_i64(S[m].re) << (16 * h));
            atomicAdd(accu + q + 512, (unsigned long long)round_i64(S[m].im) << (16 * h));
        }
        __syncthreads();  // accumulator updated before anybody rotates it again
    }
    if (a.acc_out) {
        for (int q = threadIdx.x; q < 2048; q += 512) a.acc_out[job * 2048 + q] = sAcc[q];
    } else if (wave == 0) {
        extract16_64(lane, sAcc, sAcc + 1024, a.out + job * 1025);
    }
}

// ------------------------------------------------------------------------------------------------------
// Throughput kernel: one 512-thread workgroup = TWO gates.  The cooperative kernel above is bound by the key bytes a CU
// has to pull through its vector-memory path (2l x 4 limbs x 2 outputs x 8 KiB = 256 KiB per CMux at l = 2, ~13 k cycles at the
// measured ~20 B/clk/CU, against ~5 k cycles of FP64 work).  Here every (output, limb) wave multiplies its key chunks into the
// spectra of two gates, so each key byte serves two CMuxes; the 2 x 2l forward transforms of a step keep all eight waves busy in
// phase 1 (l = 2: one each), and the transpose scratch aliases the spectrum area (a third barrier frees it for the inverses), which is
// what lets two accumulators and two sets of spectra fit: acc 32 + spectra 2 x 2l x 8 KiB (l = 3: 128 KiB).  Transforms are variant "qs"
// (first transpose in registers, pass-1 twiddles from per-lane roots: no T1 table, one LDS crossing per transform).  The eight pass-1 products
// b s^k are rebuilt in every transform from the two roots, passed through an empty asm (8 VGPRs across the CMux loop): measured on MI355X, MK2 runs
// 39.5 k gates/s when the compiler may hoist all eight out of the loop (32 VGPRs, 88 B/lane scratch), 45.8 k with only the even ones kept
// (20 VGPRs, 48 B) and 52.2 k rebuilt (8 B): with four key rows carried across the loop the registers are worth more than 28 FP64 instructions
// per transform.
// ------------------------------------------------------------------------------------------------------
// mk_pin: memory operations do not move across this point (keeps the paced key requests where they are written)
__device__ __forceinline__ void mk_pin2() { asm volatile("" ::: "memory"); }
// inverse transform of one partial spectrum with the requests for two key rows of the NEXT step between its stages
template <bool PF0, bool PF1>
__device__ __forceinline__ void inv_s_prefetch(int lane, cplx (&S)[8], cplx *xb, const LaneRoots &roots, const W64 &w, cplx (&b0)[8], const cplx *src0, cplx (&b1)[8],
                                               const cplx *src1) {   // wave_fft_inv_qs with the requests in between
    wave_sync();
    invs_seg1(lane, S, xb, w);
    mk_pin2();
    if (PF0) load8(lane, b0, src0);
    mk_pin2();
    wave_sync();
    invs_seg2_ld(lane, S, xb);
    dft8<-1>(S);
    mk_pin2();
    if (PF1) load8(lane, b1, src1);
    mk_pin2();
    wave_transpose_hi3(S);
    invq_seg3(S, LaneRoots{opaque_cplx(roots.b), opaque_cplx(roots.s)});
}
template <int L>
__global__ __launch_bounds__(512, 2) void mk_blind_rotate_pair_kernel(MKBRArgs a) {
    constexpr int ROWS = 2 * L;
    constexpr int FFTS = 2 * ROWS;
    constexpr int SPEC_SLOTS = (FFTS > 8 ? FFTS : 8) * 512;
    constexpr int PRE = ROWS <= 4 ? ROWS : 3;  // key rows in flight (32 VGPRs each); measured at l = 3: 2 rows 19.9 k, 3 rows 20.6 k gates/s (MK4), 4 rows spill 168 B/lane
    __shared__ int64_t sAcc[2][2048];
    __shared__ cplx sSpec[SPEC_SLOTS];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const W64 w64{a.tw[TwRing1k::T2 + 1 * 8 + (lane & 7)]};
    const LaneRoots roots{a.tw[TwRing1k::ROOTS + 2 * lane], a.tw[TwRing1k::ROOTS + 2 * lane + 1]};
    const long job0 = 2 * (long)blockIdx.x;
    const bool has1 = job0 + 1 < a.jobs;
    const int32_t *bara0 = a.bara + job0 * a.w_pad;
    const int32_t *bara1 = bara0 + (has1 ? a.w_pad : 0);
    const int Bgbit = a.Bgbit;
    const uint64_t offset = decomp_offset64(L, Bgbit);
    if (a.acc_in) {   // party-sharded mode: the accumulators of the party block before this one (J/3gen_mk_internals.jl:78-84)
        for (int q = threadIdx.x; q < 4096; q += 512) {
            const int g = q >> 11;
            if (g == 0 || has1) sAcc[g][q & 2047] = a.acc_in[(job0 + g) * 2048 + (q & 2047)];
        }
    } else if (wave < 2 && (wave == 0 || has1)) {
        acc_init16_64(lane, sAcc[wave], sAcc[wave] + 1024, a.barb[job0 + wave], a.mu);
    }
    __syncthreads();
    const int o = wave >> 2, h = wave & 3;

    // The first PRE key rows of a step are requested during the inverse transforms of the step before (the registers that held this
    // step's rows are dead by then), between the stages of the transforms: the 8 PRE loads per wave stream in under ~8 k cycles of
    // compute instead of queueing up in front of the multiply (256 KiB per workgroup and step at l = 2 are ~6 k cycles of the CU's
    // vector-memory path).  Unconditional loads: the last step re-requests its own rows.
    auto active = [&](int i) { return bara0[i] != 0 || (has1 && bara1[i] != 0); };   // uniform over the workgroup
    int i = 0;
    while (i < a.pn && !active(i)) i++;
    cplx B[PRE][8];
    if (i < a.pn) {
#pragma unroll
        for (int r = 0; r < PRE; r++) load8(lane, B[r], a.bk + mk_chunk_index(i, r, h, o, ROWS) * 512);
    }
    while (i < a.pn) {
        const int ai0 = bara0[i], ai1 = has1 ? bara1[i] : 0;
        int inext = i + 1;
        while (inext < a.pn && !active(inext)) inext++;
        const int inl = inext < a.pn ? inext : i;
#pragma unroll
        for (int f0 = 0; f0 < FFTS; f0 += 8) {
            const int f = f0 + wave;  // forward-transform task: gate f / ROWS, digit row f % ROWS
            if (f < FFTS) {
                const int g = f / ROWS, r = f % ROWS;
                const int ai = g ? ai1 : ai0;
                if (ai != 0) {
                    uint32_t t[16];
                    cplx z[8];
                    load_rotated16_hi(lane, sAcc[g] + (r / L) * 1024, ai & 2047, offset, t);
                    digits_to_z(t, (r % L) + 1, Bgbit, z);
                    cplx *slot = sSpec + f * 512;  // transposes run inside the task's own, not yet published, spectrum slot
                    wave_fft_fwd_qs(opaque_lane(lane), z, slot, LaneRoots{opaque_cplx(roots.b), opaque_cplx(roots.s)}, w64);
                    wave_sync();
#pragma unroll
                    for (int m = 0; m < 8; m++) slot[m * 64 + lane] = z[m];
                }
            }
        }
        __syncthreads();  // spectra published; every rotated read of the accumulators is done
        cplx S0[8], S1[8];
#pragma unroll
        for (int m = 0; m < 8; m++) S0[m] = S1[m] = cplx{0.0, 0.0};
#pragma unroll
        for (int r = 0; r < ROWS; r++) {
            cplx z[8];
            if (ai0 != 0) {
#pragma unroll
                for (int m = 0; m < 8; m++) z[m] = sSpec[r * 512 + m * 64 + lane];
                mac8r(S0, z, B[r % PRE]);
            }
            if (ai1 != 0) {
#pragma unroll
                for (int m = 0; m < 8; m++) z[m] = sSpec[(ROWS + r) * 512 + m * 64 + lane];
                mac8r(S1, z, B[r % PRE]);
            }
            mk_pin2();
            if (r + PRE < ROWS) load8(lane, B[r % PRE], a.bk + mk_chunk_index(i, r + PRE, h, o, ROWS) * 512);
            mk_pin2();
        }
        __syncthreads();  // spectra consumed: the area is transpose scratch from here on
        cplx *xb = sSpec + wave * 512;
        const int ln = opaque_lane(lane);
        const cplx *nx[4];
#pragma unroll
        for (int r = 0; r < 4; r++) nx[r] = a.bk + mk_chunk_index(inl, r < PRE ? r : 0, h, o, ROWS) * 512;
        // gate 0's transform carries the requests for rows 0 / 1 of the next step, gate 1's those for rows 2 / 3 (PRE = 4); a skipped gate's
        // requests are issued plainly so that B is complete whichever gates are active
        if (ai0 != 0) {
            unsigned long long *accu = reinterpret_cast<unsigned long long *>(sAcc[0]) + o * 1024;
            inv_s_prefetch<true, (PRE > 1)>(ln, S0, xb, roots, w64, B[0], nx[0], B[PRE > 1 ? 1 : 0], nx[1]);
#pragma unroll
            for (int m = 0; m < 8; m++) {
                const int q = lane + 64 * m;
                atomicAdd(accu + q, (unsigned long long)round_i64(S0[m].re) << (16 * h));
                atomicAdd(accu + q + 512, (unsigned long long)round_i64(S0[m].im) << (16 * h));
            }
        } else {
            load8(lane, B[0], nx[0]);
            if (PRE > 1) load8(lane, B[PRE > 1 ? 1 : 0], nx[1]);
        }
        if (ai1 != 0) {
            unsigned long long *accu = reinterpret_cast<unsigned long long *>(sAcc[1]) + o * 1024;
            inv_s_prefetch<(PRE > 2), (PRE > 3)>(ln, S1, xb, roots, w64, B[PRE > 2 ? 2 : 0], nx[2], B[PRE > 3 ? 3 : 0], nx[3]);
#pragma unroll
            for (int m = 0; m < 8; m++) {
                const int q = lane + 64 * m;
                atomicAdd(accu + q, (unsigned long long)round_i64(S1[m].re) << (16 * h));
                atomicAdd(accu + q + 512, (unsigned long long)round_i64(S1[m].im) << (16 * h));
            }
        } else {
            if (PRE > 2) load8(lane, B[PRE > 2 ? 2 : 0], nx[2]);
            if (PRE > 3) load8(lane, B[PRE > 3 ? 3 : 0], nx[3]);
        }
        __syncthreads();  // accumulators updated and scratch free before the next step
        i = inext;
    }
    if (a.acc_out) {
        for (int q = threadIdx.x; q < 4096; q += 512) {
            const int g = q >> 11;
            if (g == 0 || has1) a.acc_out[(job0 + g) * 2048 + (q & 2047)] = sAcc[g][q & 2047];
        }
    } else if (wave < 2 && (wave == 0 || has1)) {
        extract16_64(lane, sAcc[wave], sAcc[wave] + 1024, a.out + (job0 + wave) * 1025);
    }
}

// ------------------------------------------------------------------------------------------------------
// N = 2048 (BASELINE config 5).  Same wave roles as above; every 1024-point transform is a radix-2 split and two twisted
// 512-point transforms (thfhe_lane.h), so a digit row publishes TWO half spectra (16 KiB) and a phase-2 wave keeps two
// partial spectra S0 / S1.  LDS at l = 3: accumulator 32 + spectra 96 = 128 KiB (table-free "qs" transforms), so the transpose buffers
// alias the spectrum area: in phase 1 a forward unit transposes inside its own (not yet published) half-spectrum slot, in phase 2 a third
// barrier frees the whole area before the eight waves' inverse transform pairs use 8 KiB of it each.
// ------------------------------------------------------------------------------------------------------
THFHE_STAMP_STORAGE
__device__ __forceinline__ void mk_pin() { asm volatile("" ::: "memory"); }  // memory operations do not move across this point
__device__ __forceinline__ void lds_barrier_any() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }   // workgroup barrier ordering LDS traffic only

template <int LE>   // LE = l x parts: digit rows per accumulator polynomial
__global__ __launch_bounds__(512, 2) void mk_blind_rotate_coop2k_kernel(MKBRArgs a) {
    constexpr int ROWS = 2 * LE;
    const int parts = a.parts > 1 ? a.parts : 1, pw = a.pw;
    const int L = LE / parts;   // decomposition levels
    constexpr int SPEC_SLOTS = ROWS * 1024 > 8 * 512 ? ROWS * 1024 : 8 * 512;
    __shared__ int64_t sAcc[4096];
    __shared__ cplx sSpec[SPEC_SLOTS];
    __shared__ cplx sXb[4 * 512];   // transpose scratch of waves 0 - 3 (the last 32 KiB of the LDS)
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    // per-lane transform constants are phase-local (L1 / L2 hits at the start of a transform phase), not 10 VGPRs alive across the multiply
    auto tw_w64 = [&](int ln) { return W64{a.tw[TwRing2k::T2 + 1 * 8 + (ln & 7)]}; };
    auto tw_roots1 = [&](int ln) { return LaneRoots{opaque_cplx(a.tw[TwRing2k::T1_TWIST1 + ln]), opaque_cplx(a.tw[TwRing2k::RATIO + ln])}; };   // b_T = T1_T[0][lane], pass-1 ratio
    auto tw_roots5 = [&](int ln) { return LaneRoots{opaque_cplx(a.tw[TwRing2k::T1_TWIST5 + ln]), opaque_cplx(a.tw[TwRing2k::RATIO + ln])}; };
    const long job = blockIdx.x;
    const int32_t *bara = a.bara + job * a.w_pad;
    const int Bgbit = a.Bgbit;
    const uint64_t offset = decomp_offset64(L, Bgbit);
    if (a.acc_in) {
        for (int q = threadIdx.x; q < 4096; q += 512) sAcc[q] = a.acc_in[job * 4096 + q];
    } else if (wave == 0) {
        acc_init_64_n<2048>(lane, sAcc, sAcc + 2048, a.barb[job], a.mu);
    }
    __syncthreads();
    const int o = wave >> 2, h = wave & 3;
    unsigned long long *accu = reinterpret_cast<unsigned long long *>(sAcc) + o * 2048;

    // The key stream of a step is 2l rows x 2 half spectra = 4l chunks of 8 KiB per wave (l = 3: 96 KiB per wave, 768 KiB per workgroup
    // and CMux -- the CU's vector-memory path carries ~45 B/clk, so it is busy for a good part of every step).  The chunks are
    // requested two ahead of their use (registers bA / bB), and the first two chunks of the NEXT step are requested before this
    // step's inverse transforms, so the memory pipeline never waits for the compute phases and the multiply never waits for a
    // round trip of its own.  Compiler fences (mk_pin) keep the requests where they are written.
    // The step loop exists twice, for waves 0 - 3 (EARLY) and 4 - 7: the same phases with the "spectra consumed" barrier behind / in front of
    // the inverse transforms.  One loop with the barrier under a wave test made the register allocator spill 200 - 2 500 B per lane.
    auto steps = [&](auto early_tag) {
    constexpr bool EARLY = decltype(early_tag)::value;
    int i = 0;
    while (i < a.pn && bara[i] == 0) i++;
    cplx bA[8], bB[8];
    auto chunk = [&](int step, int u) { return a.bk + mk_chunk_index_2k(step, u >> 1, h, o, ROWS) * 512 + (u & 1) * 512; };  // u = 2 r + half
    if (i < a.pn) {
        load8(lane, bA, chunk(i, 0));
        load8(lane, bB, chunk(i, 1));
    }
    STAMP_DECL;
    while (i < a.pn) {
        const int a2n = bara[i] & 4095;
        int inext = i + 1;
        while (inext < a.pn && bara[inext] == 0) inext++;
        const int inl = inext < a.pn ? inext : i;   // the last step re-requests its own chunks (unconditional loads: one register set)
        // forward units (digit row, half): 2 ROWS of them on eight waves.  ROWS = 6: waves 0 - 3 take both halves of rows 0 - 3 (two transforms side
        // by side), waves 4 - 7 one half of rows 4 / 5 each -- three units per SIMD (wave w and w + 4 share one); ROWS < 6: one unit per wave
        const bool two = ROWS == 6 && wave < 4;
        const int row = ROWS == 6 ? (wave < 4 ? wave : 4 + ((wave - 4) >> 1)) : (wave >> 1);
        const int half_of = wave & 1;
        if (ROWS == 6 || wave < 2 * ROWS) {
            cplx y0[8], y1[8];   // a one-unit wave forms its half in y0
            {
                // digits of the four coefficients (j, j + 512, j + 1024, j + 1536) that make one (y0[m], y1[m]) pair: no 32-word t[],
                // no 16-point z[] alive next to the two half transforms
                const int64_t *ap = sAcc + (row / LE) * 2048;
                const int level = (row % LE) / parts, part = (row % LE) % parts;   // uniform per wave
                const int shift = 32 - (level + 1) * Bgbit;
                const uint32_t mask = (1u << Bgbit) - 1u;
                const int32_t half = 1 << (Bgbit - 1);
                const int32_t hp = pw ? 1 << (pw - 1) : 0, mp = (1 << pw) - 1;
                constexpr double R = 0.70710678118654752440;
                const double sg = half_of ? -1.0 : 1.0;
                // all 32 rotated words first (their LDS reads in flight together), then the branch-free digit arithmetic: with the loop over the
                // parts inside the unrolled body every rotated read was waited for on its own (s_waitcnt lgkmcnt(0) + a uniform branch per coefficient)
#pragma unroll
                for (int m0 = 0; m0 < 8; m0 += 4) {   // in two halves: 16 words alive next to the points already formed (all 32 spilled 56 B per lane)
                uint32_t t[4][4];
#pragma unroll
                for (int m = 0; m < 4; m++)
#pragma unroll
                    for (int q = 0; q < 4; q++) t[m][q] = (uint32_t)((rot_minus_self64_n<2048>(ap, lane + 64 * (m0 + m) + 512 * q, a2n) + offset) >> 32);
                asm volatile("" ::: "memory");
#pragma unroll
                for (int mm = 0; mm < 4; mm++) {
                    const int m = m0 + mm;
                    double d[4];
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        int32_t dg = (int32_t)((t[mm][q] >> shift) & mask) - half;      // decompose, J/tgsw.jl:112-138
                        if (parts > 1) {   // balanced parts, least significant first; at most three (l x parts <= 3); uniform selects, no branches
                            const int32_t lo0 = ((dg + hp) & mp) - hp, v1 = (dg - lo0) >> pw;
                            const int32_t lo1 = ((v1 + hp) & mp) - hp, v2 = (v1 - lo1) >> pw;
                            const int32_t p1 = parts > 2 ? lo1 : v1;
                            dg = part == 0 ? lo0 : (part == 1 ? p1 : v2);
                        }
                        d[q] = (double)dg;
                    }
                    // z[m] = (d0, d2) (coefficients j, j + 1024), z[m + 8] = (d1, d3); split2048: y0/1 = z[m] +- e^{i pi/4} z[m + 8]
                    const cplx w{(d[1] - d[3]) * R, (d[1] + d[3]) * R};
                    if (two) {
                        y0[m] = cplx{d[0] + w.re, d[2] + w.im};
                        y1[m] = cplx{d[0] - w.re, d[2] - w.im};
                    } else {
                        y0[m] = cplx{d[0] + sg * w.re, d[2] + sg * w.im};   // one rounding, like the sum / difference it stands for
                    }
                }
                }
            }
            cplx *xb = sSpec + row * 1024;
            const int ln = opaque_lane(lane);   // the swizzled LDS slot maps are recomputed here, not hoisted out of the CMux loop and spilled
            const W64 w64 = tw_w64(ln);
            if (two) {
                wave_fft_fwd_tq_two<1, 5>(ln, y0, y1, xb, xb + 512, tw_roots1(ln), tw_roots5(ln), w64);
                wave_sync();
#pragma unroll
                for (int m = 0; m < 8; m++) {
                    xb[m * 64 + ln] = y0[m];
                    xb[512 + m * 64 + ln] = y1[m];
                }
            } else {
                cplx *slot = xb + half_of * 512;
                if (half_of == 0) wave_fft_fwd_tq<1>(ln, y0, slot, tw_roots1(ln), w64);
                else wave_fft_fwd_tq<5>(ln, y0, slot, tw_roots5(ln), w64);
                wave_sync();
#pragma unroll
                for (int m = 0; m < 8; m++) slot[m * 64 + ln] = y0[m];
            }
        }
        STAMP(0);
        __syncthreads();  // spectra published; every rotated read of the accumulator is done
        STAMP(1);
        cplx S0[8], S1[8];
#pragma unroll
        for (int m = 0; m < 8; m++) S0[m] = S1[m] = cplx{0.0, 0.0};
#pragma unroll
        for (int u = 0; u < 2 * ROWS; u += 2) {
            cplx z[8];
#pragma unroll
            for (int m = 0; m < 8; m++) z[m] = sSpec[(u >> 1) * 1024 + m * 64 + lane];
            mac8r(S0, z, bA);
            mk_pin();
            load8(lane, bA, u + 2 < 2 * ROWS ? chunk(i, u + 2) : chunk(inl, 0));
            mk_pin();
#pragma unroll
            for (int m = 0; m < 8; m++) z[m] = sSpec[(u >> 1) * 1024 + 512 + m * 64 + lane];
            mac8r(S1, z, bB);
            mk_pin();
            load8(lane, bB, u + 2 < 2 * ROWS ? chunk(i, u + 3) : chunk(inl, 1));
            mk_pin();
        }
        STAMP(2);
        auto finish = [&](cplx *xb) {   // inverse transform pair, radix-2 merge, round(S) << 16h into accumulator polynomial o
            const int ln = opaque_lane(lane);
            wave_fft_inv_tq_two<1, 5>(ln, S0, S1, xb, tw_roots1(ln), tw_roots5(ln), tw_w64(ln));
            cplx lo[8], hi[8];
            merge2048(S0, S1, lo, hi);
#pragma unroll
            for (int m = 0; m < 8; m++) {
                const int q = lane + 64 * m;
                atomicAdd(accu + q, (unsigned long long)round_i64(lo[m].re) << (16 * h));
                atomicAdd(accu + q + 512, (unsigned long long)round_i64(hi[m].re) << (16 * h));
                atomicAdd(accu + q + 1024, (unsigned long long)round_i64(lo[m].im) << (16 * h));
                atomicAdd(accu + q + 1536, (unsigned long long)round_i64(hi[m].im) << (16 * h));
            }
        };
        // The older wave of every SIMD (0 - 3) is served first by the key stream and leaves the multiply ~6 k cycles before its partner.  It owns
        // 8 KiB of transpose scratch outside the spectrum area, so it does not wait for the others to finish reading the spectra: it
        // transforms at once and ARRIVES at that barrier afterwards, about when the younger waves get there from their multiply; those then
        // transform with a SIMD to themselves.  (The accumulator atomics touch nothing the multiply reads.)
        if (EARLY) {
            STAMP(4);
            finish(sXb + wave * 512);
            STAMP(3);
            __syncthreads();  // spectra consumed (reached after the transforms)
        } else {
            __syncthreads();  // spectra consumed: the area is transpose scratch from here on
            STAMP(4);
            finish(sSpec + wave * 512);
            STAMP(3);
        }
        __syncthreads();  // accumulator updated and scratch free before the next rotation
        STAMP(5);
        i = inext;
    }
    STAMP_FLUSH(blockIdx.x, wave);
    };
    if (wave < 4) steps(std::true_type{});
    else steps(std::false_type{});
    if (a.acc_out) {
        for (int q = threadIdx.x; q < 4096; q += 512) a.acc_out[job * 4096 + q] = sAcc[q];
    } else if (wave == 0) {
        extract_64_n<2048>(lane, sAcc, sAcc + 2048, a.out + job * 2049);
    }
}

// the batched N = 2048 rotation (any number of row parts, two-part digits) shared with the KMS scheme
#include "thfhe_rot2k.h"
// the ring of degree 4096 (the 64-party "for fft" and the 512-party 3-gen sets)
#include "thfhe_rot4k.h"

// ------------------------------------------------------------------------------------------------------
// N = 2048 throughput kernel: one 512-thread workgroup = TWO gates (batches above one gate per CU).  The one-gate kernel above spends half
// of every step pulling 768 KiB of key spectra (l = 3) through the CU's vector-memory path; here every key chunk multiplies the digit
// spectra of two gates.  Two accumulators (64 KiB) leave 96 KiB for spectra -- the 2 x 2l HALF spectra of one twist -- so a step runs as
// two half passes: forward transforms of the even-output halves (twist 1) of all rows of both gates, multiply into S0, the same for the
// odd-output halves (twist 5, digits extracted again: the accumulators do not change inside a step) into S1, then the four inverse
// transforms, the radix-2 merge and the integer atomics.  Transforms are the "qs" form of the twisted halves (no T1 tables in LDS, one
// LDS crossing); the barriers wait for the LDS only (vmcnt(16)), so the two key chunks a wave has requested stay in flight across them:
// the key stream never stops at a phase boundary.  LDS at l = 3: 64 + 96 = 160 KiB.
// ------------------------------------------------------------------------------------------------------
struct P2KDigits {
    int parts, pw, L, Bgbit;
    uint64_t offset;
};
// Digits of a step, computed ONCE for both half passes and all levels:
//   stage   every wave takes half of one (gate, accumulator polynomial): t = top 32 bits of (X^a acc - acc) + offset for 16 coefficients per
//           lane -> 8 KiB of 32-bit words per (gate, polynomial) in the spectrum area (slots 0..3, free at this point);
//   pack    task f = (gate f / ROWS, digit row f % ROWS) reads the 32 words of the coefficients its lane transforms, cuts out its digit
//           (level, part) and keeps the four digits of a radix-2 group as 16-bit fields of two registers: 16 VGPRs per task carry the
//           digits through both half passes (the rotated 64-bit reads + offset + decomposition cost more than a half transform).
__device__ __forceinline__ void p2k_stage(int wave, int lane, const int64_t (*sAcc)[4096], uint32_t *stage, int ai0, int ai1, uint64_t offset) {
    const int gj = wave >> 1, g = gj >> 1, j = gj & 1;
    const int ai = g ? ai1 : ai0;
    if (ai == 0) return;
    const int a2n = ai & 4095;
    const int64_t *ap = sAcc[g] + j * 2048;
    uint32_t *dst = stage + gj * 2048;
#pragma unroll
    for (int k = 0; k < 16; k++) {
        const int c = (wave & 1) * 1024 + lane + 64 * k;
        dst[c] = (uint32_t)((rot_minus_self64_n<2048>(ap, c, a2n) + offset) >> 32);
    }
}
// ONE_PART: the gadget digit is used whole (parts = 1: every set with Bgbit <= 10, e.g. BASELINE configs[4]) -- the per-coefficient part loops and
// their 32 uniform branches per task are compiled out; the general form serves the wide-base sets (two / three balanced parts).
template <int LE, bool ONE_PART>
__device__ __forceinline__ void p2k_pack(int f, int lane, const uint32_t *stage, const P2KDigits &dg, uint32_t (&pk)[8][2]) {
    constexpr int ROWS = 2 * LE;
    const int g = f / ROWS, r = f % ROWS;
    const uint32_t *src = stage + (g * 2 + r / LE) * 2048;
    const int level = ONE_PART ? (r % LE) : (r % LE) / dg.parts, part = ONE_PART ? 0 : (r % LE) % dg.parts;   // uniform per wave
    const int shift = 32 - (level + 1) * dg.Bgbit;
    const uint32_t mask = (1u << dg.Bgbit) - 1u;
    const int32_t half = 1 << (dg.Bgbit - 1);
    const int pw = dg.pw;
    const int32_t hp = pw ? 1 << (pw - 1) : 0, mp = (1 << pw) - 1;
    // all 32 staged words first (independent LDS reads in flight together), then the digit arithmetic -- branch-free: with a loop over the parts
    // inside the unrolled body every read was followed by s_waitcnt lgkmcnt(0) and a uniform branch (64 exposed LDS round trips per step)
    uint32_t t[8][4];
#pragma unroll
    for (int m = 0; m < 8; m++)
#pragma unroll
        for (int q = 0; q < 4; q++) t[m][q] = src[lane + 64 * m + 512 * q];
#pragma unroll
    for (int m = 0; m < 8; m++) {
        int32_t d[4];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            int32_t v = (int32_t)((t[m][q] >> shift) & mask) - half;      // decompose, J/tgsw.jl:112-138
            if (!ONE_PART) {   // balanced parts, least significant first; at most three (l x parts <= 3)
                const int32_t lo0 = ((v + hp) & mp) - hp, v1 = (v - lo0) >> pw;
                const int32_t lo1 = ((v1 + hp) & mp) - hp, v2 = (v1 - lo1) >> pw;
                const int32_t p0 = dg.parts > 1 ? lo0 : v, p1 = dg.parts > 2 ? lo1 : v1;
                v = part == 0 ? p0 : (part == 1 ? p1 : v2);
            }
            d[q] = v;
        }
        pk[m][0] = ((uint32_t)d[0] & 0xffffu) | ((uint32_t)d[1] << 16);
        pk[m][1] = ((uint32_t)d[2] & 0xffffu) | ((uint32_t)d[3] << 16);
    }
}
template <int LE>
__global__ __launch_bounds__(512, 2) void mk_blind_rotate_pair2k_kernel(MKBRArgs a) {
    constexpr int ROWS = 2 * LE;
    constexpr int TASKS = 2 * ROWS;
    constexpr int SLOTS = TASKS > 8 ? TASKS : 8;
    constexpr int PRE = 2;   // key chunks in flight per wave (32 VGPRs each); S0 / S1 of both gates hold 128
    __shared__ int64_t sAcc[2][4096];
    __shared__ cplx sSpec[SLOTS * 512];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    // per-lane transform constants are phase-local: fetched again (L1 / L2 hits) at the start of every transform phase instead of living in
    // 16 VGPRs across the multiply phases, where the four partial spectra, two key chunks and a digit spectrum leave no room (the allocator
    // spilled them to scratch and reloaded them in front of every use)
    auto tw_w64 = [&](int ln) { return W64{a.tw[TwRing2k::T2 + 1 * 8 + (ln & 7)]}; };
    auto tw_roots1 = [&](int ln) { return LaneRoots{a.tw[TwRing2k::T1_TWIST1 + ln], a.tw[TwRing2k::RATIO + ln]}; };         // b_T = T1_T[0][lane], ratio
    auto tw_roots5 = [&](int ln) { return LaneRoots{a.tw[TwRing2k::T1_TWIST5 + ln], a.tw[TwRing2k::RATIO + ln]}; };
    P2KDigits dg;
    dg.parts = a.parts > 1 ? a.parts : 1;
    dg.pw = a.pw;
    dg.L = LE / dg.parts;
    dg.Bgbit = a.Bgbit;
    dg.offset = decomp_offset64(dg.L, a.Bgbit);
    const long job0 = 2 * (long)blockIdx.x;
    const bool has1 = job0 + 1 < a.jobs;
    const int32_t *bara0 = a.bara + job0 * a.w_pad;
    const int32_t *bara1 = bara0 + (has1 ? a.w_pad : 0);
    if (a.acc_in) {
        for (int q = threadIdx.x; q < 8192; q += 512) {
            const int g = q >> 12;
            if (g == 0 || has1) sAcc[g][q & 4095] = a.acc_in[(job0 + g) * 4096 + (q & 4095)];
        }
    } else if (wave < 2 && (wave == 0 || has1)) {
        acc_init_64_n<2048>(lane, sAcc[wave], sAcc[wave] + 2048, a.barb[job0 + wave], a.mu);
    }
    __syncthreads();
    const int o = wave >> 2, h = wave & 3;
    auto chunk = [&](int step, int r, int half) { return a.bk + mk_chunk_index_2k(step, r, h, o, ROWS) * 512 + half * 512; };
    auto active = [&](int i) { return bara0[i] != 0 || (has1 && bara1[i] != 0); };   // uniform over the workgroup
    int i = 0;
    while (i < a.pn && !active(i)) i++;
    STAMP_DECL;
    while (i < a.pn) {
        const int ai0 = bara0[i], ai1 = has1 ? bara1[i] : 0;
        int inext = i + 1;
        while (inext < a.pn && !active(inext)) inext++;
        // ---- digits of the step
        const bool t0 = wave < TASKS && ((wave / ROWS) ? ai1 : ai0) != 0;                  // this wave's first / second forward task is live
        const bool t1 = wave + 8 < TASKS && (((wave + 8) / ROWS) ? ai1 : ai0) != 0;
        uint32_t pk0[8][2], pk1[8][2];
        p2k_stage(wave, lane, sAcc, reinterpret_cast<uint32_t *>(sSpec), ai0, ai1, dg.offset);
        lds_barrier<8 * PRE>();
        if (dg.parts == 1) {   // uniform over the launch
            if (t0) p2k_pack<LE, true>(wave, lane, reinterpret_cast<const uint32_t *>(sSpec), dg, pk0);
            if (t1) p2k_pack<LE, true>(wave + 8, lane, reinterpret_cast<const uint32_t *>(sSpec), dg, pk1);
        } else {
            if (t0) p2k_pack<LE, false>(wave, lane, reinterpret_cast<const uint32_t *>(sSpec), dg, pk0);
            if (t1) p2k_pack<LE, false>(wave + 8, lane, reinterpret_cast<const uint32_t *>(sSpec), dg, pk1);
        }
        lds_barrier<8 * PRE>();   // staged words consumed: the slots are free for the spectra
        // ---- half pass 0: even outputs (twist 1); its first key chunks are requested ahead of the transforms (no partial spectra alive yet)
        cplx B[PRE][8];
        mk_pin();
#pragma unroll
        for (int r = 0; r < PRE; r++) load8(lane, B[r], chunk(i, r, 0));
        mk_pin();
        if (t0 || t1) {
            const int ln = opaque_lane(lane);
            const W64 w64 = tw_w64(ln);
            const LaneRoots roots1 = tw_roots1(ln);
            if (t0 && t1) {
                r2k_transform_two<0>(wave, wave + 8, lane, sSpec, pk0, pk1, roots1, w64);
            } else {
                if (t0) r2k_transform<0>(wave, lane, sSpec, pk0, roots1, w64);
                if (t1) r2k_transform<0>(wave + 8, lane, sSpec, pk1, roots1, w64);
            }
        }
        STAMP(0);
        lds_barrier<8 * PRE>();   // spectra published
        STAMP(1);
        cplx S0a[8], S0b[8];
#pragma unroll
        for (int m = 0; m < 8; m++) S0a[m] = S0b[m] = cplx{0.0, 0.0};
#pragma unroll
        for (int r = 0; r < ROWS; r++) {
            cplx z[8];
            if (ai0 != 0) {
#pragma unroll
                for (int m = 0; m < 8; m++) z[m] = sSpec[r * 512 + m * 64 + lane];
                mac8r(S0a, z, B[r % PRE]);
            }
            if (ai1 != 0) {
#pragma unroll
                for (int m = 0; m < 8; m++) z[m] = sSpec[(ROWS + r) * 512 + m * 64 + lane];
                mac8r(S0b, z, B[r % PRE]);
            }
            mk_pin();
            if (r + PRE < ROWS) load8(lane, B[r % PRE], chunk(i, r + PRE, 0));
            mk_pin();
        }
        STAMP(2);
        lds_barrier<8 * PRE>();   // spectra consumed
        STAMP(4);
        // ---- half pass 1: odd outputs (twist 5), same digits
        if (t0 || t1) {
            const int ln = opaque_lane(lane);
            const W64 w64 = tw_w64(ln);
            const LaneRoots roots5 = tw_roots5(ln);
            if (t0 && t1) {
                r2k_transform_two<1>(wave, wave + 8, lane, sSpec, pk0, pk1, roots5, w64);
            } else {
                if (t0) r2k_transform<1>(wave, lane, sSpec, pk0, roots5, w64);
                if (t1) r2k_transform<1>(wave + 8, lane, sSpec, pk1, roots5, w64);
            }
        }
        mk_pin();
#pragma unroll
        for (int r = 0; r < PRE; r++) load8(lane, B[r], chunk(i, r, 1));
        mk_pin();
        STAMP(0);
        lds_barrier<8 * PRE>();
        STAMP(1);
        cplx S1a[8], S1b[8];
#pragma unroll
        for (int m = 0; m < 8; m++) S1a[m] = S1b[m] = cplx{0.0, 0.0};
#pragma unroll
        for (int r = 0; r < ROWS; r++) {
            cplx z[8];
            if (ai0 != 0) {
#pragma unroll
                for (int m = 0; m < 8; m++) z[m] = sSpec[r * 512 + m * 64 + lane];
                mac8r(S1a, z, B[r % PRE]);
            }
            if (ai1 != 0) {
#pragma unroll
                for (int m = 0; m < 8; m++) z[m] = sSpec[(ROWS + r) * 512 + m * 64 + lane];
                mac8r(S1b, z, B[r % PRE]);
            }
            mk_pin();
            if (r + PRE < ROWS) load8(lane, B[r % PRE], chunk(i, r + PRE, 1));
            mk_pin();
        }
        STAMP(2);
        lds_barrier<8 * PRE>();   // spectra consumed: the area is transpose scratch from here on; every rotated read of the accumulators is done
        STAMP(4);
        // ---- inverse transforms, merge, accumulate
        {
            cplx *xb = sSpec + wave * 512;
            const int ln = opaque_lane(lane);
            const W64 w64 = tw_w64(ln);
            const LaneRoots roots1 = tw_roots1(ln), roots5 = tw_roots5(ln);
            const bool both = ai0 != 0 && ai1 != 0;   // all but one step in 4096: both jobs' transforms of a twist run side by side
            if (both) {
                {
                    const LaneRoots r{opaque_cplx(roots1.b), opaque_cplx(roots1.s)};
                    wave_fft_inv_tq_two<1, 1>(ln, S0a, S0b, xb, r, r, w64);
                }
                {
                    const LaneRoots r{opaque_cplx(roots5.b), opaque_cplx(roots5.s)};
                    wave_fft_inv_tq_two<5, 5>(ln, S1a, S1b, xb, r, r, w64);
                }
            }
            if (ai0 != 0) {
                unsigned long long *accu = reinterpret_cast<unsigned long long *>(sAcc[0]) + o * 2048;
                if (!both) {
                    wave_fft_inv_tq<1>(ln, S0a, xb, LaneRoots{opaque_cplx(roots1.b), opaque_cplx(roots1.s)}, w64);
                    wave_fft_inv_tq<5>(ln, S1a, xb, LaneRoots{opaque_cplx(roots5.b), opaque_cplx(roots5.s)}, w64);
                }
                cplx lo[8], hi[8];
                merge2048(S0a, S1a, lo, hi);
#pragma unroll
                for (int m = 0; m < 8; m++) {
                    const int q = lane + 64 * m;
                    atomicAdd(accu + q, (unsigned long long)round_i64(lo[m].re) << (16 * h));
                    atomicAdd(accu + q + 512, (unsigned long long)round_i64(hi[m].re) << (16 * h));
                    atomicAdd(accu + q + 1024, (unsigned long long)round_i64(lo[m].im) << (16 * h));
                    atomicAdd(accu + q + 1536, (unsigned long long)round_i64(hi[m].im) << (16 * h));
                }
            }
            if (ai1 != 0) {
                unsigned long long *accu = reinterpret_cast<unsigned long long *>(sAcc[1]) + o * 2048;
                if (!both) {
                    wave_fft_inv_tq<1>(ln, S0b, xb, LaneRoots{opaque_cplx(roots1.b), opaque_cplx(roots1.s)}, w64);
                    wave_fft_inv_tq<5>(ln, S1b, xb, LaneRoots{opaque_cplx(roots5.b), opaque_cplx(roots5.s)}, w64);
                }
                cplx lo[8], hi[8];
                merge2048(S0b, S1b, lo, hi);
#pragma unroll
                for (int m = 0; m < 8; m++) {
                    const int q = lane + 64 * m;
                    atomicAdd(accu + q, (unsigned long long)round_i64(lo[m].re) << (16 * h));
                    atomicAdd(accu + q + 512, (unsigned long long)round_i64(hi[m].re) << (16 * h));
                    atomicAdd(accu + q + 1024, (unsigned long long)round_i64(lo[m].im) << (16 * h));
                    atomicAdd(accu + q + 1536, (unsigned long long)round_i64(hi[m].im) << (16 * h));
                }
            }
        }
        STAMP(3);
        lds_barrier<8 * PRE>();   // accumulators updated and scratch free before the next step
        STAMP(5);
        i = inext;
    }
    STAMP_FLUSH(blockIdx.x, wave);
    __syncthreads();
    if (a.acc_out) {
        for (int q = threadIdx.x; q < 8192; q += 512) {
            const int g = q >> 12;
            if (g == 0 || has1) a.acc_out[(job0 + g) * 4096 + (q & 4095)] = sAcc[g][q & 4095];
        }
    } else if (wave < 2 && (wave == 0 || has1)) {
        extract_64_n<2048>(lane, sAcc[wave], sAcc[wave] + 2048, a.out + (job0 + wave) * 2049);
    }
}


// initial accumulator of the batched path, in global memory: acc = (0, X^{-barb} * (mu, ..., mu))   (J/3gen_mk_internals.jl:91-92)
__global__ __launch_bounds__(256) void mk_acc_init_2k_kernel(const int32_t *__restrict__ barb, int64_t mu, long jobs, int64_t *__restrict__ acc, int N = 2048) {
    const long job = blockIdx.x;
    if (job >= jobs) return;
    const int b = barb[job];
    for (int q = threadIdx.x; q < N; q += 256) {
        acc[job * 2 * N + q] = 0;
        acc[job * 2 * N + N + q] = (((q + b) & (2 * N - 1)) & N) ? (int64_t)(0ull - (uint64_t)mu) : mu;
    }
}

// ------------------------------------------------------------------------------------------------------
// programmable bootstrap (thfhe_mk_lut_bootstrap): only the two ends of the rotation are new; the rotation kernels take the
// accumulator from global memory and return it there (MKBRArgs::acc_in / acc_out).
// ------------------------------------------------------------------------------------------------------
// prologue: lut_prologue_kernel (thfhe_lut_prologue.h) over the P n + 1 record words.
// accumulator start acc[job] = (0, X^{-barb} * tv[lut_idx[job]]) over Torus64 (oracle_mul_by_monomial64): coefficient q is tv[(q + barb) mod N],
// negated when (q + barb) mod 2N >= N.  mk_acc_init_2k_kernel with a per-sample table instead of a constant; N = 1024, 2048 or 4096.
__global__ __launch_bounds__(256) void mk_lut_acc_init_kernel(const int32_t *__restrict__ barb, const int64_t *__restrict__ tv,
                                                               const int32_t *__restrict__ lut_idx, long jobs, int N, int64_t *__restrict__ acc) {
    const long job = blockIdx.x;
    if (job >= jobs) return;
    const int b = barb[job];
    const int64_t *t = tv + (lut_idx ? (size_t)lut_idx[job] * N : 0);
    int64_t *ap = acc + job * 2 * N;
    for (int q = threadIdx.x; q < N; q += 256) {
        const int e = (q + b) & (2 * N - 1);
        const int64_t v = t[e & (N - 1)];
        ap[q] = 0;
        ap[N + q] = (e & N) ? (int64_t)(0ull - (uint64_t)v) : v;
    }
}

// extraction of coefficients j = blockIdx.y < theta: record (job theta + j) of N + 1 words, a'_i = t64tot32(a_{j-i}) for i <= j,
// t64tot32(-a_{N+j-i}) for i > j (negated mod 2^64 before the conversion), b' = t64tot32(body_j).  j = 0 is mk_extract_kernel.
__global__ __launch_bounds__(256) void mk_extract_at_kernel(const int64_t *__restrict__ acc, int32_t *__restrict__ out, long jobs, int N, int theta) {
    const long job = blockIdx.x;
    const int j = blockIdx.y;
    if (job >= jobs || j >= theta) return;
    const int64_t *ap = acc + job * 2 * N;
    int32_t *o = out + (job * theta + j) * (N + 1);
    for (int q = threadIdx.x; q <= N; q += 256) {
        int64_t v;
        if (q == N) v = ap[N + j];
        else {
            v = ap[(j - q) & (N - 1)];
            if (q > j) v = (int64_t)(0ull - (uint64_t)v);
        }
        o[q] = t64tot32(v);
    }
}

// multi-value epilogue (thfhe_mk_mv_lut_bootstrap): the q outputs of job blockIdx.x from its accumulator in global memory, record
// (job q + j) of NN + 1 words = extract_mv64 with the taps w[table][j][0 .. p), table = tab_idx[job] (null: table 0).  The mask polynomial is staged
// once in LDS (8 / 16 / 32 KiB) with the p body words the taps meet; the q outputs then read LDS only.  Taps and table index are wave-uniform loads.
struct MkMvArgs {
    const int32_t *w;   // [n_tables][q][p] taps
    int p, q;
    int64_t out_bias;   // added to the body word of every output before its conversion
};
template <int NN>
__global__ __launch_bounds__(256) void mk_extract_mv_kernel(const int64_t *__restrict__ acc, MkMvArgs mv, const int32_t *__restrict__ tab_idx, long jobs,
                                                            int32_t *__restrict__ out) {
    __shared__ int64_t sMask[NN];
    __shared__ int64_t sBody[64];
    const long job = blockIdx.x;
    if (job >= jobs) return;
    const int64_t *ap = acc + job * 2 * NN;
    for (int q = threadIdx.x; q < NN; q += 256) sMask[q] = ap[q];
    const int box = NN / mv.p;
    if ((int)threadIdx.x < mv.p) sBody[threadIdx.x] = ap[NN + NN - (box >> 1) - (int)threadIdx.x * box];
    __syncthreads();
    const uniform_i32_ptr w = as_uniform(mv.w) + (size_t)(tab_idx ? as_uniform(tab_idx)[job] : 0) * mv.q * mv.p;
    for (int j = 0; j < mv.q; j++) extract_mv64<NN>((int)threadIdx.x, sMask, sBody, w + j * mv.p, mv.p, mv.out_bias, out + (job * mv.q + j) * (NN + 1));
}

__global__ __launch_bounds__(256) void mk_linear_kernel(const int32_t *__restrict__ x, const int32_t *__restrict__ y, int32_t *__restrict__ out,
                                                         size_t words, size_t rec, int mode) {
    // mode 0: copy, 1: negate, 2: (0, 1/8) + x + y   (the 3-gen MUX epilogue, J/3gen_mk_gates.jl:144-147)
    const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= words) return;
    uint32_t v = (uint32_t)x[q];
    if (mode == 1) v = 0u - v;
    if (mode == 2) {
        v += (uint32_t)y[q];
        if (q % rec == rec - 1) v += 1u << 29;
    }
    out[q] = (int32_t)v;
}

__global__ __launch_bounds__(256) void mk_mux_combine_kernel(const int32_t *__restrict__ t, int32_t *__restrict__ out, size_t words, size_t rec) {
    const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= words) return;
    const size_t g = q / rec, w = q % rec;
    uint32_t v = (uint32_t)t[(2 * g) * rec + w] + (uint32_t)t[(2 * g + 1) * rec + w];
    if (w == rec - 1) v += 1u << 29;
    out[q] = (int32_t)v;
}

}  // namespace

struct thfhe_mk_ctx;
// Device-resident TGSW samples of thfhe_mk_tgsw_set_create: the spectra of count x d address bits in the layout of the batched
// path's key table, (sample d + bit) in the place of the key index.  Belongs to the context that made it and is destroyed before it.  Whoever
// fills `spec` -- the upload of thfhe_mk_lhe.h today, a device-side producer later -- writes that layout in place.
struct THFHE_INTERNAL thfhe_mk_tgsw_set {
    thfhe_mk_ctx *ctx = nullptr;
    DevBuf spec;
    size_t count = 0;
    int d = 0;
};

struct THFHE_INTERNAL thfhe_mk_ctx : DevCtx {
    thfhe_params p;
    DevBuf d_bk;
    KsKey ksk;
    int w_pad = 0, words = 0, log2_2n = 11;   // words: the mask words P n of a record
    int rec_words() const { return words + 1; }
    DevBuf park;                 // batched N = 2048 rotation, two jobs per workgroup: partial spectra between row-part batches (thfhe_rot2k.h)
    long pair_threshold = 256;  // batches of more rotations than this run two gates per workgroup (mk_blind_rotate_pair_kernel)
    bool batched = false;       // N = 2048 with l x digit parts > 3: thfhe_rot2k.h (row parts through the LDS in batches), key table in its layout
    DevBuf d_acc;               // batched path: accumulators in global memory, int64[jobs][2][2048]
    int parts = 1, pw = 0;      // N = 2048 with a wide gadget base: digit parts and their width (MKBRArgs)
    DevBuf d_bara, d_barb, d_u, d_tmp;
    DevBuf d_tv, d_lut_idx;     // programmable bootstrap: Torus64 test-vector table and per-sample table index (grow-only)
    Stage stage;
    LinBufs lin;      // dense layer (thfhe_mk_lwe_linear, thfhe_mk_linear_lut_bootstrap)
    DagBuffers dag;   // gate-DAG executor tables (thfhe_dag.h)
    size_t dag_slice = 8192;  // gates per launch of a DAG level
    // multi-value bootstrap (thfhe_mk_mv_lut_bootstrap): the factor tables of a flat call (d_tv holds its base vector); the base vectors
    // and the factor array of a gate-DAG run (thfhe_mk_dag_run_mv_batch)
    DevBuf d_mv_w, d_dag_mv_tv0, d_dag_mv_w;
    size_t mv_slice = 4096;   // output records (samples x q) per slice of a multi-value call: (N + 1) x 4 B of d_u each
    // packing key switch, encrypted tables and the tree
    DevBuf d_pk;                              // the packing key int64[D][t][R][2][N] (thfhe_mk_pack_key_set)
    int pk_D = 0, pk_t = 0, pk_basebit = 0;   // its shape; pk_D == 0: no key
    DevBuf d_tva;                             // encrypted tables: the masks (d_tv holds the bodies)
    DevBuf d_pin, d_pt;                       // a packing call's records and the per-record sums T int64[records][2][N]
    DevBuf d_tab_a, d_tab_b, d_tree_tab;      // a tree slice's packed tables (mask, body) and table indices
    size_t tree_slice = 16384;                // level-1 candidates (samples x p_hi) per slice of a tree or packing call: 2 N x 8 B of d_pt each
    DevBuf d_dag_enc_a, d_dag_enc_b, d_dag_tv1;   // a gate-DAG run's encrypted tables and level-1 rows (thfhe_mk_dag_run_tree_batch)
    size_t pack_wide_threshold = kMkPackWideDefault;   // record counts from here on pack with mk_pack_rows_wide_kernel; 0: never
    // leveled lookup on this ring (thfhe_mk_lhe_cmux, thfhe_mk_lhe_lookup): the CMux tree's workspace (masks, bodies) and the flat CMux's four operands
    DevBuf d_lhe_a, d_lhe_b, d_lhe_in[4];
};

namespace {

// workspace of `jobs` rotations: bara / barb, one extracted record each, the MUX halves; theta > 0: of PBS jobs with theta records each, plus
// their accumulators
int mk_ensure_workspace(thfhe_mk_ctx *c, size_t jobs, int theta = 0) {
    int rc = c->d_bara.grow(jobs * c->w_pad * sizeof(int32_t));
    if (!rc) rc = c->d_barb.grow(jobs * sizeof(int32_t));
    if (!rc) rc = c->d_u.grow(jobs * std::max(theta, 1) * ((size_t)c->p.N + 1) * sizeof(int32_t));
    if (!rc) rc = c->d_tmp.grow(jobs * c->rec_words() * sizeof(int32_t));
    if (!rc && theta) rc = c->d_acc.grow(jobs * 2 * (size_t)c->p.N * sizeof(int64_t));
    return rc;
}

__global__ void mk_extract_kernel(const int64_t *__restrict__ acc, int32_t *__restrict__ out, long jobs, int N);
int mk_launch_rotation(thfhe_mk_ctx *c, const MKBRArgs &a);

// bootstrap (prologue + blind rotate + key switch) of `jobs` = gates * rot jobs; results to d_dst[jobs][P*n+1]
// the key switch of `count` extracted records of N + 1 words (one mask for all parties) into d_out; the plain kernel's coordinate ranges
// fill the chip at small batch sizes, and a block holds <= 2048 mask words
int mk_keyswitch(thfhe_mk_ctx *c, const int32_t *d_u, int32_t *d_out, size_t count) {
    const size_t s = count * c->p.parties;
    const int nsplit = s <= 64 ? 16 : (s <= 256 ? 4 : (c->p.N > 2048 ? 2 : 1));
    return ks_enqueue(c->ksk, c->ksk.args(d_u, d_out, (long)count), nsplit, c->stream);
}

int mk_enqueue_bootstraps(thfhe_mk_ctx *c, const int32_t *d0, const int32_t *d1, const int32_t *d2, MKLin L0, MKLin L1, int rot,
                          size_t gates, int64_t mu, int32_t *d_dst, const int32_t *d_ops = nullptr) {
    const size_t jobs = gates * rot;
    if (c->profiling) THFHE_HIP(hipEventRecord(c->ev[0], c->stream));
    dim3 pg((unsigned)((c->rec_words() + 255) / 256), (unsigned)jobs);
    hipLaunchKernelGGL(mk_prologue_kernel, pg, dim3(256), 0, c->stream, d0, d1, d2, L0, L1, d_ops, rot, c->words, c->w_pad, c->log2_2n, (long)jobs, c->d_bara.as<int32_t>(), c->d_barb.as<int32_t>());
    if (c->profiling) THFHE_HIP(hipEventRecord(c->ev[1], c->stream));
    MKBRArgs a{c->d_bk.as<cplx>(), c->d_tw.as<cplx>(), c->d_bara.as<int32_t>(), c->d_barb.as<int32_t>(), c->d_u.as<int32_t>(), (long)jobs, c->p.parties * c->p.n, c->w_pad, c->p.Bgbit, mu};
    {
        int rc = mk_launch_rotation(c, a);
        if (rc) return rc;
    }
    if (c->profiling) THFHE_HIP(hipEventRecord(c->ev[2], c->stream));
    THFHE_TRY(mk_keyswitch(c, c->d_u.as<int32_t>(), d_dst, jobs));
    if (c->profiling) {
        THFHE_HIP(hipEventRecord(c->ev[3], c->stream));
        c->ev_valid = true;
    }
    return THFHE_OK;
}

// One PBS stage on the context's stream, the workspace sized by the caller (mk_ensure_workspace with theta): the prologue of `jobs` jobs of `src`, the
// accumulator start from each job's table of d_tv, the rotation of mk_bootstrap_3gen, extraction of theta coefficients into d_u [jobs][theta][N+1];
// then, with ks_dst, the key switch of the jobs x theta records into it.  A source that writes no table index rotates on d_idx (null: table 0).
// timed: the profiling events of a flat call (prologue + accumulator start | rotation + extraction | key switch); a gate-DAG run records none.
// d_tva: the tables are RLWE samples (d_tva, d_tv) under Z; the accumulator starts at (X^{-barb} d_tva[t], X^{-barb} d_tv[t]).
// mv: every job rotates the ONE base vector d_tv (theta is 1), the index picks its factor table, and the extraction is
// mk_extract_mv_kernel's mv->q records per job, d_u [jobs][q][N+1].
template <typename Src>
int mk_enqueue_pbs(thfhe_mk_ctx *c, const Src &src, size_t jobs, const int64_t *d_tv, const int64_t *d_tva, int theta, const int32_t *d_idx, int32_t *ks_dst,
                   bool timed = false, const MkMvArgs *mv = nullptr) {
    const int N = c->p.N;
    const bool ev = timed && c->profiling;
    int32_t *const idx = c->d_lut_idx.as<int32_t>();
    if (Src::kIdx != LutIdx::none) d_idx = idx;   // the prologue writes the index the rotation reads
    int64_t *acc = c->d_acc.as<int64_t>();
    if (ev) THFHE_HIP(hipEventRecord(c->ev[0], c->stream));
    lut_prologue_launch(src, jobs, c->words, c->w_pad, c->log2_2n, c->d_bara.as<int32_t>(), c->d_barb.as<int32_t>(), idx, c->stream);
    if (d_tva)   // an encrypted table: both polynomials start rotated
        hipLaunchKernelGGL(mk_lut_acc_init_enc_kernel, dim3((unsigned)jobs), dim3(256), 0, c->stream, c->d_barb.as<int32_t>(), d_tva, d_tv, d_idx, (long)jobs, N,
                           acc);
    else
        hipLaunchKernelGGL(mk_lut_acc_init_kernel, dim3((unsigned)jobs), dim3(256), 0, c->stream, c->d_barb.as<int32_t>(), d_tv, mv ? nullptr : d_idx,
                           (long)jobs, N, acc);
    if (ev) THFHE_HIP(hipEventRecord(c->ev[1], c->stream));
    // acc_in == acc_out == d_acc: every rotation shape may run in place.  The N = 1024 / 2048 coop and pair kernels copy their job's
    // accumulator(s) into LDS before the first barrier and write them back only after the last CMux, and no workgroup touches another job's
    // slot; the batched two-level path (c->batched) always rotates the global accumulator in place; the N = 4096 path skips its copy when
    // acc_in is the accumulator it rotates.  barb is not read when acc_in is given: the start above already applied X^{-barb}.
    MKBRArgs a{c->d_bk.as<cplx>(), c->d_tw.as<cplx>(), c->d_bara.as<int32_t>(), c->d_barb.as<int32_t>(), nullptr, (long)jobs, c->p.parties * c->p.n,
               c->w_pad, c->p.Bgbit, 0, acc, acc};
    THFHE_TRY(mk_launch_rotation(c, a));
    if (mv) {
        const dim3 grid((unsigned)jobs), block(256);
        switch (N) {
        case 1024: hipLaunchKernelGGL(mk_extract_mv_kernel<1024>, grid, block, 0, c->stream, (const int64_t *)acc, *mv, d_idx, (long)jobs, c->d_u.as<int32_t>()); break;
        case 2048: hipLaunchKernelGGL(mk_extract_mv_kernel<2048>, grid, block, 0, c->stream, (const int64_t *)acc, *mv, d_idx, (long)jobs, c->d_u.as<int32_t>()); break;
        default: hipLaunchKernelGGL(mk_extract_mv_kernel<4096>, grid, block, 0, c->stream, (const int64_t *)acc, *mv, d_idx, (long)jobs, c->d_u.as<int32_t>()); break;
        }
    } else {
        hipLaunchKernelGGL(mk_extract_at_kernel, dim3((unsigned)jobs, (unsigned)theta), dim3(256), 0, c->stream, (const int64_t *)acc, c->d_u.as<int32_t>(),
                           (long)jobs, N, theta);
    }
    if (ev) THFHE_HIP(hipEventRecord(c->ev[2], c->stream));
    if (ks_dst) THFHE_TRY(mk_keyswitch(c, c->d_u.as<int32_t>(), ks_dst, jobs * (mv ? mv->q : theta)));
    if (ev) {
        THFHE_HIP(hipEventRecord(c->ev[3], c->stream));
        c->ev_valid = true;
    }
    THFHE_HIP(hipGetLastError());
    return THFHE_OK;
}

int mk_launch_rotation(thfhe_mk_ctx *c, const MKBRArgs &a) {
    using namespace launch_plan;
    const dim3 grid((unsigned)a.jobs), block(512);
    const MkChoice ch = mk_rotation_choice(c->p.N, c->p.l, c->parts, c->batched, a.jobs, c->pair_threshold);   // thfhe_launch_plan.h
    if (ch.family == kR4k) {
        // ring of degree 4096: accumulators in global memory, rotated in place by r4k_rotate_kernel (thfhe_rot4k.h)
        int64_t *acc = a.acc_out;
        if (!acc) {
            THFHE_TRY(c->d_acc.grow((size_t)a.jobs * 8192 * sizeof(int64_t)));
            acc = c->d_acc.as<int64_t>();
        }
        if (!a.acc_in) hipLaunchKernelGGL(mk_acc_init_2k_kernel, dim3((unsigned)a.jobs), dim3(256), 0, c->stream, a.barb, a.mu, a.jobs, acc, 4096);
        else if (a.acc_in != acc) THFHE_HIP(hipMemcpyAsync(acc, a.acc_in, (size_t)a.jobs * 8192 * sizeof(int64_t), hipMemcpyDeviceToDevice, c->stream));
        R4KArgs k{c->d_bk.as<cplx>(), c->d_tw.as<cplx>(), a.bara, acc, a.jobs, a.pn, c->p.l, c->p.Bgbit, c->parts, c->pw, a.w_pad};
        const size_t park_bytes = (size_t)a.jobs * 8 * 2 * 512 * sizeof(cplx);   // 128 KiB per workgroup for the parked partial spectra (thfhe_rot4k.h)
        if (park_bytes > c->park.bytes()) {
            THFHE_HIP(hipStreamSynchronize(c->stream));
            THFHE_TRY(c->park.grow(park_bytes));
        }
        hipLaunchKernelGGL(r4k_rotate_kernel, grid, block, 0, c->stream, k, c->park.as<cplx>());
        if (!a.acc_out) hipLaunchKernelGGL(mk_extract_kernel, grid, dim3(256), 0, c->stream, (const int64_t *)acc, a.out, a.jobs, 4096);
        THFHE_HIP(hipGetLastError());
        return THFHE_OK;
    }
    if (ch.family == kRot2kSingle || ch.family == kRot2kPair) {   // rot2k_launch takes the one of the two
        // accumulators in global memory: start (unless the caller hands one in), rotate by all P n key bits in place, then extract (unless the caller wants
        // the accumulator itself)
        int64_t *acc = a.acc_out;
        if (!acc) {
            THFHE_TRY(c->d_acc.grow((size_t)a.jobs * 4096 * sizeof(int64_t)));
            acc = c->d_acc.as<int64_t>();
        }
        if (!a.acc_in) hipLaunchKernelGGL(mk_acc_init_2k_kernel, dim3((unsigned)a.jobs), dim3(256), 0, c->stream, a.barb, a.mu, a.jobs, acc);
        KmsBRArgs k{c->d_bk.as<cplx>(), c->d_tw.as<cplx>(), a.bara, acc, a.acc_in ? a.acc_in : acc, a.jobs, a.pn, c->p.l, c->p.Bgbit, c->parts, c->pw, 1, 1, a.w_pad};
        {
            int rc = rot2k_launch(k, c->stream, c->pair_threshold, c->park);
            if (rc) return rc;
        }
        if (!a.acc_out) hipLaunchKernelGGL(mk_extract_kernel, grid, dim3(256), 0, c->stream, (const int64_t *)acc, a.out, a.jobs, 2048);
        THFHE_HIP(hipGetLastError());
        return THFHE_OK;
    }
    // the one-pass kernels: two gates per workgroup share every key chunk (more gates than CUs, also the party-sharded pieces), else one
    const dim3 pgrid((unsigned)((a.jobs + 1) / 2));
    MKBRArgs b = a;   // N = 2048: with the digit parts
    b.parts = c->parts;
    b.pw = c->pw;
    constexpr const char *kBadLE = "N = 2048 needs l x digit parts <= 3";
    int rc;
    switch (ch.family) {
    case kPair2k: rc = with_static_int<3>(ch.LE, kBadLE, [&](auto le) { hipLaunchKernelGGL(mk_blind_rotate_pair2k_kernel<decltype(le)::value>, pgrid, block, 0, c->stream, b); }); break;
    case kCoop2k: rc = with_static_int<3>(ch.LE, kBadLE, [&](auto le) { hipLaunchKernelGGL(mk_blind_rotate_coop2k_kernel<decltype(le)::value>, grid, block, 0, c->stream, b); }); break;
    case kMkPair: rc = with_static_int<3>(ch.LE, kBadL, [&](auto l) { hipLaunchKernelGGL(mk_blind_rotate_pair_kernel<decltype(l)::value>, pgrid, block, 0, c->stream, a); }); break;
    default: rc = with_static_int<4>(ch.LE, kBadL, [&](auto l) { hipLaunchKernelGGL(mk_blind_rotate_coop_kernel<decltype(l)::value>, grid, block, 0, c->stream, a); }); break;
    }
    if (rc) return rc;
    THFHE_HIP(hipGetLastError());
    return THFHE_OK;
}

__global__ __launch_bounds__(256) void mk_extract_kernel(const int64_t *__restrict__ acc, int32_t *__restrict__ out, long jobs, int N) {
    const long job = blockIdx.x;
    if (job >= jobs) return;
    const int64_t *ap = acc + job * 2 * N;
    for (int q = threadIdx.x; q <= N; q += 256) {
        int64_t v = q == N ? ap[N] : (q == 0 ? ap[0] : (int64_t)(0ull - (uint64_t)ap[N - q]));
        out[job * (N + 1) + q] = t64tot32(v);
    }
}

// party-sharded prologue: the gate's linear part + mod-switch for the n mask words of this context's block of parties (record
// words [first_word, first_word + n), n = parties_of_this_context * n_lwe) and for b.  Records have rec_words = P_total * n_lwe + 1 words.
__global__ __launch_bounds__(256) void mk_prologue_slice_kernel(const int32_t *__restrict__ in0, const int32_t *__restrict__ in1,
                                                                 const int32_t *__restrict__ in2, MKLin L, int rec_words, int first_word, int n,
                                                                 int log2_2n, long jobs, int32_t *__restrict__ bara, int32_t *__restrict__ barb) {
    const long job = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (job >= jobs || i > n) return;
    const size_t off = (size_t)job * rec_words + (i == n ? rec_words - 1 : first_word + i);
    uint32_t v = (uint32_t)L.cx * (uint32_t)in0[off];
    if (L.cy != 0) v += (uint32_t)L.cy * (uint32_t)in1[off];
    if (L.cz != 0) v += (uint32_t)L.cz * (uint32_t)in2[off];
    if (i == n) {
        v += (uint32_t)L.cb;
        barb[job] = modswitch2n((int32_t)v, log2_2n);
    } else {
        bara[job * n + i] = modswitch2n((int32_t)v, log2_2n);
    }
}

int mk_gates_dev_locked(thfhe_mk_ctx *c, int op, const int32_t *d0, const int32_t *d1, const int32_t *d2, int32_t *dout, size_t count) {
    if (count == 0) return THFHE_OK;
    if (count > (size_t)INT32_MAX / 4) return thfhe_fail(THFHE_E_INVALID, "count too large");
    THFHE_HIP(hipSetDevice(c->device));
    const size_t rec = c->rec_words(), words = count * rec;
    const unsigned lb = (unsigned)((words + 255) / 256);
    if (op == THFHE_NOT || op == THFHE_COPY) {
        hipLaunchKernelGGL(mk_linear_kernel, dim3(lb), dim3(256), 0, c->stream, d0, d0, dout, words, rec, op == THFHE_NOT ? 1 : 0);
        THFHE_HIP(hipGetLastError());
        return THFHE_OK;
    }
    MKLin L0, L1;
    if (!mk_gate_lin(op, 0, L0) || op == kOpIdentity) return thfhe_fail(THFHE_E_INVALID, "gate not defined for the 3-gen multi-key scheme");
    mk_gate_lin(op, 1, L1);
    if (!d1 || ((op == THFHE_MUX || op == THFHE_AND3) && !d2)) return thfhe_fail(THFHE_E_INVALID, "null operand");
    const int64_t MU = (int64_t)1 << 61;  // encode_message64(1, 8)
    if (op != THFHE_MUX) {
        int rc = mk_ensure_workspace(c, count);
        if (rc) return rc;
        return mk_enqueue_bootstraps(c, d0, d1, d2, L0, L0, 1, count, MU, dout);
    }
    // MUX: t1 = AND(x, y), t2 = AND(-x, z) as two full bootstraps, then (0, 1/8) + t1 + t2 without bootstrapping
    int rc = mk_ensure_workspace(c, 2 * count);
    if (rc) return rc;
    rc = mk_enqueue_bootstraps(c, d0, d1, d2, L0, L1, 2, count, MU, c->d_tmp.as<int32_t>());  // job 2g: AND(x,y); job 2g+1: AND(-x,z)
    if (rc) return rc;
    // d_tmp holds [t1_0, t2_0, t1_1, t2_1, ...]: out = (0, 1/8) + t1 + t2            J/3gen_mk_gates.jl:144-147
    hipLaunchKernelGGL(mk_mux_combine_kernel, dim3(lb), dim3(256), 0, c->stream, c->d_tmp.as<int32_t>(), dout, words, rec);
    THFHE_HIP(hipGetLastError());
    return THFHE_OK;
}

// gate classes of the 3-gen gate DAG (thfhe_dag.h): two-input gates NAND / OR / AND / XOR, MUX, NOT / COPY, AND3
int mk_dag_classify(int op) {
    if (op == THFHE_NOT || op == THFHE_COPY) return kDagLinear;
    if (op == THFHE_MUX) return kDagMux;
    if (op == THFHE_AND3) return kDagGate3;
    return op == THFHE_NAND || op == THFHE_OR || op == THFHE_AND || op == THFHE_XOR ? kDagGate2 : -1;
}

// one launch of a gate-DAG gate class from the staging arrays into stage.out (dag_execute's run): two-input gates with per-gate opcodes, MUX
// or AND3
int mk_dag_gate_class(thfhe_mk_ctx *c, int cls, const int32_t *d_ops, size_t n) {
    MKLin L;
    mk_gate_lin(THFHE_NAND, 0, L);
    if (cls == kDagGate2) return mk_enqueue_bootstraps(c, c->stage.in_ptr(0), c->stage.in_ptr(1), nullptr, L, L, 1, n, (int64_t)1 << 61, c->stage.out_ptr(), d_ops);
    return mk_gates_dev_locked(c, cls == kDagMux ? THFHE_MUX : THFHE_AND3, c->stage.in_ptr(0), c->stage.in_ptr(1), c->stage.in_ptr(2), c->stage.out_ptr(), n);
}

// dag_execute's ensure (dag_ensure, thfhe_pbs_host.h) on this engine's workspace
int mk_dag_ensure(thfhe_mk_ctx *c, size_t max_gates, int theta_max, int32_t **in, int32_t **out) {
    return dag_ensure(c, max_gates, theta_max, in, out, [&](size_t jobs, int theta) { return mk_ensure_workspace(c, jobs, theta); });
}

// thfhe_mk_lwe_linear / thfhe_mk_linear_lut_bootstrap(_wo_keyswitch): ctx_linear (thfhe_pbs_host.h) on this engine's workspace and PBS stage
int mk_linear(thfhe_mk_ctx *c, const int32_t *W, const int32_t *bias, int M, int K, bool fused, int theta, const int64_t *tv, int n_luts,
              const int32_t *lut_index, const int32_t *in, int32_t *out, size_t count, bool keyswitch) {
    return ctx_linear(c, W, bias, M, K, fused, theta, tv, n_luts, lut_index, in, out, count, keyswitch,
                      [&](size_t jobs, int th) { return mk_ensure_workspace(c, jobs, th); }, [&](auto &&...a) { return mk_enqueue_pbs(c, a...); });
}

// thfhe_mk_lut_bootstrap(_enc)(_wo_keyswitch): ctx_lut_bootstrap (thfhe_pbs_host.h) on this engine's workspace and PBS stage; the encrypted tables
// are RLWE samples (tv_a, tv) under Z
int mk_lut_bootstrap(thfhe_mk_ctx *c, const thfhe_lut_spec *sp, const int64_t *tv, int n_luts, const int32_t *lut_index, const int32_t *in0,
                     const int32_t *in1, const int32_t *in2, int32_t *out, size_t count, bool keyswitch, bool enc = false, const int64_t *tv_a = nullptr) {
    return ctx_lut_bootstrap(c, sp, tv, tv_a, enc, n_luts, lut_index, in0, in1, in2, out, count, keyswitch,
                             [&](size_t jobs, int theta) { return mk_ensure_workspace(c, jobs, theta); }, [&](auto &&...a) { return mk_enqueue_pbs(c, a...); });
}

// ---- the packing key switch and the two-digit tree ----
// host checks of a packing call that need no context
int mk_pack_validate(const int32_t *recs, size_t count, int p, const int64_t *tv_a, const int64_t *tv_b) {
    if (!recs || !tv_a || !tv_b) return thfhe_fail(THFHE_E_INVALID, "null argument");
    if (p < 2 || p > 64 || (p & (p - 1))) return thfhe_fail(THFHE_E_INVALID, "pack: p must be a power of two in 2 .. 64");
    if (count % (size_t)p) return thfhe_fail(THFHE_E_INVALID, "pack: count must be a multiple of p");
    if (count > (size_t)INT32_MAX / 16) return thfhe_fail(THFHE_E_INVALID, "count too large");
    return THFHE_OK;
}

// grow the scratch of packing `count` records: their sums T
int mk_pack_reserve(thfhe_mk_ctx *c, size_t count) { return c->d_pt.grow(count * 2 * (size_t)c->p.N * sizeof(int64_t)); }

// thfhe_mk_pack_boxes on device records, enqueued on the context's stream: d_recs int32[count][D + 1] (D = the packing key's), count a multiple of p
// -> d_a, d_b int64[count / p][N].  The scratch is sized by mk_pack_reserve.
int mk_pack_enqueue(thfhe_mk_ctx *c, const int32_t *d_recs, size_t count, int p, int64_t *d_a, int64_t *d_b) {
    const int N = c->p.N;
    const MkPackArgs a{d_recs, c->d_pk.as<int64_t>(), c->d_pt.as<int64_t>(), (long)count, c->pk_D, c->pk_t, c->pk_basebit, N};
    if (launch_plan::mk_pack_wide(count, c->pack_wide_threshold))   // the one place the two rows kernels are chosen between
        hipLaunchKernelGGL(mk_pack_rows_wide_kernel, dim3((unsigned)((count + kMkPackWideGroup - 1) / kMkPackWideGroup), (unsigned)(2 * N / kMkPackWideTile)), dim3(256), 0, c->stream, a);
    else
        hipLaunchKernelGGL(mk_pack_rows_kernel, dim3((unsigned)((count + kMkPackGroup - 1) / kMkPackGroup), (unsigned)(2 * N / kMkPackTile)), dim3(256), 0, c->stream, a);
    const dim3 grid((unsigned)(count / p), 2), block(1024);
    const int64_t *T = c->d_pt.as<int64_t>();
    switch (N) {
    case 1024: hipLaunchKernelGGL(mk_pack_boxes_kernel<1024>, grid, block, 0, c->stream, T, p, d_a, d_b); break;
    case 2048: hipLaunchKernelGGL(mk_pack_boxes_kernel<2048>, grid, block, 0, c->stream, T, p, d_a, d_b); break;
    default: hipLaunchKernelGGL(mk_pack_boxes_kernel<4096>, grid, block, 0, c->stream, T, p, d_a, d_b); break;
    }
    THFHE_HIP(hipGetLastError());
    return THFHE_OK;
}

// thfhe_mk_pack_boxes: in slices of at most tree_slice records (a multiple of p): only a slice's records go up and its tables come down
int mk_pack_boxes(thfhe_mk_ctx *c, const int32_t *recs, size_t count, int p, int64_t *tv_a, int64_t *tv_b) {
    THFHE_TRY(mk_pack_validate(recs, count, p, tv_a, tv_b));
    if (!c) return thfhe_fail(THFHE_E_INVALID, "null ctx");
    DevLock lk(*c);
    if (lk.rc) return lk.rc;
    if (!c->pk_D) return thfhe_fail(THFHE_E_INVALID, "pack: no packing key set (thfhe_mk_pack_key_set)");
    if (count == 0) return THFHE_OK;
    const size_t N = c->p.N, rec = (size_t)c->pk_D + 1;
    const size_t S_max = std::min(count, std::max<size_t>(1, c->tree_slice / p) * p);
    int rc = mk_pack_reserve(c, S_max);
    if (!rc) rc = c->d_pin.grow(S_max * rec * sizeof(int32_t));
    if (!rc) rc = c->d_tab_a.grow(S_max / p * N * sizeof(int64_t));
    if (!rc) rc = c->d_tab_b.grow(S_max / p * N * sizeof(int64_t));
    if (rc) return rc;
    for (size_t s0 = 0; s0 < count; s0 += S_max) {
        const size_t S = std::min(S_max, count - s0), tab_bytes = S / p * N * sizeof(int64_t);
        THFHE_HIP(hipMemcpyAsync(c->d_pin.as<int32_t>(), recs + s0 * rec, S * rec * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
        THFHE_TRY(mk_pack_enqueue(c, c->d_pin.as<int32_t>(), S, p, c->d_tab_a.as<int64_t>(), c->d_tab_b.as<int64_t>()));
        THFHE_HIP(hipMemcpyAsync(tv_a + s0 / p * N, c->d_tab_a.as<int64_t>(), tab_bytes, hipMemcpyDeviceToHost, c->stream));
        THFHE_HIP(hipMemcpyAsync(tv_b + s0 / p * N, c->d_tab_b.as<int64_t>(), tab_bytes, hipMemcpyDeviceToHost, c->stream));
    }
    THFHE_HIP(hipStreamSynchronize(c->stream));
    return THFHE_OK;
}

// what tree_validate_rows (thfhe_pbs_host.h) admits here: p_hi up to the 64 records one packing takes
constexpr TreeRules kMkTreeRules{64, "tree: p_hi must be a power of two in 2 .. 64", "tree: n_tables must be >= 1 and n_tables * p_hi / theta <= 262144"};

// the packing key of a tree: set, and taking the [N + 1] records level 1 leaves in d_u
int mk_tree_key_check(const thfhe_mk_ctx *c, size_t N) {
    if (!c->pk_D) return thfhe_fail(THFHE_E_INVALID, "tree: no packing key set (thfhe_mk_pack_key_set)");
    if (c->pk_D != (int)N) return thfhe_fail(THFHE_E_INVALID, "tree: the packing key must take the ring key's coefficients (D = N)");
    return THFHE_OK;
}

// Grow-only workspace of one tree chain over S samples / nodes: S R level-1 rotations of theta_lo records each (their accumulators, the S k p
// candidates in d_u), S k selection rotations, an index per job of the larger stage, the packing sums of the S k p candidates and the S k packed
// tables (k tables per sample, DESIGN 4.23: R = 1, theta_lo = k p).  With k = 1 the second grow and the max are redundant -- S <= S R, one record
// per job <= theta_lo -- and the sizes are those of the first.
int mk_tree_workspace(thfhe_mk_ctx *c, size_t S, size_t p, size_t R, size_t theta_lo, size_t k = 1) {
    const size_t N = c->p.N;
    int rc = mk_ensure_workspace(c, S * R, (int)theta_lo);
    if (!rc) rc = mk_ensure_workspace(c, S * k, 1);
    if (!rc) rc = c->d_lut_idx.grow(std::max(S * R, S * k) * sizeof(int32_t));
    if (!rc) rc = mk_pack_reserve(c, S * k * p);
    if (!rc) rc = c->d_tab_a.grow(S * k * N * sizeof(int64_t));
    if (!rc) rc = c->d_tab_b.grow(S * k * N * sizeof(int64_t));
    return rc;
}

// One tree chain over S samples / nodes on the context's stream, the workspace sized by mk_tree_workspace, nothing visiting the host
// in between.  Level 1: S (p / theta_lo) many-LUT rotations of the plaintext rows d_tv1 on the `lo` source, no key switch -- the S p candidates stay
// in d_u as [N + 1] records under the coefficients of Z, candidate h of sample s at record s p + h, the order the rotations write them in.  Then
// mk_pack_enqueue with the D = N key packs them in place into S encrypted tables (d_tab_a[s], d_tab_b[s]), and the selection: sample s rotates its
// own table on the `hi` source, theta = 1, coefficient 0, mk_keyswitch into d_out.  seam(1) / seam(2) run after level 1 and after the packing: what
// the caller has to put on the stream there.  mv: level 1 is ONE multi-value rotation per sample of the base vector d_tv1 with
// mk_extract_mv_kernel's theta_lo = k p outputs (taps of the job's table, out_bias on the body) -- output j p + h is candidate h of table j, at
// record s k p + j p + h, so the packed table of (s, j) is sample s k + j, and selection job s k + j rotates it on sample s's `hi` operands (the
// `hi` source repeats every sample k times and numbers its jobs): S k records into d_out.
template <typename Lo, typename Hi, typename Seam>
int mk_enqueue_tree_chain(thfhe_mk_ctx *c, const Lo &lo, const int64_t *d_tv1, int theta_lo, const Hi &hi, size_t S, int p, int32_t *d_out, Seam seam,
                          const MkMvArgs *mv = nullptr, size_t k = 1) {
    int64_t *const tab_a = c->d_tab_a.as<int64_t>(), *const tab_b = c->d_tab_b.as<int64_t>();
    THFHE_TRY(mk_enqueue_pbs(c, lo, mv ? S : S * (p / theta_lo), d_tv1, nullptr, mv ? 1 : theta_lo, nullptr, nullptr, false, mv));
    THFHE_TRY(seam(1));
    THFHE_TRY(mk_pack_enqueue(c, c->d_u.as<int32_t>(), S * k * p, p, tab_a, tab_b));
    THFHE_TRY(seam(2));
    return mk_enqueue_pbs(c, hi, S * k, tab_b, tab_a, 1, nullptr, d_out);
}

// mk_enqueue_tree_chain into stage.out as the shared call bodies (thfhe_pbs_host.h) call it; w, mv_p: the taps of a multi-value level 1 (null: rows)
auto mk_tree_chain_of(thfhe_mk_ctx *c, int64_t out_bias) {
    return [=](const auto &lo, const int64_t *d_tv1, int theta_lo, const auto &hi, size_t S, int p, auto seam, const int32_t *w, int mv_p, size_t k) {
        const MkMvArgs mv{w, mv_p, (int)k * p, out_bias};
        return mk_enqueue_tree_chain(c, lo, d_tv1, theta_lo, hi, S, p, c->stage.out_ptr(), seam, w ? &mv : nullptr, k);
    };
}

// thfhe_mk_tree_lut_bootstrap(_mvk): the lock and the packing key's check, then ctx_tree_bootstrap (thfhe_pbs_host.h) on this
// engine's tree workspace and chain, every profiling event on the call's last slice.  The arguments have passed the entry's host checks.
int mk_tree_bootstrap(thfhe_mk_ctx *c, const thfhe_lut_spec &lo, const thfhe_lut_spec &hi, int p_hi, const int64_t *tv, size_t tv_rows, const int32_t *factors,
                      int p_lo, int n_tables, const int32_t *table_index, int64_t out_bias, const int32_t *lo0, const int32_t *lo1, const int32_t *lo2,
                      const int32_t *hi0, const int32_t *hi1, const int32_t *hi2, int32_t *out, size_t count, int k = 1) {
    if (!c) return thfhe_fail(THFHE_E_INVALID, "null ctx");
    DevLock lk(*c);
    if (lk.rc) return lk.rc;
    THFHE_TRY(mk_tree_key_check(c, c->p.N));
    return ctx_tree_bootstrap(c, lo, hi, p_hi, tv, tv_rows, factors, p_lo, n_tables, table_index, lo0, lo1, lo2, hi0, hi1, hi2, out, count, k, false,
                              [&](auto... a) { return mk_tree_workspace(c, a...); }, mk_tree_chain_of(c, out_bias));
}

// thfhe_mk_mv_lut_bootstrap(_wo_keyswitch): ctx_mv_lut_bootstrap (thfhe_pbs_host.h) in slices of at most mv_slice records, one stage
// with the multi-value epilogue per slice
int mk_mv_lut_bootstrap(thfhe_mk_ctx *c, const thfhe_lut_spec *sp, const int64_t *tv0, const int32_t *factors, int p, int q, int n_tables,
                        const int32_t *table_index, int64_t out_bias, const int32_t *in0, const int32_t *in1, const int32_t *in2, int32_t *out, size_t count,
                        bool keyswitch) {
    return ctx_mv_lut_bootstrap(c, sp, tv0, factors, p, q, n_tables, table_index, in0, in1, in2, out, count, keyswitch, &thfhe_mk_ctx::mv_slice,
                                [&](size_t jobs, int theta) { return mk_ensure_workspace(c, jobs, theta); },
                                [&](const auto &src, size_t S, const int32_t *d_idx, int32_t *ks_dst, bool last) {
                                    const MkMvArgs mv{c->d_mv_w.as<int32_t>(), p, q, out_bias};
                                    return mk_enqueue_pbs(c, src, S, c->d_tv.as<int64_t>(), nullptr, 1, d_idx, ks_dst, last, &mv);
                                });
}

// The six-column entries of the 3-gen executor (F: the entry's families and the generations it admits): the host checks and the plan before the
// context is looked at, then the run.  The gate classes run as in thfhe_mk_dag_run_batch; a LUT launch group is one PBS stage on the wire table
// (lut_prologue_kernel over the P n + 1 record words) with the key switch into the staging output.  TREE, TREE_MV and MV groups
//  are dag_run_group's (thfhe_pbs_host.h) on this engine's chain and its stage with the multi-value epilogue, MV groups in
// slices by mv_slice; DENSE groups are dag_run_dense_group's on this engine's PBS stage.  Only the PBS stage of a DENSE group's last slice records profiling events.
int mk_dag_run(thfhe_mk_ctx *c, const DagCall &A, const DagFamilies &F, const int64_t *mv_out_bias, size_t instances, int64_t *stats) {
    DagPlan plan;
    if ((F.gens & kDagGenTree) && A.nodes)   // before the plan: a SELECT row has a refusal of its own on this engine
        for (size_t g = 0; g < A.n_nodes; g++)
            if (A.nodes[6 * g] == THFHE_SELECT)
                return thfhe_fail(THFHE_E_INVALID, "SELECT node: not run on the 3-gen engine -- its candidates are key-switched P n-word records and need the "
                                                   "D = P n packing key, trees the D = N key, and a context holds one key");
    THFHE_TRY(dag_checked_plan(A, F, mk_dag_classify, plan));
    for (const DagBatch &b : plan.batches)   // the flat tree's rule: one packing takes at most 64 records
        if (b.cls == kDagTree && F.trees[b.tree].p_hi > kMkTreeRules.p_hi_max) return thfhe_fail(THFHE_E_INVALID, kMkTreeRules.p_hi_text);
    const bool mv_entry = F.gens & kDagGenMv;
    if (stats && mv_entry) plan.fill_stats(stats);   // the plan's figures need no device
    if (!c) return thfhe_fail(THFHE_E_INVALID, "null ctx");
    if (stats && !mv_entry) plan.fill_stats(stats);   // thfhe_mk_dag_run_lut_batch gives them to a caller with a context only
    DevLock lk(*c);
    if (lk.rc) return lk.rc;
    // TREE / TREE_MV groups pack [N + 1] records: the D = N key (SELECT rows never reach a plan of this engine)
    if (plan.has_tree_groups()) THFHE_TRY(mk_tree_key_check(c, c->p.N));
    size_t w_cand = 0;   // not needed: mk_tree_workspace reserves its own packing
    THFHE_TRY(dag_reserve_groups(c, plan, F, instances, &thfhe_mk_ctx::mv_slice, w_cand, [&](auto... a) { return mk_tree_workspace(c, a...); },
                                 [&](size_t jobs, int theta) { return mk_ensure_workspace(c, jobs, theta); }));
    THFHE_TRY(dag_upload_families<int64_t>(c, c->stream, F));
    return dag_execute(
        plan, c->dag, c->stream, c->rec_words(), A, instances, c->dag_slice,
        [&](size_t max_gates, int32_t **in, int32_t **out) { return mk_dag_ensure(c, max_gates, plan.max_theta, in, out); },
        [&](int cls, const int32_t *d_ops, size_t n) { return mk_dag_gate_class(c, cls, d_ops, n); },
        [&](int theta, const DagLutSlice &s) {
            return mk_enqueue_pbs(c, s.src(c->dag.specs.as<thfhe_lut_spec>()), (size_t)s.total, (s.enc ? c->d_dag_enc_b : c->d_tv).as<int64_t>(),
                                  s.enc ? c->d_dag_enc_a.as<int64_t>() : nullptr, theta, nullptr, c->stage.out_ptr());
        },
        [&](const DagExtGroup &g) -> int {
            if (g.cls == kDagDense) return dag_run_dense_group<int64_t>(c, F, g, &thfhe_mk_ctx::mv_slice, [&](auto &&...a) { return mk_enqueue_pbs(c, a...); });
            if (g.cls != kDagTree && g.cls != kDagMv && g.cls != kDagTreeMv) return thfhe_fail(THFHE_E_INVALID, "grouped node kind not defined for the 3-gen engine");
            const int64_t bias = mv_out_bias && g.cls != kDagTree ? mv_out_bias[g.tree] : 0;
            return dag_run_group<int64_t>(c, F, g, &thfhe_mk_ctx::mv_slice, mk_tree_chain_of(c, bias), [&](const auto &lo, size_t S, const int64_t *tv0, const int32_t *w, int mv_p, int q) {
                const MkMvArgs mv{w, mv_p, q, bias};
                return mk_enqueue_pbs(c, lo, S, tv0, nullptr, 1, nullptr, c->stage.out_ptr(), false, &mv);
            });
        });
}

// leveled CMux and table lookup on the ring of degree 2048
#include "thfhe_mk_lhe.h"

}  // namespace

extern "C" {

int thfhe_mk_ctx_create(const thfhe_params *p, const int64_t *bk_coeff, const int32_t *ksk, int device, thfhe_mk_ctx **out) {
    if (!p || !bk_coeff || !ksk || !out) return thfhe_fail(THFHE_E_INVALID, "null argument");
    *out = nullptr;
    if (p->torus_bits != 64) return thfhe_fail(THFHE_E_UNSUPPORTED, "thfhe_mk_ctx_create is the Torus64 3-gen multi-key path");
    if ((p->N != 1024 && p->N != 2048 && p->N != 4096) || p->k != 1) return thfhe_fail(THFHE_E_UNSUPPORTED, "only N = 1024 / 2048 / 4096, k = 1 is implemented");
    if (p->N == 2048 && p->l > 3) return thfhe_fail(THFHE_E_UNSUPPORTED, "N = 2048 needs decomposition length l <= 3");
    if (p->parties < 1 || p->parties > 512) return thfhe_fail(THFHE_E_UNSUPPORTED, "need 1 <= parties <= 512");
    // the digit parts and the batched N = 2048 path: launch_plan::mk_digit_parts (thfhe_launch_plan.h)
    const auto [parts, pw, batched] = launch_plan::mk_digit_parts(p->N, p->l, p->Bgbit);
    const bool ring4k = p->N == 4096;   // thfhe_rot4k.h: at most six row parts, digits from the top 32 bits; |sum| <= 6 x 4096 x 2^8 x 2^15 = 2^37.6 (one level more than N = 2048)
    if (ring4k && (p->l < 1 || 2 * p->l * parts > 6 || p->l * p->Bgbit > 32 || (double)(2 * p->l * parts) * 4096.0 * (double)(1 << ((parts > 1 ? pw : p->Bgbit) - 1)) * 32768.0 > 274877906944.0))
        return thfhe_fail(THFHE_E_UNSUPPORTED, "N = 4096 needs l x ceil(Bgbit / 9) <= 3, l*Bgbit <= 32 and the FP64 exactness bound 2 l parts N 2^(part bits - 1) 2^15 <= 2^38");
    if (p->l < 1 || p->l > 4 || p->Bgbit < 1 || (!batched && p->l * p->Bgbit > 32) || p->l * p->Bgbit > 64 || (parts > 1 && p->N == 1024) || (batched && parts > 2) ||
        (batched && (double)(2 * p->l * parts) * 2048.0 * (double)(1 << ((parts > 1 ? pw : p->Bgbit) - 1)) * 32768.0 > 137438953472.0))
        return thfhe_fail(THFHE_E_UNSUPPORTED, "need 1 <= l <= 4, l*Bgbit <= 32 (64 on the batched path), and Bgbit <= 10 (FP64 exactness bound) unless N = 2048 with l x ceil(Bgbit / 9) <= 3 or two-part digits");
    if (p->n < 1 || p->n > 767) return thfhe_fail(THFHE_E_UNSUPPORTED, "need 1 <= n <= 767");
    if (p->ks_t < 1 || p->ks_basebit < 1 || p->ks_t * p->ks_basebit > 31) return thfhe_fail(THFHE_E_INVALID, "bad key-switch parameters");
    std::unique_ptr<thfhe_mk_ctx> c(new (std::nothrow) thfhe_mk_ctx);
    if (!c) return thfhe_fail(THFHE_E_NOMEM, "out of host memory");
    THFHE_TRY(c->open(device, true));
    c->p = *p;
    c->words = p->parties * p->n;
    c->w_pad = (c->words + 3) & ~3;
    c->log2_2n = ilog2(2 * p->N);
    c->parts = parts;
    c->pw = pw;
    c->batched = batched;
    THFHE_TRY(c->upload_twiddles(p->N));
    if (ring4k || batched) {
        // key table of thfhe_rot4k.h / thfhe_rot2k.h, staged party by party: row part (j l + level) parts + part of output o is
        // part_{mk_part_index(j, o)}[level] shifted left by part * pw bits
        const int l = p->l;
        auto src = [&](int q, int i, int r, int o) { return bk_coeff + ((((size_t)q * p->n + i) * 4 + mk_part_index(r / l, o)) * l + r % l) * p->N; };
        THFHE_TRY(ring4k ? stage_party_keys<4096>(*c, c->d_bk, p->parties, p->n, 2 * l, parts, pw, src)
                         : stage_party_keys<2048>(*c, c->d_bk, p->parties, p->n, 2 * l, parts, pw, src));
    } else {
        const long PN = (long)p->parties * p->n;
        const size_t coeff_words = (size_t)PN * 4 * p->l * p->N;
        DevBuf coeff;  // upload staging
        THFHE_TRY(coeff.grow(coeff_words * sizeof(int64_t)));
        THFHE_HIP(hipMemcpyAsync(coeff.as<int64_t>(), bk_coeff, coeff_words * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
        const int le = p->l * parts;
        const long npolys = PN * 2 * le * 2;   // (pi, row, output)
        THFHE_TRY(c->d_bk.grow((size_t)npolys * 4 * (p->N / 2) * sizeof(cplx)));
        if (p->N == 2048) {
            if (parts > 1) {   // key rows followed by their copies shifted left by pw, 2 pw bits (wrapping): d (*) K = sum_w d_w (*) (K << pw w)
                DevBuf exp;
                THFHE_TRY(exp.grow(coeff_words * parts * sizeof(int64_t)));
                const long polys = PN * 4 * p->l;
                hipLaunchKernelGGL(mk_expand_parts_kernel, dim3((unsigned)polys, (unsigned)parts), dim3(256), 0, c->stream, coeff.as<int64_t>(), exp.as<int64_t>(), p->l, parts, pw);
                THFHE_HIP(hipGetLastError());
                THFHE_HIP(hipStreamSynchronize(c->stream));
                coeff = std::move(exp);
            }
            THFHE_TRY((launch_torus_transform<2048, 64>(c->stream, coeff.as<int64_t>(), npolys, c->d_tw.as<cplx>(), c->d_bk.as<cplx>(), MkResidentMap{le})));
        } else {
            THFHE_TRY((launch_torus_transform<1024, 64>(c->stream, coeff.as<int64_t>(), npolys, c->d_tw.as<cplx>(), c->d_bk.as<cplx>(), MkResidentMap{le})));
        }
        THFHE_HIP(hipStreamSynchronize(c->stream));   // before `coeff` is freed
    }
    THFHE_TRY(c->ksk.upload(ksk, p->parties, p->N, p->n, p->ks_t, p->ks_basebit, false, c->stream));
    *out = c.release();
    return THFHE_OK;
}

void thfhe_mk_ctx_destroy(thfhe_mk_ctx *c) { ctx_destroy(c); }

int thfhe_mk_ctx_info(const thfhe_mk_ctx *c, thfhe_params *params, int *device) {
    if (!c || !params || !device) return thfhe_fail(THFHE_E_INVALID, "null argument");
    *params = c->p, *device = c->device;
    return THFHE_OK;
}

void *thfhe_mk_dev_alloc(thfhe_mk_ctx *c, size_t bytes) { return ctx_dev_alloc(c, bytes); }
void thfhe_mk_dev_free(thfhe_mk_ctx *c, void *p) { ctx_dev_free(c, p); }
int thfhe_mk_copy_h2d(thfhe_mk_ctx *c, void *dst, const void *src, size_t bytes) { return ctx_copy(c, dst, src, bytes, hipMemcpyHostToDevice); }
int thfhe_mk_copy_d2h(thfhe_mk_ctx *c, void *dst, const void *src, size_t bytes) { return ctx_copy(c, dst, src, bytes, hipMemcpyDeviceToHost); }
int thfhe_mk_reserve(thfhe_mk_ctx *c, size_t max_count) {
    if (!c) return thfhe_fail(THFHE_E_INVALID, "null ctx");
    DevLock lk(*c);
    if (lk.rc) return lk.rc;
    return mk_ensure_workspace(c, max_count * 2);
}
int thfhe_mk_sync(thfhe_mk_ctx *c) { return ctx_sync(c); }
int thfhe_mk_set_profiling(thfhe_mk_ctx *c, int enabled) { return ctx_set_profiling(c, enabled); }
int thfhe_mk_last_timings(thfhe_mk_ctx *c, float ms[4]) { return ctx_last_timings(c, ms); }

int thfhe_mk_gates_dev(thfhe_mk_ctx *c, int op, const int32_t *d0, const int32_t *d1, const int32_t *d2, int32_t *dout, size_t count) {
    if (!c || !d0 || !dout) return thfhe_fail(THFHE_E_INVALID, "null argument");
    std::lock_guard<std::mutex> g(c->mu);
    return mk_gates_dev_locked(c, op, d0, d1, d2, dout, count);
}

int thfhe_mk_gates(thfhe_mk_ctx *c, int op, const int32_t *in0, const int32_t *in1, const int32_t *in2, int32_t *out, size_t count) {
    return ctx_gates(c, in0, in1, in2, out, count, [&](const int32_t *d0, const int32_t *d1, const int32_t *d2, int32_t *dout, size_t n) {
        return mk_gates_dev_locked(c, op, d0, d1, d2, dout, n);
    });
}

// Gate-DAG evaluation for the 3-gen scheme: the reference's integer circuits (mk_add_3gen ... mk_int_mul_3gen, J/3gen_mk_gates.jl:183-362) as
// ASAP levels, wires resident in HBM (thfhe_dag.h), `instances` independent evaluations side by side.  Classes: two-input gates NAND / OR /
// AND / XOR with per-gate opcodes in one launch, AND3, MUX (two ANDs + linear combine, :133-150), NOT / COPY (mk_gate_not_3gen,
// mk_copy_3gen: no bootstrap).
int thfhe_mk_dag_run_batch(thfhe_mk_ctx *c, const int32_t *inputs, size_t n_inputs, const int32_t *gates, size_t n_gates, size_t instances,
                           const int32_t *out_wires, size_t n_out, int32_t *outputs, int64_t *stats) {
    return dag_gates_run_batch(
        c, DagCall{inputs, n_inputs, gates, n_gates, out_wires, n_out, outputs}, instances, stats, mk_dag_classify,
        [&](size_t max_gates, int32_t **in, int32_t **out) { return mk_dag_ensure(c, max_gates, 0, in, out); },
        [&](int cls, const int32_t *d_ops, size_t n) { return mk_dag_gate_class(c, cls, d_ops, n); });
}

// LUT nodes among the 3-gen gates: mk_dag_run with the LUT generation, both families required.
int thfhe_mk_dag_run_lut_batch(thfhe_mk_ctx *c, const int32_t *inputs, size_t n_inputs, const int32_t *nodes, size_t n_nodes,
                               const thfhe_lut_spec *specs, int n_specs, const int64_t *tv, int n_luts, size_t instances, const int32_t *out_wires,
                               size_t n_out, int32_t *outputs, int64_t *stats) {
    return mk_dag_run(c, DagCall{inputs, n_inputs, nodes, n_nodes, out_wires, n_out, outputs}, DagFamilies{kDagGenLut, specs, n_specs, tv, n_luts}, nullptr,
                      instances, stats);
}

// ... and multi-value nodes: MV rows on the run's Torus64 base vectors; without the multi-value families the call is the one above.
int thfhe_mk_dag_run_mv_batch(thfhe_mk_ctx *c, const int32_t *inputs, size_t n_inputs, const int32_t *nodes, size_t n_nodes, const thfhe_lut_spec *specs,
                              int n_specs, const int64_t *tv, int n_luts, const thfhe_mv_spec *mvs, int n_mvs, const int64_t *mv_tv0, int n_bases,
                              const int32_t *mv_factors, size_t n_factor_words, const int64_t *mv_out_bias, size_t instances, const int32_t *out_wires,
                              size_t n_out, int32_t *outputs, int64_t *stats) {
    if (!mvs && !n_mvs && !mv_tv0 && !n_bases && !mv_factors && !n_factor_words)
        return thfhe_mk_dag_run_lut_batch(c, inputs, n_inputs, nodes, n_nodes, specs, n_specs, tv, n_luts, instances, out_wires, n_out, outputs, stats);
    DagFamilies F{kDagGenLut | kDagGenMv, specs, n_specs, tv, n_luts};
    F.mvs = mvs, F.n_mvs = n_mvs, F.mv_tv0 = mv_tv0, F.n_bases = n_bases, F.mv_factors = mv_factors, F.n_factor_words = n_factor_words;
    return mk_dag_run(c, DagCall{inputs, n_inputs, nodes, n_nodes, out_wires, n_out, outputs}, F, mv_out_bias, instances, stats);
}

// ... and encrypted-table, tree and multi-value tree nodes: LUT_ENC rows on the run's RLWE tables, TREE rows on its int64 level-1
// rows, TREE_MV rows on the multi-value families; SELECT rows are refused.  The tree generation's families travel as int64 behind DagFamilies'
// int32 pointers (host pointers: null checks and the upload only).
int thfhe_mk_dag_run_tree_batch(thfhe_mk_ctx *c, const int32_t *inputs, size_t n_inputs, const int32_t *nodes, size_t n_nodes, const thfhe_lut_spec *specs,
                                int n_specs, const int64_t *tv, int n_luts, const int64_t *enc_a, const int64_t *enc_b, int n_enc, const thfhe_tree_spec *trees,
                                int n_trees, const int64_t *tv1, int n_tv1_rows, const thfhe_mv_spec *mvs, int n_mvs, const int64_t *mv_tv0, int n_bases,
                                const int32_t *mv_factors, size_t n_factor_words, const int64_t *mv_out_bias, size_t instances, const int32_t *out_wires,
                                size_t n_out, int32_t *outputs, int64_t *stats) {
    DagFamilies F{kDagGenLut | kDagGenTree | kDagGenMv, specs, n_specs, tv, n_luts, reinterpret_cast<const int32_t *>(enc_a), reinterpret_cast<const int32_t *>(enc_b),
                  n_enc, trees, n_trees, reinterpret_cast<const int32_t *>(tv1), n_tv1_rows};
    F.mvs = mvs, F.n_mvs = n_mvs, F.mv_tv0 = mv_tv0, F.n_bases = n_bases, F.mv_factors = mv_factors, F.n_factor_words = n_factor_words;
    return mk_dag_run(c, DagCall{inputs, n_inputs, nodes, n_nodes, out_wires, n_out, outputs}, F, mv_out_bias, instances, stats);
}

// ... and dense-layer nodes: DENSE rows on the run's Torus64 tables; without the family (dense NULL) the call is the one above.
int thfhe_mk_dag_run_dense_batch(thfhe_mk_ctx *c, const int32_t *inputs, size_t n_inputs, const int32_t *nodes, size_t n_nodes, const thfhe_lut_spec *specs,
                                 int n_specs, const int64_t *tv, int n_luts, const int64_t *enc_a, const int64_t *enc_b, int n_enc, const thfhe_tree_spec *trees,
                                 int n_trees, const int64_t *tv1, int n_tv1_rows, const thfhe_mv_spec *mvs, int n_mvs, const int64_t *mv_tv0, int n_bases,
                                 const int32_t *mv_factors, size_t n_factor_words, const int64_t *mv_out_bias, const thfhe_dag_dense_families *dense,
                                 size_t instances, const int32_t *out_wires, size_t n_out, int32_t *outputs, int64_t *stats) {
    DagFamilies F{kDagGenLut | kDagGenTree | kDagGenMv | (dense ? kDagGenDense : 0u), specs, n_specs, tv, n_luts, reinterpret_cast<const int32_t *>(enc_a),
                  reinterpret_cast<const int32_t *>(enc_b), n_enc, trees, n_trees, reinterpret_cast<const int32_t *>(tv1), n_tv1_rows};
    F.mvs = mvs, F.n_mvs = n_mvs, F.mv_tv0 = mv_tv0, F.n_bases = n_bases, F.mv_factors = mv_factors, F.n_factor_words = n_factor_words, F.dense = dense;
    return mk_dag_run(c, DagCall{inputs, n_inputs, nodes, n_nodes, out_wires, n_out, outputs}, F, mv_out_bias, instances, stats);
}

int thfhe_mk_set_dag_slice(thfhe_mk_ctx *c, size_t max_gates) { return ctx_set_dag_slice(c, max_gates); }

int thfhe_mk_set_mv_slice(thfhe_mk_ctx *c, size_t max_records) {
    if (!c || max_records < 1 || max_records > ((size_t)1 << 20)) return thfhe_fail(THFHE_E_INVALID, "slice must be 1 .. 2^20 records");
    std::lock_guard<std::mutex> g(c->mu);
    c->mv_slice = max_records;
    return THFHE_OK;
}

int thfhe_mk_dag_run(thfhe_mk_ctx *c, int32_t *wires, size_t n_inputs, const int32_t *gates, size_t n_gates, int64_t *stats) {
    return dag_gates_run(c, wires, n_inputs, gates, n_gates, stats, thfhe_mk_dag_run_batch);
}

int thfhe_mk_gates_mixed(thfhe_mk_ctx *c, const int32_t *ops, const int32_t *in0, const int32_t *in1, int32_t *out, size_t count) {
    if (!c || !ops || !in0 || !in1 || !out) return thfhe_fail(THFHE_E_INVALID, "null argument");
    if (count == 0) return THFHE_OK;
    for (size_t g = 0; g < count; g++)
        if (!(ops[g] == THFHE_NAND || ops[g] == THFHE_OR || ops[g] == THFHE_AND || ops[g] == THFHE_XOR))
            return thfhe_fail(THFHE_E_INVALID, "thfhe_mk_gates_mixed takes the two-input 3-gen gates NAND / OR / AND / XOR only");
    MKLin L;
    mk_gate_lin(THFHE_NAND, 0, L);
    return ctx_gates_mixed(c, ops, in0, in1, out, count, [&](const int32_t *d0, const int32_t *d1, const int32_t *d_ops, int32_t *dout) {
        int rc = mk_ensure_workspace(c, count);
        return rc ? rc : mk_enqueue_bootstraps(c, d0, d1, nullptr, L, L, 1, count, (int64_t)1 << 61, dout, d_ops);
    });
}

// ---- party-sharded building blocks (device pointers; see include/thfhe_hip.h and thfhe/party_sharded.py) -------------------
int thfhe_mk_rotate_partial_dev(thfhe_mk_ctx *c, const int32_t *d_bara, const int32_t *d_barb, int64_t mu, const int64_t *d_acc_in,
                                int64_t *d_acc_out, size_t count) {
    if (!c || !d_bara || !d_acc_out || (!d_acc_in && !d_barb)) return thfhe_fail(THFHE_E_INVALID, "null argument");
    if (count == 0) return THFHE_OK;
    DevLock lk(*c);
    if (lk.rc) return lk.rc;
    MKBRArgs a{c->d_bk.as<cplx>(), c->d_tw.as<cplx>(), d_bara, d_barb, nullptr, (long)count, c->p.parties * c->p.n, c->words, c->p.Bgbit, mu, d_acc_in, d_acc_out};
    return mk_launch_rotation(c, a);
}
// the front of mk_enqueue_pbs on the caller's accumulators: the theta-rounded prologue of the records themselves (one input, weight 1, bias 0),
// the start X^{-barb} d_tv from the ONE table, the rotation in place.  The caller extracts.
int thfhe_mk_lut_rotate_dev(thfhe_mk_ctx *c, const int32_t *d_recs, int theta, const int64_t *d_tv, int64_t *d_acc, size_t count) {
    if (!d_recs || !d_tv || !d_acc) return thfhe_fail(THFHE_E_INVALID, "null argument");
    if (theta != 1 && theta != 2 && theta != 4) return thfhe_fail(THFHE_E_INVALID, "theta must be 1, 2 or 4");
    if (count > ((size_t)1 << 24)) return thfhe_fail(THFHE_E_INVALID, "count must be at most 2^24");
    if (!c) return thfhe_fail(THFHE_E_INVALID, "null ctx");
    if (count == 0) return THFHE_OK;
    DevLock lk(*c);
    if (lk.rc) return lk.rc;
    THFHE_TRY(mk_ensure_workspace(c, count));
    thfhe_lut_spec sp{};
    sp.n_inputs = 1, sp.weights[0] = 1, sp.theta = theta;
    const LutFlatSrc<LutIdx::none> src{d_recs, d_recs, d_recs, sp, 1, nullptr};
    lut_prologue_launch(src, count, c->words, c->w_pad, c->log2_2n, c->d_bara.as<int32_t>(), c->d_barb.as<int32_t>(), nullptr, c->stream);
    hipLaunchKernelGGL(mk_lut_acc_init_kernel, dim3((unsigned)count), dim3(256), 0, c->stream, c->d_barb.as<int32_t>(), d_tv, nullptr, (long)count, c->p.N,
                       d_acc);
    THFHE_HIP(hipGetLastError());
    MKBRArgs a{c->d_bk.as<cplx>(), c->d_tw.as<cplx>(), c->d_bara.as<int32_t>(), c->d_barb.as<int32_t>(), nullptr, (long)count, c->p.parties * c->p.n,
               c->w_pad, c->p.Bgbit, 0, d_acc, d_acc};
    return mk_launch_rotation(c, a);
}
int thfhe_mk_prologue_dev(thfhe_mk_ctx *c, int op, int which, const int32_t *d0, const int32_t *d1, const int32_t *d2, int rec_words,
                          int first_word, int32_t *d_bara, int32_t *d_barb, size_t count) {
    if (!c || !d0 || !d_bara || !d_barb) return thfhe_fail(THFHE_E_INVALID, "null argument");
    if (count == 0) return THFHE_OK;
    MKLin L;
    if (op == -1) op = kOpIdentity;  // plain bootstrap of in0
    if (!mk_gate_lin(op, which, L)) return thfhe_fail(THFHE_E_INVALID, "gate not defined for the 3-gen multi-key scheme");
    if ((L.cy != 0 && !d1) || (L.cz != 0 && !d2)) return thfhe_fail(THFHE_E_INVALID, "null operand");
    const int nw = c->words;  // this context's parties are contiguous in the record: parties * n mask words
    if (first_word < 0 || first_word + nw > rec_words - 1) return thfhe_fail(THFHE_E_INVALID, "party slice outside the record");
    DevLock lk(*c);
    if (lk.rc) return lk.rc;
    const dim3 grid((unsigned)((nw + 1 + 255) / 256), (unsigned)count);
    hipLaunchKernelGGL(mk_prologue_slice_kernel, grid, dim3(256), 0, c->stream, d0, d1, d2, L, rec_words, first_word, nw, c->log2_2n, (long)count, d_bara, d_barb);
    THFHE_HIP(hipGetLastError());
    return THFHE_OK;
}
#ifdef THFHE_STAMPS
int thfhe_debug_read_stamps_mk(unsigned long long *dst, size_t count) {
    return hipMemcpyFromSymbol(dst, HIP_SYMBOL(g_stamps), count * sizeof(unsigned long long)) == hipSuccess ? 0 : -1;
}
#endif
int thfhe_mk_set_pair_threshold(thfhe_mk_ctx *c, long max_single_jobs) {
    if (!c || max_single_jobs < 0) return thfhe_fail(THFHE_E_INVALID, "bad argument");
    std::lock_guard<std::mutex> g(c->mu);
    c->pair_threshold = max_single_jobs;
    return THFHE_OK;
}
int thfhe_mk_rotation_kernel_name(const thfhe_mk_ctx *c, size_t rotations, char *buf, int len) {
    if (!c || !buf) return thfhe_fail(THFHE_E_INVALID, "null argument");
    std::lock_guard<std::mutex> g(const_cast<thfhe_mk_ctx *>(c)->mu);   // the threshold is set under it
    return kernel_name_result(len, launch_plan::mk_kernel_name(c->p.N, c->p.l, c->parts, c->batched, (long)rotations, c->pair_threshold, buf, len > 0 ? (size_t)len : 0));
}
int thfhe_mk_set_stream(thfhe_mk_ctx *c, void *hip_stream) {
    if (!c) return thfhe_fail(THFHE_E_INVALID, "null ctx");
    std::lock_guard<std::mutex> g(c->mu);
    THFHE_HIP(hipStreamSynchronize(c->stream));
    c->stream = hip_stream ? (hipStream_t)hip_stream : c->own_stream;
    return THFHE_OK;
}
int thfhe_mk_extract_dev(thfhe_mk_ctx *c, const int64_t *d_acc, int32_t *d_u, size_t count) {
    if (!c || !d_acc || !d_u) return thfhe_fail(THFHE_E_INVALID, "null argument");
    if (count == 0) return THFHE_OK;
    DevLock lk(*c);
    if (lk.rc) return lk.rc;
    hipLaunchKernelGGL(mk_extract_kernel, dim3((unsigned)count), dim3(256), 0, c->stream, d_acc, d_u, (long)count, c->p.N);
    THFHE_HIP(hipGetLastError());
    return THFHE_OK;
}
int thfhe_mk_keyswitch_dev(thfhe_mk_ctx *c, const int32_t *d_u, int32_t *d_out, size_t count) {
    if (!c || !d_u || !d_out) return thfhe_fail(THFHE_E_INVALID, "null argument");
    if (count == 0) return THFHE_OK;
    DevLock lk(*c);
    if (lk.rc) return lk.rc;
    return mk_keyswitch(c, d_u, d_out, count);
}

int thfhe_mk_bootstrap(thfhe_mk_ctx *c, int64_t mu, const int32_t *x, int32_t *out, size_t count) {
    if (!c || !x || !out) return thfhe_fail(THFHE_E_INVALID, "null argument");
    if (count == 0) return THFHE_OK;
    const size_t words = count * c->rec_words(), bytes = words * sizeof(int32_t);
    MKLin L;
    mk_gate_lin(kOpIdentity, 0, L);
    return ctx_staged(c, words, {x, nullptr, nullptr}, {bytes, 0, 0}, [&] {
        int rc = mk_ensure_workspace(c, count);
        return rc ? rc : mk_enqueue_bootstraps(c, c->stage.in_ptr(0), c->stage.in_ptr(0), c->stage.in_ptr(0), L, L, 1, count, mu, c->stage.out_ptr());
    }, c->stage.out, out, bytes);
}

int thfhe_mk_lut_bootstrap(thfhe_mk_ctx *c, const thfhe_lut_spec *spec, const int64_t *tv, int n_luts, const int32_t *lut_index, const int32_t *in0,
                           const int32_t *in1, const int32_t *in2, int32_t *out, size_t count) {
    return mk_lut_bootstrap(c, spec, tv, n_luts, lut_index, in0, in1, in2, out, count, true);
}

int thfhe_mk_lut_bootstrap_wo_keyswitch(thfhe_mk_ctx *c, const thfhe_lut_spec *spec, const int64_t *tv, int n_luts, const int32_t *lut_index,
                                        const int32_t *in0, const int32_t *in1, const int32_t *in2, int32_t *out_N1, size_t count) {
    return mk_lut_bootstrap(c, spec, tv, n_luts, lut_index, in0, in1, in2, out_N1, count, false);
}

int thfhe_mk_lut_bootstrap_enc(thfhe_mk_ctx *c, const thfhe_lut_spec *spec, const int64_t *tv_a, const int64_t *tv_b, int n_luts, const int32_t *lut_index,
                               const int32_t *in0, const int32_t *in1, const int32_t *in2, int32_t *out, size_t count) {
    return mk_lut_bootstrap(c, spec, tv_b, n_luts, lut_index, in0, in1, in2, out, count, true, true, tv_a);
}

int thfhe_mk_lut_bootstrap_enc_wo_keyswitch(thfhe_mk_ctx *c, const thfhe_lut_spec *spec, const int64_t *tv_a, const int64_t *tv_b, int n_luts,
                                            const int32_t *lut_index, const int32_t *in0, const int32_t *in1, const int32_t *in2, int32_t *out,
                                            size_t count) {
    return mk_lut_bootstrap(c, spec, tv_b, n_luts, lut_index, in0, in1, in2, out, count, false, true, tv_a);
}

int thfhe_mk_pack_key_set(thfhe_mk_ctx *c, const int64_t *pk, int D, int t, int basebit) {
    if (!pk) return thfhe_fail(THFHE_E_INVALID, "null argument");
    if (basebit < 1 || basebit > 4 || t < 1 || t * basebit > 32) return thfhe_fail(THFHE_E_INVALID, "pack key: need 1 <= basebit <= 4, t >= 1, t * basebit <= 32");
    if (!c) return thfhe_fail(THFHE_E_INVALID, "null ctx");
    DevLock lk(*c);
    if (lk.rc) return lk.rc;
    if (D != c->p.N && D != c->words) return thfhe_fail(THFHE_E_INVALID, "pack key: D must be the ring degree N or the record's P * n mask words");
    const size_t bytes = (size_t)D * t * ((1u << basebit) - 1) * 2 * c->p.N * sizeof(int64_t);
    THFHE_HIP(hipStreamSynchronize(c->stream));   // nothing reads the key it replaces
    c->pk_D = 0;
    THFHE_TRY(c->d_pk.grow(bytes));
    THFHE_HIP(hipMemcpyAsync(c->d_pk.as<int64_t>(), pk, bytes, hipMemcpyHostToDevice, c->stream));
    THFHE_HIP(hipStreamSynchronize(c->stream));
    c->pk_D = D, c->pk_t = t, c->pk_basebit = basebit;
    return THFHE_OK;
}

int thfhe_mk_pack_boxes(thfhe_mk_ctx *c, const int32_t *recs, size_t count, int p, int64_t *tv_a, int64_t *tv_b) {
    return mk_pack_boxes(c, recs, count, p, tv_a, tv_b);
}

int thfhe_mk_tree_lut_bootstrap(thfhe_mk_ctx *c, const thfhe_lut_spec *spec_lo, const thfhe_lut_spec *spec_hi, int p_hi, const int64_t *tv1, int n_tables,
                                const int32_t *table_index, const int32_t *lo0, const int32_t *lo1, const int32_t *lo2, const int32_t *hi0,
                                const int32_t *hi1, const int32_t *hi2, int32_t *out, size_t count) {
    // host checks, before the context is looked at
    THFHE_TRY(tree_validate_rows(kMkTreeRules, spec_lo, spec_hi, p_hi, tv1, n_tables, table_index, lo0, lo1, lo2, hi0, hi1, hi2, out, count));
    return mk_tree_bootstrap(c, *spec_lo, *spec_hi, p_hi, tv1, (size_t)n_tables * (p_hi / spec_lo->theta), nullptr, 0, 0, table_index, 0, lo0, lo1, lo2, hi0, hi1,
                             hi2, out, count);
}

int thfhe_mk_tree_lut_bootstrap_mvk(thfhe_mk_ctx *c, const thfhe_lut_spec *spec_lo, const thfhe_lut_spec *spec_hi, int p_hi, int p_lo, int k, const int64_t *tv0,
                                    const int32_t *factors, int n_tables, const int32_t *table_index, int64_t out_bias, const int32_t *lo0,
                                    const int32_t *lo1, const int32_t *lo2, const int32_t *hi0, const int32_t *hi1, const int32_t *hi2, int32_t *out,
                                    size_t count) {
    // host checks, before the context is looked at: those of thfhe_tree_lut_bootstrap_mvk
    THFHE_TRY(tree_validate(kMkTreeRules, spec_lo, spec_hi, p_hi, tv0, lo0, lo1, lo2, hi0, hi1, hi2, out));
    if (!factors) return thfhe_fail(THFHE_E_INVALID, "null argument");
    THFHE_TRY(mv_validate(*spec_lo, p_lo, p_hi, n_tables));
    THFHE_TRY(tree_validate_index(table_index, n_tables, count));
    THFHE_TRY(mvk_validate(p_hi, k));
    const int32_t *const ins[6] = {lo0, spec_lo->n_inputs > 1 ? lo1 : nullptr, spec_lo->n_inputs > 2 ? lo2 : nullptr, hi0, spec_hi->n_inputs > 1 ? hi1 : nullptr,
                                   spec_hi->n_inputs > 2 ? hi2 : nullptr};
    for (const int32_t *in : ins)
        if (in == out) return thfhe_fail(THFHE_E_INVALID, "tree: out must not alias an input");
    return mk_tree_bootstrap(c, *spec_lo, *spec_hi, p_hi, tv0, 1, factors, p_lo, n_tables, table_index, out_bias, lo0, lo1, lo2, hi0, hi1, hi2, out, count, k);
}

int thfhe_mk_set_pack_wide_threshold(thfhe_mk_ctx *c, size_t min_records) {
    if (!c) return thfhe_fail(THFHE_E_INVALID, "null ctx");
    std::lock_guard<std::mutex> g(c->mu);
    c->pack_wide_threshold = min_records;
    return THFHE_OK;
}

int thfhe_mk_pack_kernel_name(const thfhe_mk_ctx *c, size_t count, char *buf, int len) {
    if (!c || !buf) return thfhe_fail(THFHE_E_INVALID, "null argument");
    std::lock_guard<std::mutex> g(const_cast<thfhe_mk_ctx *>(c)->mu);   // the threshold is set under it
    return kernel_name_result(len, launch_plan::mk_pack_kernel_name(count, c->pack_wide_threshold, buf, len > 0 ? (size_t)len : 0));
}

int thfhe_mk_lwe_linear(thfhe_mk_ctx *c, const int32_t *W, const int32_t *bias, int M, int K, const int32_t *in, int32_t *out, size_t count) {
    return mk_linear(c, W, bias, M, K, false, 1, nullptr, 1, nullptr, in, out, count, false);
}

int thfhe_mk_linear_lut_bootstrap(thfhe_mk_ctx *c, const int32_t *W, const int32_t *bias, int M, int K, int theta, const int64_t *tv, int n_luts,
                                  const int32_t *lut_index, const int32_t *in, int32_t *out, size_t count) {
    return mk_linear(c, W, bias, M, K, true, theta, tv, n_luts, lut_index, in, out, count, true);
}

int thfhe_mk_linear_lut_bootstrap_wo_keyswitch(thfhe_mk_ctx *c, const int32_t *W, const int32_t *bias, int M, int K, int theta, const int64_t *tv, int n_luts,
                                               const int32_t *lut_index, const int32_t *in, int32_t *out_N1, size_t count) {
    return mk_linear(c, W, bias, M, K, true, theta, tv, n_luts, lut_index, in, out_N1, count, false);
}

int thfhe_mk_set_linear_slice(thfhe_mk_ctx *c, size_t jobs) { return ctx_set_linear_slice(c, jobs); }

int thfhe_mk_linear_last_timings(thfhe_mk_ctx *c, float ms[3]) { return ctx_linear_last_timings(c, ms); }

int thfhe_mk_set_tree_slice(thfhe_mk_ctx *c, size_t max_candidates) {
    if (!c || max_candidates < 1 || max_candidates > ((size_t)1 << 18)) return thfhe_fail(THFHE_E_INVALID, "slice must be 1 .. 2^18 candidates");
    std::lock_guard<std::mutex> g(c->mu);
    c->tree_slice = max_candidates;
    return THFHE_OK;
}

int thfhe_mk_tgsw_set_create(thfhe_mk_ctx *c, const int64_t *tgsw, size_t count, int d, thfhe_mk_tgsw_set **out) {
    return ctx_tgsw_set_create(c, tgsw, count, d, out, kMkLheRules, mk_tgsw_set_fill);
}

void thfhe_mk_tgsw_set_destroy(thfhe_mk_tgsw_set *set) { ctx_tgsw_set_destroy(set); }

int thfhe_mk_lhe_cmux(thfhe_mk_ctx *c, const thfhe_mk_tgsw_set *set, int bit, const int64_t *d1_a, const int64_t *d1_b, const int64_t *d0_a,
                      const int64_t *d0_b, int64_t *out_a, int64_t *out_b, size_t count) {
    return mk_lhe_cmux(c, set, bit, d1_a, d1_b, d0_a, d0_b, out_a, out_b, count);
}

int thfhe_mk_lhe_lookup(thfhe_mk_ctx *c, const thfhe_mk_tgsw_set *set, size_t first, size_t count, int d_tree, int d_rot, int theta, const int64_t *tab_a,
                        const int64_t *tab_b, int n_tables, const int32_t *table_index, int32_t *out) {
    return mk_lhe_lookup(c, set, first, count, d_tree, d_rot, theta, tab_a, tab_b, n_tables, table_index, out, true);
}

int thfhe_mk_lhe_lookup_wo_keyswitch(thfhe_mk_ctx *c, const thfhe_mk_tgsw_set *set, size_t first, size_t count, int d_tree, int d_rot, int theta,
                                     const int64_t *tab_a, const int64_t *tab_b, int n_tables, const int32_t *table_index, int32_t *out_N1) {
    return mk_lhe_lookup(c, set, first, count, d_tree, d_rot, theta, tab_a, tab_b, n_tables, table_index, out_N1, false);
}

int thfhe_mk_mv_lut_bootstrap(thfhe_mk_ctx *c, const thfhe_lut_spec *spec, const int64_t *tv0, const int32_t *factors, int p, int q, int n_tables,
                              const int32_t *table_index, int64_t out_bias, const int32_t *in0, const int32_t *in1, const int32_t *in2, int32_t *out,
                              size_t count) {
    return mk_mv_lut_bootstrap(c, spec, tv0, factors, p, q, n_tables, table_index, out_bias, in0, in1, in2, out, count, true);
}

int thfhe_mk_mv_lut_bootstrap_wo_keyswitch(thfhe_mk_ctx *c, const thfhe_lut_spec *spec, const int64_t *tv0, const int32_t *factors, int p, int q,
                                           int n_tables, const int32_t *table_index, int64_t out_bias, const int32_t *in0, const int32_t *in1,
                                           const int32_t *in2, int32_t *out_N1, size_t count) {
    return mk_mv_lut_bootstrap(c, spec, tv0, factors, p, q, n_tables, table_index, out_bias, in0, in1, in2, out_N1, count, false);
}

}  // extern "C"
