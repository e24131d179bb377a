// thfhe_sk.hip -- single-key (Torus32) gate bootstrapping on gfx950: kernels + C ABI.
//
// Kernels (one HIP stream per context, no host sync inside a call):
//   torus_transform_kernel    BootstrapKey forward_transform step (J/bootstrap.jl:11-12): coefficient-domain TGSW
//   (thfhe_transform.h)       rows -> two-limb FP64 spectra in the blind-rotate kernel's register order
//   sk_prologue_kernel        gate linear part (J/gates.jl:15-177) + mod-switch decode_message(.,2N)
//                             (J/bootstrap.jl:80-81) -> bara[job][n], barb[job]
//   lut_prologue_kernel       programmable bootstrap (thfhe_lut_bootstrap): weighted sum of 1-3 inputs + bias, mod-switch to multiples of theta
//   (thfhe_lut_prologue.h,    (DESIGN 4.7); one kernel for every PBS front half, instantiated on where a job's operands live: contiguous arrays
//   shared with thfhe_mk.hip) (the flat calls, both levels of thfhe_tree_lut_bootstrap) or the gate DAG's wire table (LUT, LUT_ENC,
//                             SELECT and TREE nodes; dag_select_gather_kernel in thfhe_dag.h collects a SELECT's candidates).
//                             The blind-rotate kernels' LUT instantiations start from a test vector and extract theta coefficients
//   sk_blind_rotate_ring_kernel / sk_blind_rotate_coop_kernel   blind_rotate_and_extract (J/bootstrap.jl:38-65): accumulator in
//                             LDS for all n CMuxes; throughput (8 gates per workgroup, key through an LDS-DMA ring) and latency
//                             (one workgroup per gate) kernels; each is built in one form only, the forms that were measured against
//                             them and lost are written up in profiles/r03_ring_variants.md and r04_ring_multiply_phase.md
//   ks_plain_kernel / ks_staged_kernel / sk_keyswitch_mfma_kernel   keyswitch (J/keyswitch.jl:45-80) (+ the MUX combine of J/gates.jl:172-176),
//   (thfhe_keyswitch.h, shared with the multi-key engines): one gate per workgroup (small batches); from 192 gates on the rows of a few
//                             (i, j) staged in LDS for 32 gates, the digit selecting an address; from 512 gates on an int8 GEMM on the matrix cores
//   sk_linear_kernel          NOT / COPY (J/gates.jl:76-79)
//   lwe_linear_kernel         dense layer (thfhe_lwe_linear, thfhe_linear_lut_bootstrap): integer matrix x LWE vector mod 2^32, the sums
//   (thfhe_linear.h, shared   staying on the device for the PBS of the same call
//   with thfhe_mk.hip)
//                             ; on the wire-table source (LinWireSrc) the DENSE nodes of the gate DAG (thfhe_dag_run_dense_batch),
//                             with dense_lut_idx_kernel for a group's per-job table indices
#include <hip/hip_runtime.h>

#include <algorithm>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "../../include/thfhe_hip.h"
#include "thfhe_cb.h"
#include "thfhe_common.h"
#include "thfhe_dag.h"
#include "thfhe_devctx.h"
#include "thfhe_keyswitch.h"
#include "thfhe_lane.h"
#include "thfhe_launch_plan.h"
#include "thfhe_pack.h"
#include "thfhe_pbs_host.h"
#include "thfhe_lhe_host.h"   // builds on thfhe_pbs_host.h
#include "thfhe_ring_schedule.h"

using namespace thfhe;

namespace {

#include "thfhe_transform.h"

// ------------------------------------------------------------------------------------------------------
// prologue: tmp = (0, cb) + cx * x + cy * y ; bara = decode_message(tmp.a, 2N) ; barb likewise
// ------------------------------------------------------------------------------------------------------
struct Lin {
    int32_t cb, cx, cy;
    int ysel;  // 1: second operand is in1, 2: in2
};
__host__ __device__ inline bool gate_lin(int op, int which, Lin &L) {
    const int32_t E8 = 1 << 29, E4 = 1 << 30;  // encode_message(1,8), (1,4)   J/numeric-functions.jl:86-89
    switch (op) {
    case THFHE_NAND: L = Lin{E8, -1, -1, 1}; return true;
    case THFHE_OR: L = Lin{E8, 1, 1, 1}; return true;
    case THFHE_AND: L = Lin{-E8, 1, 1, 1}; return true;
    case THFHE_XOR: L = Lin{E4, 2, 2, 1}; return true;
    case THFHE_XNOR: L = Lin{-E4, -2, -2, 1}; return true;
    case THFHE_NOR: L = Lin{-E8, -1, -1, 1}; return true;
    case THFHE_ANDNY: L = Lin{-E8, -1, 1, 1}; return true;
    case THFHE_ANDYN: L = Lin{-E8, 1, -1, 1}; return true;
    case THFHE_ORNY: L = Lin{E8, -1, 1, 1}; return true;
    case THFHE_ORYN: L = Lin{E8, 1, -1, 1}; return true;
    case THFHE_MUX: L = which == 0 ? Lin{-E8, 1, 1, 1} : Lin{-E8, -1, 1, 2}; return true;  // J/gates.jl:166-171
    case kOpIdentity: L = Lin{0, 1, 0, 1}; return true;                                      // plain bootstrap(x)
    default: return false;
    }
}

__global__ __launch_bounds__(256) void sk_prologue_kernel(const int32_t *__restrict__ in0, const int32_t *__restrict__ in1,
                                                           const int32_t *__restrict__ in2, int op, const int32_t *__restrict__ ops,
                                                           int rot_per_gate, int n, int n_pad, int log2_2n, long jobs,
                                                           int32_t *__restrict__ bara, int32_t *__restrict__ barb) {
    const long job = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (job >= jobs || i > n) return;
    const long gate = job / rot_per_gate;
    const int which = (int)(job % rot_per_gate);
    Lin L;
    gate_lin(ops ? ops[gate] : op, which, L);  // ops: per-gate opcodes of a mixed level (validated on the host)
    const size_t off = (size_t)gate * (n + 1) + i;
    uint32_t v = (uint32_t)L.cx * (uint32_t)in0[off];
    if (L.cy != 0) v += (uint32_t)L.cy * (uint32_t)(L.ysel == 2 ? in2[off] : in1[off]);
    if (i == n) {
        v += (uint32_t)L.cb;
        barb[job] = modswitch2n((int32_t)v, log2_2n);
    } else {
        bara[job * n_pad + i] = modswitch2n((int32_t)v, log2_2n);
    }
}

THFHE_STAMP_STORAGE

// arguments of the blind-rotate kernels
struct BRArgs {
    const cplx *bk;        // spectral key (the cooperative kernel)
    const cplx *bk_ring;   // its phased copy (thfhe_ctx::d_bk_ring): what the ring kernels stream
    const cplx *tw;        // T1[512] ++ T2[64]
    const int32_t *bara;   // [jobs][n_pad]
    const int32_t *barb;   // [jobs]
    int32_t *out;          // [jobs][N+1]; LUT kernels: [jobs][theta][N+1]; kLutMv: [jobs][q][N+1]
    long jobs;
    int n, n_pad, Bgbit;
    int32_t mu;
    // LUT kernels only (programmable bootstrap): accumulator X^{-barb} * tv, coefficients 0 .. theta-1 extracted
    const int32_t *tv;       // [n_luts][N]
    const int32_t *lut_idx;  // [jobs] test vector of each job, or null: table 0
    int theta;               // records per job: 1, 2 or 4 coefficients extracted; kLutMv: its q outputs, 1 .. 64
    // encrypted-table kernels only (LUT == kLutEnc): the tables are TLWE samples (tv_a, tv) under the ring key, accumulator X^{-barb} * (tv_a, tv)
    const int32_t *tv_a;     // [n_luts][N] masks; `tv` holds the bodies
    // multi-value kernels only (LUT == kLutMv): every job rotates tv[0 .. N); lut_idx picks its table of `theta` factors of mv_p taps
    const int32_t *mv_w;     // [n_tables][theta][mv_p] taps; written before the launch, read as wave-uniform scalars
    int mv_p, mv_box;        // taps per output (a power of two, 2 .. 64) and N / mv_p
};

// what a blind-rotate instantiation starts from: the gates' constant test vector, a plaintext table, an encrypted table (4.11);
// kLutMv starts like kLut, from the one base vector of a multi-value bootstrap, and ends in extract_mv16 (4.13)
constexpr int kGate = 0, kLut = 1, kLutEnc = 2, kLutMv = 3;

// ------------------------------------------------------------------------------------------------------
// blind rotate + extract, throughput kernel ("LDS ring", second generation).
//
// One 512-thread workgroup = 8 wavefronts = 8 jobs, one workgroup per CU, all 160 KiB of LDS:
//     8 x (accumulator int32[2][1024] 8 KiB + transpose buffer 9 KiB) | key ring 3 x 8 KiB                  = 163 840 B
// Each wave owns one job; its accumulator never leaves LDS during the n CMuxes.  The eight waves walk the key index i, the digit
// rows and the four (column, limb) chunks of a row in lock step.  A chunk is 8 KiB of key spectrum = 8 slices of 1 KiB; wave w brings
// slice w into its slot with ONE global_load_lds_dwordx4 (LDS-DMA, no registers), so the whole key crosses the CU's vector-memory
// path once per workgroup instead of once per wave.
//
// Hand-off per ROW (thfhe_ring_schedule.h holds the slot schedule; tests/cpp/ring_schedule_test.cpp replays it on the host).  The transpose
// buffers are touched only inside transforms, and between the first and the last barrier of a row no wave is inside one: the first 8 KiB of
// transpose buffer 0 are a fourth slot for that time.  With c0 .. c3 the row's chunks (column, limb) = (0,0), (0,1), (1,0), (1,1), and a
// hand-off = s_waitcnt vmcnt(N) lgkmcnt(0) (own slices landed, N = younger DMAs in flight; own LDS reads returned) + s_barrier:
//   A  after the forward transform: c0 c1 c2 are complete in ring slots 0 1 2 (issued at X of the row before, or by the prologue) and
//      everybody is out of the transform -> DMA c3 into the borrowed slot; c0 c1 c2 consumed back to back, no barrier between them
//   X  c3 is complete, everybody's reads of c0 .. c2 have returned -> DMA the NEXT row's c0 c1 c2 into slots 0 1 2 (they land under the rest
//      of this row and the next transform; the next row may be the next CMux's); c3 consumed from the borrowed slot
//   B  everybody's reads of the borrowed slot have returned (c3's second half sits in registers) -> transpose buffer 0 is wave 0's again
// Per row: 3 barriers, 4 DMA issues per wave (the per-chunk hand-off this replaces: 5 barriers); a wave still issues the key in linear order.
// A wave whose mod-switched mask word is 0 (J/bootstrap.jl:40) or that has no job still streams and synchronises.  Measured
// (profiles/r09_handoff_timing.md): what the barriers cost was skew between the two waves of a SIMD, not the multiply phase itself.
//
// What the kernel does about its bounds.  An in-kernel cycle trace and the PMC counters of the first generation (tools/ring_stamps.py,
// profiles/r02_ring_generations.md) showed it, at two waves per SIMD, bound by exposed LDS round trips and by the LDS instruction pipe (69 % busy,
// bursts in lock step) with the VALU 55 % busy; since then the time is the FP64 instruction stream (an FP64 wave instruction holds the SIMD's
// vector pipe for 4 cycles).  Per 4096 gates 34.8 -> 33.3 -> 29.9 -> 28.7 -> 27.70 ms; the forms that were tried and lost are in
// profiles/r03_ring_variants.md and r04_ring_multiply_phase.md.
//   * the FIRST transpose of every transform (register index <-> lane bits 3..5) stays in registers: v_permlane32_swap, v_permlane16_swap and
//     row_ror:8 DPP moves instead of 8 ds_write_b128 + 8 ds_read_b128.  It is the exchange of variant "x" (wave_transpose_x3; thfhe_lane.h): lane
//     bit 3 trades with register bit 2, the pairs (r, r + 4) that a pass writes last and reads first.  In the inverse transforms that stage is 16
//     unmasked moves: the lanes with bit 3 set name those pairs the other way round, which a negated per-lane root produces and conj(W^4), a
//     signed and rescaled untwist constant consume -- 24 instructions fewer per transform than two masked moves and a kept 64-bit copy per
//     double.  1 311 -> 1 223 other vector instructions per CMux and wave, 27.74 -> 27.33 ms per 4096 gates (profiles/r11_exchange.md).  The
//     FORWARD transforms take the same 16 moves (variant "p"): the flipped names come from a negated pass-1 root (one signed constant pair and
//     four sign XORs) and are consumed by conj(W^4) in pass 2's first stage (one XOR), which leaves rho^(-32) on the spectra of the lanes with
//     bit 3 set.  No folded pass can take that scalar out; the KEY does: this kernel streams a.bk_ring, a second spectral array of the context
//     that holds the spectrum of X^32 b at exactly those points (bit 5 of nu) and the plain value elsewhere -- an exact negacyclic rotation of
//     the integer limb polynomials, made by the key transform at context creation (thfhe_transform.h: MapPhased).  Every product is what it
//     was; the inverse and the accumulator see no difference; the cooperative kernel keeps the plain array.  A lane stands for the natural
//     position nu = lane_nu(lane) throughout: digit reads, key reads, roots and the accumulator update take nu; the key's order in memory and
//     in the ring is untouched.  1 223 -> 1 109 other vector instructions (profiles/r12_phased_key.md);
//   * the inverse's outputs m + 4 leave their scale R = 1/sqrt 2 (of conj(C[4])) to the rounding add of the accumulator update: one
//     fma(R, x, 1.5 * 2^52) per component instead of a multiply and an add (invx_seg3_ring / acc_update16_ring): 3 356 -> 3 324 FP64 instructions;
//   * the second transpose uses the padded 576-slot buffer (there is no T1 table in the LDS, its 8 KiB pay for the padding): its slot maps are
//     base + immediate, 2 LDS address registers per wave instead of 16 for XOR-swizzled maps;
//   * no twiddle is read from a table: the transforms are variant "f" (thfhe_lane.h).  Every inter-pass twiddle sits on the input side of the pass
//     that follows it and is folded into that pass's radix-2 butterflies (a + W b as two dependent FMAs per component, a - W b = 2 a - x as one), a
//     twiddled DFT8 = 72 FP64 instructions from four constants per root.  Forward: the twist C[m] rides in pass 1 (wave-uniform constants), pass 2
//     and pass 3 take one per-lane root each (TwRing1k::ROOTSF); inverse: the two conjugate per-lane roots of TwRing1k::ROOTS, the untwist stays a
//     product.  Per CMux and wave 3 356 FP64 instructions (forward transform 240), no scratch within the 256 VGPRs of two waves per SIMD: the roots are made opaque IN PLACE per
//     transform (no register copies), so their powers are rebuilt and not kept across the CMux loop; only the four untwist constants are shared by a
//     CMux's inverse transforms.  Sharing one or both roots' powers as well (3 320 / 3 284 instructions) spilled 6 / 15 registers around the inverse
//     phase and measured 0.45 ms SLOWER than this form (profiles/r06_fold_static_counts.md);
//   * rotate + decompose in one step on byte offsets (thfhe_lane.h: rotated_word / mixed_digits_z), the index / sign / subtraction work once per
//     accumulator polynomial (fields kept across its l levels), a level = one v_bfe_i32 + one conversion per coefficient;
//   * the multiply-accumulate is software-pipelined over half chunks: the four ring reads of one half are in flight under the 16 FMAs of the half
//     before, S += z * b is four FMAs, and the multiply negates the key operand, not z.im (cfma_negkey in thfhe_lane.h): the compiler had carried a
//     negated copy of every z.im through the row;
//   * the key-stream cursor is scalar (below; ring_dma in thfhe_common.h).
// The scalar cursor, KEEP64 and cfma_negkey took the other (non-FP64) third of the vector stream from 1 545 to 1 311 instructions per CMux and wave
// (28.26 -> 27.70 ms; profiles/r10_valu_diet.md).
// ------------------------------------------------------------------------------------------------------
// W = waves (= jobs) per workgroup.  W = 8 is the throughput shape described above.  W = 4 (one wave per SIMD, 92 KiB of LDS, each wave
// brings TWO slices of a chunk) is the shape for batches that cannot give every CU eight jobs (<= 1024 rotations): a wave alone on its
// SIMD issues at ~87 % of what a pair reaches together (tools/probes/issue_probe.hip), so four jobs finish much sooner than eight.
// LUT = kLut, kLutEnc: programmable bootstrap, the accumulator starts from a test vector (kLutEnc: from a TLWE sample, mask included) and theta
// coefficients are extracted; kLutMv: multi-value bootstrap, the kLut start on one base vector and a.theta = q outputs, each a
// p-tap combination of extractions (extract_mv16); the CMux loop is the same code.
template <int L, int W = 8, int LUT = kGate>
__global__ __launch_bounds__(64 * W, W == 8 ? 2 : 1) void sk_blind_rotate_ring_kernel(BRArgs a) {
    __shared__ __attribute__((aligned(4096))) int32_t sAcc[W][2048];   // rotated_digits_z ORs byte offsets into the polynomial base
    __shared__ cplx sX[W][kXbufSlots];
    __shared__ cplx sRing[3][512];
    constexpr int ROWS = 2 * L;
    constexpr int DPC = 8 / W;   // ring DMAs per wave and chunk
    namespace RS = ring_schedule;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    // the roots are variables: opaque_in_place makes them loop-carried in the registers they already occupy
    // variant "x" (thfhe_lane.h): past the forward exchange the lane stands for the natural position nu; the lanes with bit 3 set carry the flipped names
    const int nu = lane_nu(lane);
    const uint32_t flip = lane_flip_x(lane);
    W64 w64 = lane_w64_x(a.tw[TwRing1k::T2 + 1 * 8 + (lane & 7)], flip);                        // inverse transforms
    LaneRoots roots = lane_roots_x(a.tw, TwRing1k::T1, TwRing1k::ROOTS, lane);
    LaneRootsF rootsf{a.tw[TwRing1k::ROOTSF + 2 * nu], a.tw[TwRing1k::ROOTSF + 2 * nu + 1]};   // forward transforms
    const long job = (long)blockIdx.x * W + wave;
    const bool has_job = job < a.jobs;
    int32_t *acc = sAcc[wave];
    cplx *xb = sX[wave];
    const uniform_i32_ptr bara = as_uniform(a.bara + (has_job ? job : 0) * a.n_pad);   // job is wave-uniform: scalar loads
    const int Bgbit = a.Bgbit;
    if (has_job) {
        if constexpr (LUT == kLutEnc) {
            const size_t t = a.lut_idx ? (size_t)a.lut_idx[job] * 1024 : 0;
            acc_init_tlwe16(lane, acc, acc + 1024, a.barb[job], a.tv_a + t, a.tv + t);
        } else if constexpr (LUT == kLutMv) acc_init_tv16(lane, acc, acc + 1024, a.barb[job], a.tv);
        else if constexpr (LUT) acc_init_tv16(lane, acc, acc + 1024, a.barb[job], a.tv + (a.lut_idx ? (size_t)a.lut_idx[job] * 1024 : 0));
        else acc_init16(lane, acc, acc + 1024, a.barb[job], a.mu);
    }

    // The key-stream cursor is wave-uniform and lives in SGPRs: the stream position as a 64-bit base, the count of chunks still ahead of it; the only
    // per-lane part of a DMA's address is one loop-invariant 32-bit byte offset.  An issue costs the vector pipe nothing but the DMA itself.
    static_assert(DPC == 1 || DPC == 2, "a wave brings one slice of a chunk, or two 1 KiB apart");
    const uint32_t lane_off = (uint32_t)(wave * (64 * DPC) + lane) * (uint32_t)sizeof(cplx);
    uint64_t gbase = (uint64_t)(size_t)a.bk_ring;
    int chunks_ahead = a.n * ROWS * RS::kChunksPerRow - 1;   // issues past the end of the stream repeat its last chunk
    asm volatile("" : "+s"(gbase), "+s"(chunks_ahead));
    // slots 0 .. 2 are the key ring, slot 3 is borrowed from transpose buffer 0 between barriers A and B of a row (thfhe_ring_schedule.h)
    static_assert(RS::kResidentSlots * RS::kSlotBytes == sizeof(sRing) && RS::kSlotBytes <= sizeof(sX[0]), "ring schedule against the LDS layout");
    const uint32_t ring_base = (uint32_t)(size_t)(__attribute__((address_space(3))) void *)&sRing[0][0] + (uint32_t)wave * (1024u * DPC);
    const uint32_t lent_base = (uint32_t)(size_t)(__attribute__((address_space(3))) void *)&sX[0][0] + (uint32_t)wave * (1024u * DPC);
    auto issue = [&](int slot) {
        const uint32_t dst = slot == RS::kBorrowedSlot ? lent_base : ring_base + (uint32_t)slot * (uint32_t)RS::kSlotBytes;
        ring_dma(gbase, lane_off, dst);
        if constexpr (DPC == 2) ring_dma<1024>(gbase, lane_off, dst);   // + 1 KiB in the key and in the slot
        gbase += chunks_ahead > 0 ? (uint32_t)RS::kSlotBytes : 0u;   // scalar compare, select, add with carry
        chunks_ahead = chunks_ahead > 0 ? chunks_ahead - 1 : 0;
    };
    auto slot_ptr = [&](int slot) -> const cplx * { return slot == RS::kBorrowedSlot ? &sX[0][0] : &sRing[slot][0]; };
    __syncthreads();
#pragma unroll
    for (int k = 0; k < RS::kPrologueIssues; k++) issue(RS::kPlan[k].slot);
    STAMP_DECL;

    for (int i = 0; i < a.n; i++) {
        const int ai = bara[i];
        const bool active = has_job && ai != 0;
        const int a2n = ai & 2047;
        cplx S[2][2][8];
#pragma unroll
        for (int c = 0; c < 2; c++)
#pragma unroll
            for (int h = 0; h < 2; h++)
#pragma unroll
                for (int m = 0; m < 8; m++) S[c][h][m] = cplx{0.0, 0.0};
        constexpr int NF = 16;   // rotated fields kept across the levels of a polynomial (register budget)
        uint32_t fld[NF];
#pragma unroll
        for (int r = 0; r < ROWS; r++) {
            cplx z[8];
            if (active) {
                // index / sign / subtraction once per accumulator polynomial, then one signed bit-field extract + one conversion per level
                int a2n_r = a2n;
                asm volatile("" : "+s"(a2n_r));  // opaque per row: the rotated LDS addresses are recomputed, not kept alive
                if (r % L == 0) rotated_fields_keep<NF, W == 4>(nu, acc + (r / L) * 1024, a2n_r, L, Bgbit, fld);
                asm volatile("" : "+s"(a2n_r));
                mixed_digits_z<NF>(nu, acc + (r / L) * 1024, a2n_r, (r % L) + 1, L, Bgbit, fld, z);
                // eight-wave shape: the two forward roots are made opaque per transform, so their powers (12 FP64 instructions each) are rebuilt and
                // not hoisted out of the CMux loop.  With nothing derived from the roots live across the loop the compiler parks nothing in scratch: no
                // reload in front of a row's digits waits for the ring DMAs (s_waitcnt vmcnt(0) follows every reload).  Rebuilding instead of keeping
                // measured 30.21 -> 29.97 ms per 4096 gates, 44 -> 0 B of scratch per lane, when it was introduced (on the transforms before these;
                // DESIGN 4.1, profiles/r04_summary.md).  The four-wave shape has registers to spare and lets the compiler keep what it likes.
                if (W == 8) opaque_in_place(rootsf.s), opaque_in_place(rootsf.w);
                wave_fft_fwd_x(lane, z, xb, rootsf, flip);
            }
            STAMP(0);
            cplx bA[4], bB[4];
            // one chunk: its first half is read, the second half of the chunk before multiplied under those reads, its second half read, its first
            // half multiplied -- the same software pipeline whether or not a barrier stands between two chunks
            auto consume = [&](int c4) {
                const cplx *B = slot_ptr(RS::kPlan[c4].slot);
                if (active) {
#pragma unroll
                    for (int m = 0; m < 4; m++) bA[m] = B[m * 64 + nu];
                    if (c4 > 0) {
#pragma unroll
                        for (int m = 0; m < 4; m++) cfma_negkey(S[(c4 - 1) >> 1][(c4 - 1) & 1][4 + m], z[4 + m], bB[m]);
                    }
#pragma unroll
                    for (int m = 0; m < 4; m++) bB[m] = B[(4 + m) * 64 + nu];
#pragma unroll
                    for (int m = 0; m < 4; m++) cfma_negkey(S[c4 >> 1][c4 & 1][m], z[m], bA[m]);
                }
            };
            // barrier A: c0 c1 c2 have landed and no wave is inside a transform -> c3 into the borrowed slot, c0 c1 c2 consumed back to back
            ring_barrier<RS::vmcnt_at(RS::kBarA) * DPC>();
            STAMP(1);
#pragma unroll
            for (int k = 0; k < RS::issues_at(RS::kBarA); k++) issue(RS::issue_slot(RS::kBarA, k));
#pragma unroll
            for (int c4 = RS::first_consumed(RS::kBarA); c4 < RS::first_consumed(RS::kBarX); c4++) consume(c4);
            STAMP(2);
            // barrier X: c3 has landed and everybody's reads of c0 c1 c2 have returned -> the next row's c0 c1 c2 into the ring, c3 consumed
            ring_barrier<RS::vmcnt_at(RS::kBarX) * DPC>();
            STAMP(1);
#pragma unroll
            for (int k = 0; k < RS::issues_at(RS::kBarX); k++) issue(RS::issue_slot(RS::kBarX, k));
#pragma unroll
            for (int c4 = RS::first_consumed(RS::kBarX); c4 < RS::first_consumed(RS::kBarB); c4++) consume(c4);
            STAMP(2);
            // barrier B: everybody's reads of the borrowed slot have returned (c3's second half sits in bB) -> transpose buffer 0 is wave 0's again
            ring_barrier<RS::vmcnt_at(RS::kBarB) * DPC>();
            static_assert(RS::issues_at(RS::kBarB) == 0 && RS::first_consumed(RS::kBarB) == RS::kChunksPerRow, "nothing is issued or read after barrier B");
            STAMP(1);
            if (active) {
#pragma unroll
                for (int m = 0; m < 4; m++) cfma_negkey(S[1][1][4 + m], z[4 + m], bB[m]);
            }
            STAMP(2);
        }
        if (active) {
            wave_sync();
            // the untwist constants b C[m] are built once per CMux for the four inverse transforms, from a root made opaque here so that they are not
            // kept across the multiply phase
            cplx bc[4];
            if (W == 8) opaque_in_place(roots.b);
            make_untwist_x(roots.b, flip, bc);
#pragma unroll
            for (int c = 0; c < 2; c++) {
                wave_fft_inv_x<W == 8>(lane, S[c][0], xb, w64, roots, flip, bc);
                wave_fft_inv_x<W == 8>(lane, S[c][1], xb, w64, roots, flip, bc);
                acc_update16_ring(nu, acc + c * 1024, S[c][0], S[c][1]);
            }
            wave_sync();
        }
        STAMP(3);
    }
    STAMP_FLUSH(blockIdx.x, wave);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (has_job) {
        if constexpr (LUT == kLutMv) {
            // the job's factor table: job is wave-uniform, so the index and every tap are scalar loads
            const uniform_i32_ptr w = as_uniform(a.mv_w) + (size_t)(a.lut_idx ? as_uniform(a.lut_idx)[job] : 0) * a.theta * a.mv_p;
            for (int j = 0; j < a.theta; j++) extract_mv16(lane, acc, acc + 1024, w + j * a.mv_p, a.mv_p, a.mv_box, a.out + (job * a.theta + j) * 1025);
        } else if constexpr (LUT) {
            for (int j = 0; j < a.theta; j++) extract_at16(lane, acc, acc + 1024, j, a.out + (job * a.theta + j) * 1025);
        } else {
            extract16(lane, acc, acc + 1024, a.out + job * 1025);
        }
    }
}

// ------------------------------------------------------------------------------------------------------
// blind rotate + extract, latency kernel ("cooperative", second generation): one 512-thread workgroup = ONE job.  For the small
// batches the reference's gate-at-a-time callers produce (boots* shims, ripple-carry circuits: 855 of the 1 033 levels of the KNN
// decision hold 1-3 gates) the ring kernel leaves 7/8 of a CU idle; here the work of one CMux is spread over the eight waves and
// the n CMuxes are a dependent chain, so what counts is the length of one step's critical path:
//   F  waves 0 .. 2l-1: wave r rotates / decomposes / transforms digit row r and publishes its spectrum in LDS;       barrier
//   M  wave w = (column c, limb h, half): S = sum over its half of the rows of spectrum_r * key(r, c, h) (key chunks in registers);
//      the waves of half 1 hand their partial sums to their partners through LDS;                                     barrier
//   I  waves 0-3 (one per SIMD) add the partner's partial sum, inverse-transform, and add round(S) << 16h into accumulator
//      polynomial c with 32-bit LDS atomics (two limbs per polynomial; integer adds commute -> bit-exact);            barrier
// The key stream is what the first generation tripped over: it requested the 24 chunks of a step (192 KiB per workgroup at l = 3)
// at the top of the step, in front of the forward transforms -- 192 wave-loads queue up on the CU's one vector-memory path
// (64 B/clk: ~3 k cycles) and a wave cannot start its transform before its own loads have been accepted.  A microbenchmark
// (tools/probes/fetch_probe.hip, profiles/r02_fetch_probe.md) shows one CU can pull the 121 MB key at 95-113 GB/s when loads are
// spread out, 2.4x what that kernel reached.  Here the chunks of step i+1 are requested during step i, once the registers that
// held step i's chunks are dead: the idle waves of half 1 right after the hand-off, the transforming waves one row's worth at a
// time between the stages of their inverse transform (compiler fences pin the places) -- nobody's transform waits on the queue.
// Transforms are variant "q" (first transpose in registers, padded buffer, pass-1 twiddles from per-lane roots): LDS = acc 8 + spectra 2l x 8 + 8 x 9 KiB.
// ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void wg_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
__device__ __forceinline__ void pin() { asm volatile("" ::: "memory"); }  // memory operations do not move across this point

template <int L, int LUT = kGate>
__global__ __launch_bounds__(512, 2) void sk_blind_rotate_coop_kernel(BRArgs a) {
    constexpr int ROWS = 2 * L;
    __shared__ __attribute__((aligned(4096))) int32_t sAcc[2048];
    __shared__ cplx sSpec[ROWS][512];
    __shared__ cplx sX[8][kXbufSlots];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const W64 w64{a.tw[TwRing1k::T2 + 1 * 8 + (lane & 7)]};
    const LaneRoots roots{a.tw[TwRing1k::ROOTS + 2 * lane], a.tw[TwRing1k::ROOTS + 2 * lane + 1]};
    const long job = blockIdx.x;
    const uniform_i32_ptr bara = as_uniform(a.bara + job * a.n_pad);
    const int Bgbit = a.Bgbit;
    if (wave == 0) {
        if constexpr (LUT == kLutEnc) {
            const size_t t = a.lut_idx ? (size_t)a.lut_idx[job] * 1024 : 0;
            acc_init_tlwe16(lane, sAcc, sAcc + 1024, a.barb[job], a.tv_a + t, a.tv + t);
        } else if constexpr (LUT == kLutMv) acc_init_tv16(lane, sAcc, sAcc + 1024, a.barb[job], a.tv);
        else if constexpr (LUT) acc_init_tv16(lane, sAcc, sAcc + 1024, a.barb[job], a.tv + (a.lut_idx ? (size_t)a.lut_idx[job] * 1024 : 0));
        else acc_init16(lane, sAcc, sAcc + 1024, a.barb[job], a.mu);
    }
    const int c = (wave >> 1) & 1, h = wave & 1, half = wave >> 2, r0 = half * L;  // role in M: rows r0 .. r0+L-1 of (column c, limb h)
    unsigned int *ap = reinterpret_cast<unsigned int *>(sAcc) + c * 1024;
    cplx *xb = sX[wave];

    int i = 0;
    while (i < a.n && bara[i] == 0) i++;   // J/bootstrap.jl:40: mask words that mod-switch to 0 are skipped (uniform over the workgroup)
    cplx B[L][8];
    if (i < a.n) {
#pragma unroll
        for (int r = 0; r < L; r++) load8(lane, B[r], a.bk + bk_spec_index(i, r0 + r, c, h, ROWS));
    }
    wg_barrier();
    STAMP_DECL;
    while (i < a.n) {
        const int a2n = bara[i] & 2047;
        int inext = i + 1;
        while (inext < a.n && bara[inext] == 0) inext++;
        const int inl = inext < a.n ? inext : i;   // the last step re-requests its own chunks: unconditional loads keep B one set of registers
        // ---- F ----
        if (wave < ROWS) {
            cplx z[8];
            rotated_digits_z(lane, sAcc + (wave / L) * 1024, a2n, (wave % L) + 1, L, Bgbit, z);
            wave_fft_fwd_q(lane, z, xb, roots, w64);
#pragma unroll
            for (int m = 0; m < 8; m++) sSpec[wave][m * 64 + lane] = z[m];
        }
        STAMP(0);
        wg_barrier();  // spectra published; every rotated read of the accumulator is done
        STAMP(1);
        // ---- M ----
        cplx S[8];
#pragma unroll
        for (int m = 0; m < 8; m++) S[m] = cplx{0.0, 0.0};
#pragma unroll
        for (int r = 0; r < L; r++) {
            cplx z[8];
#pragma unroll
            for (int m = 0; m < 8; m++) z[m] = sSpec[r0 + r][m * 64 + lane];
            mac8r(S, z, B[r]);
            pin();   // one row's spectrum in registers at a time (hoisting all 2l x 8 reads costs more registers than there are)
        }
        STAMP(2);
        if (half == 1) {
#pragma unroll
            for (int m = 0; m < 8; m++) xb[m * 64 + lane] = S[m];   // hand-off to wave - 4 (this wave's transpose buffer is idle)
            pin();
            STAMP(3);
            wg_barrier();
            STAMP(4);
            // nothing else to do until the next step: request all of its chunks now (AFTER the barrier: the partners' inverse
            // transforms must not wait for these 8 l loads to be accepted by the memory pipeline)
#pragma unroll
            for (int r = 0; r < L; r++) {
                const cplx *src = a.bk + bk_spec_index(inl, r0 + r, c, h, ROWS);
#pragma unroll
                for (int m = 0; m < 8; m++) {
                    B[r][m] = src[m * 64 + lane];
                    pin();
                    __builtin_amdgcn_s_sleep(1);   // paced: these waves have the whole inverse phase; a flooded queue stalls the partners' loads
                }
            }
        } else {
            load8(lane, B[0], a.bk + bk_spec_index(inl, r0, c, h, ROWS));
            pin();
            STAMP(3);
            wg_barrier();
            STAMP(4);
            // ---- I ----
            const cplx *px = sX[wave + 4];
#pragma unroll
            for (int m = 0; m < 8; m++) {
                const cplx v = px[m * 64 + lane];
                S[m].re += v.re;
                S[m].im += v.im;
            }
            wave_sync();
            invr_seg1(lane, S, xb, w64);
            pin();
            if (L > 1) load8(lane, B[L > 1 ? 1 : 0], a.bk + bk_spec_index(inl, r0 + 1, c, h, ROWS));
            pin();
            wave_sync();
            inv_seg2_ld(lane, S, xb);
            dft8<-1>(S);
            pin();
            if (L > 2) load8(lane, B[L > 2 ? 2 : 0], a.bk + bk_spec_index(inl, r0 + 2, c, h, ROWS));
            if (L > 3) load8(lane, B[L > 3 ? 3 : 0], a.bk + bk_spec_index(inl, r0 + 3, c, h, ROWS));
            pin();
            wave_transpose_hi3(S);
            invq_seg3(S, roots);
#pragma unroll
            for (int m = 0; m < 8; m++) {
                const int q = lane + 64 * m;
                atomicAdd(ap + q, round_lo32(S[m].re) << (16 * h));
                atomicAdd(ap + q + 512, round_lo32(S[m].im) << (16 * h));
            }
        }
        STAMP(3);
        wg_barrier();  // accumulator updated before anybody rotates it again
        STAMP(5);
        i = inext;
    }
    STAMP_FLUSH(blockIdx.x, wave);
    if constexpr (LUT == kLutMv) {
        const uniform_i32_ptr w = as_uniform(a.mv_w) + (size_t)(a.lut_idx ? as_uniform(a.lut_idx)[job] : 0) * a.theta * a.mv_p;
        for (int j = wave; j < a.theta; j += 8)   // the q outputs dealt over the eight waves
            extract_mv16(lane, sAcc, sAcc + 1024, w + j * a.mv_p, a.mv_p, a.mv_box, a.out + (job * a.theta + j) * 1025);
    } else if constexpr (LUT) {
        if (wave < a.theta) extract_at16(lane, sAcc, sAcc + 1024, wave, a.out + (job * a.theta + wave) * 1025);   // one wave per output
    } else {
        if (wave == 0) extract16(lane, sAcc, sAcc + 1024, a.out + job * 1025);
    }
}

__global__ __launch_bounds__(256) void sk_linear_kernel(const int32_t *__restrict__ in0, int32_t *__restrict__ out, size_t words, int negate) {
    const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (q < words) out[q] = negate ? (int32_t)(0u - (uint32_t)in0[q]) : in0[q];
}

}  // namespace

// ======================================================================================================
// host side
// ======================================================================================================
// Device-resident TGSW samples of thfhe_tgsw_set_create: the spectra of count x d address bits, laid out like the bootstrapping key's with
// (sample d + bit) in the place of the key index.  Belongs to the context that made it and is destroyed before it; the computed sets of the gate DAG
// (thfhe_dag_run_cb_batch) are the context's own.
struct THFHE_INTERNAL thfhe_tgsw_set {
    thfhe_ctx *ctx = nullptr;
    DevBuf spec;
    size_t count = 0;
    int d = 0;
};

struct THFHE_INTERNAL thfhe_ctx : DevCtx {
    thfhe_params p;
    int rec_words() const { return p.n + 1; }
    DevBuf d_bk;              // spectral key
    DevBuf d_bk_ring;         // the same size again: its phased copy for the ring kernels (variant "p" in thfhe_lane.h), X^32 b at the points with bit 5 of nu set
    KsKey ksk;                // padded rows (+ the matrix-core planes)
    int coop_max_jobs = 768;    // remainders (batch mod 2048) up to this many rotations use the cooperative (latency) kernel
    int ring4_max_jobs = 1024;  // ... above it and up to this many, the four-wave ring kernel (launch_br)
    // workspace
    int n_pad = 0;
    DevBuf d_bara, d_barb, d_u;
    DevBuf d_tv, d_lut_idx;   // programmable bootstrap: test-vector table and per-sample table index (grow-only)
    DevBuf d_tva;             // encrypted tables (thfhe_lut_bootstrap_enc): the masks; d_tv holds the bodies
    DevBuf d_mv_w;            // multi-value bootstrap (thfhe_mv_lut_bootstrap, thfhe_tree_lut_bootstrap_mv): the factor tables; d_tv holds the base vector
    // tree PBS (thfhe_tree_lut_bootstrap): a slice's table indices, key-switched level-1 candidates and packed tables (mask, body)
    DevBuf d_tree_tab, d_tree_lwe, d_tree_a, d_tree_b;
    // encrypted-table and tree nodes of the gate DAG (thfhe_dag_run_tree_batch): the run's encrypted tables (masks, bodies) and level-1 rows
    DevBuf d_dag_enc_a, d_dag_enc_b, d_dag_tv1;
    // multi-value nodes of the gate DAG (thfhe_dag_run_mv_batch): the run's base vectors and the factor array of all its specs
    DevBuf d_dag_mv_tv0, d_dag_mv_w;
    // leveled nodes of the gate DAG (thfhe_dag_run_lhe_batch): the run's table polynomials and final weights (masks, bodies) and the automata's word pool
    DevBuf d_dag_lhe_tab_a, d_dag_lhe_tab_b, d_dag_lhe_fin_a, d_dag_lhe_fin_b, d_dag_lhe_words;
    // leveled lookup (thfhe_lhe_cmux, thfhe_lhe_lookup): the CMux tree's workspace (masks, bodies) and the flat CMux's four operands
    DevBuf d_lhe_a, d_lhe_b, d_lhe_in[4];
    // layered automata (thfhe_lhe_wfa): the two layers alternate between d_lhe_a and d_lhe_b; the transition table and the start states
    DevBuf d_wfa_tab;
    // leveled scatter (thfhe_lhe_demux, thfhe_lhe_scatter): the demux trees run in d_lhe_a ([sample][leaf][mask | body]); the tables
    // being summed ([masks | bodies][n_tables][2^d_tree][N]) and a slice's value and table indices ([2][samples])
    DevBuf d_sc_tab, d_sc_idx;
    // circuit bootstrapping (thfhe_cb_key_set, thfhe_circuit_bootstrap): the private key-switching key; a slice's gate records, their
    // level-2 mod-switched words, level-2 accumulators, extracted records of one level, the l records per bit and the TGSW rows; the Torus64 test
    // vector of the one-rotation mode
    CbKey cb;
    // circuit-bootstrap nodes of the gate DAG (thfhe_dag_run_cb_batch): the computed sets (grow-only spectra, reused by the next run,
    // freed by thfhe_dag_cb_release), and the sets of the current run in the order its rows name them, the client's then the computed ones
    std::vector<std::unique_ptr<thfhe_tgsw_set>> cb_sets;
    std::vector<const thfhe_tgsw_set *> dag_sets;
    DevBuf d_cb_lwe, d_cb_bara, d_cb_barb, d_cb_acc, d_cb_x, d_cb_lwe2, d_cb_rows, d_cb_tv;
    int cus = 0;         // compute units of the device, asked once (ctx_cus)
    int wfa_chunk = 0;   // states per workgroup of sk_lhe_wfa_step_kernel, 0: chosen per slice (wfa_chunk_for)
    size_t tree_slice = 65536;   // level-1 candidates (samples x p_hi) per slice: bounds the workspace (8 KiB of T_i scratch per candidate); also the output records (samples x q) per slice of thfhe_mv_lut_bootstrap
    // staging for the host-buffer API
    Stage stage;
    LinBufs lin;   // dense layer (thfhe_lwe_linear, thfhe_linear_lut_bootstrap)
    // gate-DAG executor: wire table and index tables (grow-only, reused by every thfhe_dag_run on this context)
    DagBuffers dag;
    size_t dag_slice = 28672;  // gates per launch of a DAG level: 14 x 2048 (a MUX slice is 57 344 rotations); it sizes the staging arrays, not the prologue's grid: the runtime runs grid.y > 65 535 (66 636 rotations in one call, tests/test_gpu_large_batch.py)
    // thfhe_dag_last_group_ms: events of their own around a run's last SELECT / TREE / MV / TREE_MV / leveled group (made by the first profiled group);
    // ev[] stays what the stages record, so thfhe_last_timings answers as it did
    hipEvent_t grp_ev[2] = {nullptr, nullptr};
    bool grp_valid = false;
    ~thfhe_ctx() {
        for (hipEvent_t e : grp_ev)
            if (e) (void)hipEventDestroy(e);
    }
};

namespace {

// workspace of `jobs` rotations: bara / barb and one extracted record each; theta > 0: of PBS jobs with theta records each
int ensure_workspace(thfhe_ctx *c, size_t jobs, int theta = 0) {
    int rc = c->d_bara.grow(jobs * c->n_pad * sizeof(int32_t));
    if (!rc) rc = c->d_barb.grow(jobs * sizeof(int32_t));
    if (!rc) rc = c->d_u.grow(jobs * std::max(theta, 1) * ((size_t)c->p.N + 1) * sizeof(int32_t));
    return rc;
}

// One launch of `a.jobs` rotations on one kernel shape.  LUT: kGate, or a programmable-bootstrap instantiation.
template <int L, int LUT>
void launch_coop(const BRArgs &a, hipStream_t s) {
    hipLaunchKernelGGL((sk_blind_rotate_coop_kernel<L, LUT>), dim3((unsigned)a.jobs), dim3(512), 0, s, a);
}
template <int L, int LUT>
void launch_ring4(const BRArgs &a, hipStream_t s) {
    hipLaunchKernelGGL((sk_blind_rotate_ring_kernel<L, 4, LUT>), dim3((unsigned)((a.jobs + 3) / 4)), dim3(256), 0, s, a);
}
template <int L, int LUT>
void launch_ring8(const BRArgs &a, hipStream_t s) {
    hipLaunchKernelGGL((sk_blind_rotate_ring_kernel<L, 8, LUT>), dim3((unsigned)((a.jobs + 7) / 8)), dim3(512), 0, s, a);
}

// The rotations of a batch, piece by piece of launch_plan::sk_rotation_plan (thfhe_launch_plan.h: whole rounds on the eight-wave ring kernel,
// the remainder on the cheapest shape).  The pieces are independent jobs on disjoint slices of the same arrays, launched back to back on
// the context's stream.
template <int L, int LUT>
void launch_br(const BRArgs &a, hipStream_t s, int coop_max, int ring4_max) {
    auto piece = [&](long first, long count) {
        BRArgs b = a;
        b.bara += first * a.n_pad, b.barb += first, b.jobs = count;
        b.out += first * (LUT ? a.theta : 1) * 1025;
        if (LUT && b.lut_idx) b.lut_idx += first;
        return b;
    };
    launch_plan::SkPiece pc[launch_plan::kMaxPieces];
    const int n = launch_plan::sk_rotation_plan(a.jobs, coop_max, ring4_max, pc);
    for (int i = 0; i < n; i++) {
        const BRArgs b = piece(pc[i].first, pc[i].count);
        if (pc[i].shape == launch_plan::kRing8) launch_ring8<L, LUT>(b, s);
        else if (pc[i].shape == launch_plan::kCoop) launch_coop<L, LUT>(b, s);
        else launch_ring4<L, LUT>(b, s);
    }
}

// the blind rotations of `a` on the kernel shapes of launch_br, for the context's decomposition length
template <int LUT>
int launch_rotations(thfhe_ctx *c, const BRArgs &a) {
    return with_static_int<4>(c->p.l, kBadL, [&](auto l) { launch_br<decltype(l)::value, LUT>(a, c->stream, c->coop_max_jobs, c->ring4_max_jobs); });
}

// rotations (prologue + blind rotate) of `jobs` = gates * rot_per_gate jobs into c->d_u
int enqueue_rotations(thfhe_ctx *c, int op, const int32_t *d0, const int32_t *d1, const int32_t *d2, size_t gates,
                      int rot_per_gate, int32_t mu, const int32_t *d_ops = nullptr) {
    const size_t jobs = gates * rot_per_gate;
    int rc = ensure_workspace(c, jobs);
    if (rc) return rc;
    const int n = c->p.n;
    if (c->profiling) THFHE_HIP(hipEventRecord(c->ev[0], c->stream));
    dim3 pg((unsigned)((n + 1 + 255) / 256), (unsigned)jobs);
    hipLaunchKernelGGL(sk_prologue_kernel, pg, dim3(256), 0, c->stream, d0, d1, d2, op, d_ops, rot_per_gate, n, c->n_pad,
                       ilog2(2 * c->p.N), (long)jobs, c->d_bara.as<int32_t>(), c->d_barb.as<int32_t>());
    if (c->profiling) THFHE_HIP(hipEventRecord(c->ev[1], c->stream));
    BRArgs a{c->d_bk.as<cplx>(), c->d_bk_ring.as<cplx>(), c->d_tw.as<cplx>(), c->d_bara.as<int32_t>(), c->d_barb.as<int32_t>(), c->d_u.as<int32_t>(), (long)jobs, n, c->n_pad, c->p.Bgbit, mu};
    rc = launch_rotations<kGate>(c, a);
    if (rc) return rc;
    if (c->profiling) THFHE_HIP(hipEventRecord(c->ev[2], c->stream));
    THFHE_HIP(hipGetLastError());
    return THFHE_OK;
}

int enqueue_keyswitch(thfhe_ctx *c, const int32_t *d_u, int32_t *d_out, size_t gates, int rot_per_gate, bool timed) {
    KsArgs k = c->ksk.args(d_u, d_out, (long)gates);
    k.rot_per_gate = rot_per_gate;
    const int nsplit = gates <= 32 ? 16 : (gates <= 128 ? 8 : (gates <= 512 ? 2 : 1));  // fill the chip at small batch sizes
    THFHE_TRY(ks_enqueue(c->ksk, k, nsplit, c->stream));
    if (timed && c->profiling) {
        THFHE_HIP(hipEventRecord(c->ev[3], c->stream));
        c->ev_valid = true;
    }
    return THFHE_OK;
}

// the device side of a multi-value rotation's factor tables: int32[n_tables][q][p] taps
struct MvArgs {
    const int32_t *w;
    int p;
};

// One PBS stage on the context's stream, the workspace sized by the caller: the prologue of `jobs` jobs of `src`, their rotations on the plaintext
// tables tv (kLut) or, with tv_a, on the encrypted tables (tv_a, tv) (kLutEnc), theta records each into c->d_u; then, with ks_dst, the key switch of
// those jobs x theta records into it.  A source that writes no table index rotates on d_idx (null: table 0).  timed: the profiling events of a
// flat call (prologue | rotations | key switch).  mv: multi-value rotations (kLutMv) of the base vector tv, the index picks a table of theta = q factors.
template <typename Src>
int enqueue_pbs(thfhe_ctx *c, const Src &src, size_t jobs, const int32_t *tv, const int32_t *tv_a, int theta, const int32_t *d_idx, int32_t *ks_dst,
                bool timed = false, const MvArgs *mv = nullptr) {
    const int n = c->p.n;
    const bool ev = timed && c->profiling;
    int32_t *const idx = c->d_lut_idx.as<int32_t>();
    if (ev) THFHE_HIP(hipEventRecord(c->ev[0], c->stream));
    lut_prologue_launch(src, jobs, n, c->n_pad, ilog2(2 * c->p.N), c->d_bara.as<int32_t>(), c->d_barb.as<int32_t>(), idx, c->stream);
    if (ev) THFHE_HIP(hipEventRecord(c->ev[1], c->stream));
    BRArgs a{c->d_bk.as<cplx>(), c->d_bk_ring.as<cplx>(), c->d_tw.as<cplx>(), c->d_bara.as<int32_t>(), c->d_barb.as<int32_t>(), c->d_u.as<int32_t>(), (long)jobs, n, c->n_pad, c->p.Bgbit,
             0, tv, Src::kIdx == LutIdx::none ? d_idx : idx, theta, tv_a};
    if (mv) {
        a.mv_w = mv->w, a.mv_p = mv->p, a.mv_box = c->p.N / mv->p;
        THFHE_TRY(launch_rotations<kLutMv>(c, a));
    } else THFHE_TRY(tv_a ? launch_rotations<kLutEnc>(c, a) : launch_rotations<kLut>(c, a));
    if (ev) THFHE_HIP(hipEventRecord(c->ev[2], c->stream));
    THFHE_HIP(hipGetLastError());
    return ks_dst ? enqueue_keyswitch(c, c->d_u.as<int32_t>(), ks_dst, jobs * theta, 1, timed) : THFHE_OK;
}

int gates_dev_locked(thfhe_ctx *c, int op, const int32_t *d0, const int32_t *d1, const int32_t *d2, int32_t *dout, size_t count) {
    if (count == 0) return THFHE_OK;
    if (count > (size_t)INT32_MAX / 4) return thfhe_fail(THFHE_E_INVALID, "count too large");
    THFHE_HIP(hipSetDevice(c->device));
    if (op == THFHE_NOT || op == THFHE_COPY) {
        const size_t words = count * c->rec_words();
        hipLaunchKernelGGL(sk_linear_kernel, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, c->stream, d0, dout, words,
                           op == THFHE_NOT ? 1 : 0);
        THFHE_HIP(hipGetLastError());
        return THFHE_OK;
    }
    Lin L;
    if (!gate_lin(op, 0, L) || op == kOpIdentity) return thfhe_fail(THFHE_E_INVALID, "unknown gate opcode");
    if (!d0 || !d1 || (op == THFHE_MUX && !d2)) return thfhe_fail(THFHE_E_INVALID, "null operand");
    const int rot = op == THFHE_MUX ? 2 : 1;
    int rc = enqueue_rotations(c, op, d0, d1, d2, count, rot, 1 << 29);
    if (rc) return rc;
    return enqueue_keyswitch(c, c->d_u.as<int32_t>(), dout, count, rot, true);
}

// one launch of a gate-DAG gate class from the staging arrays into stage.out (thfhe_dag.h, dag_execute's run): two-input gates with per-gate
// opcodes, or MUX
int dag_gate_class(thfhe_ctx *c, int cls, const int32_t *d_ops, size_t n) {
    const bool is_mux = cls == kDagMux;
    int r = enqueue_rotations(c, is_mux ? THFHE_MUX : THFHE_NAND, c->stage.in_ptr(0), c->stage.in_ptr(1), is_mux ? c->stage.in_ptr(2) : nullptr, n, is_mux ? 2 : 1, 1 << 29,
                              is_mux ? nullptr : d_ops);
    if (!r) r = enqueue_keyswitch(c, c->d_u.as<int32_t>(), c->stage.out_ptr(), n, is_mux ? 2 : 1, false);
    return r;
}

// thfhe_lut_bootstrap(_enc)(_wo_keyswitch): ctx_lut_bootstrap (thfhe_pbs_host.h) on this engine's workspace and PBS stage
int lut_bootstrap(thfhe_ctx *c, const thfhe_lut_spec *sp, const int32_t *tv, int n_luts, const int32_t *lut_index, const int32_t *in0,
                  const int32_t *in1, const int32_t *in2, int32_t *out, size_t count, bool keyswitch, bool enc = false, const int32_t *tv_a = nullptr) {
    return ctx_lut_bootstrap(c, sp, tv, tv_a, enc, n_luts, lut_index, in0, in1, in2, out, count, keyswitch,
                             [&](size_t jobs, int theta) { return ensure_workspace(c, jobs, theta); }, [&](auto &&...a) { return enqueue_pbs(c, a...); });
}

// thfhe_lwe_linear / thfhe_linear_lut_bootstrap(_wo_keyswitch): ctx_linear (thfhe_pbs_host.h) on this engine's workspace and PBS stage
int linear(thfhe_ctx *c, const int32_t *W, const int32_t *bias, int M, int K, bool fused, int theta, const int32_t *tv, int n_luts, const int32_t *lut_index,
           const int32_t *in, int32_t *out, size_t count, bool keyswitch) {
    return ctx_linear(c, W, bias, M, K, fused, theta, tv, n_luts, lut_index, in, out, count, keyswitch,
                      [&](size_t jobs, int th) { return ensure_workspace(c, jobs, th); }, [&](auto &&...a) { return enqueue_pbs(c, a...); });
}

// Grow-only workspace of one tree chain over S samples / nodes: S R level-1 jobs of theta_lo records each (a SELECT group, whose candidates are
// gathered: R = theta_lo = 1, the selection rotation alone), their S k p candidates, S k packed tables and selection jobs (k tables per sample,
// R = 1, theta_lo = k p).
int tree_workspace(thfhe_ctx *c, size_t S, size_t p, size_t R, size_t theta_lo, size_t k = 1) {
    const size_t jobs = S * std::max(R, k), N = c->p.N;
    int rc = ensure_workspace(c, jobs);
    if (!rc) rc = c->d_u.grow(std::max(S * R * theta_lo, S * k) * (N + 1) * sizeof(int32_t));
    if (!rc) rc = c->d_lut_idx.grow(jobs * sizeof(int32_t));
    if (!rc) rc = c->d_tree_lwe.grow(S * k * p * c->rec_words() * sizeof(int32_t));
    if (!rc) rc = c->d_tree_a.grow(S * k * N * sizeof(int32_t));
    if (!rc) rc = c->d_tree_b.grow(S * k * N * sizeof(int32_t));
    return rc;
}

// One tree chain over S samples / nodes on the gate context's stream, the workspace sized by tree_workspace.  Level 1: S (p / theta_lo)
// rotations of the plaintext rows d_tv1 on the `lo` source, key-switched into the candidate buffer -- candidate k of sample s is record s p + k, the
// order the rotations write them in; lo = nullptr (SELECT): the caller has gathered the candidates there in that order.  Then the packing context's
// box packing of the candidates into S encrypted tables (pack_boxes_enqueue enqueues on the stream it is given), and the selection: sample s rotates
// its own packed table on the `hi` source, coefficient 0 key-switched into d_out.  seam(1) / seam(2) run after level 1 and after the packing: what
// the caller has to put on the stream there.  mv: level 1 is ONE multi-value rotation per sample of the base vector d_tv1 with
// theta_lo = k p outputs, the candidates in the same order.  k > 1 (mv only): k tables per sample -- output j p + h of the rotation is
// candidate h of table j, so the packed table of (s, j) is sample s k + j, and selection job s k + j rotates it on sample s's `hi` operands (the
// `hi` source repeats every sample k times and numbers its jobs): S k records into d_out.
template <typename Lo, typename Hi, typename Seam>
int enqueue_tree_chain(thfhe_ctx *c, thfhe_poly_ctx *pc, const Lo &lo, const int32_t *d_tv1, int theta_lo, const Hi &hi, size_t S, int p, int32_t *d_out,
                       Seam seam, const MvArgs *mv = nullptr, size_t k = 1) {
    int32_t *const cand = c->d_tree_lwe.as<int32_t>(), *const tab_a = c->d_tree_a.as<int32_t>(), *const tab_b = c->d_tree_b.as<int32_t>();
    if constexpr (!std::is_same_v<Lo, std::nullptr_t>) THFHE_TRY(enqueue_pbs(c, lo, S * (k * p / theta_lo), d_tv1, nullptr, theta_lo, nullptr, cand, false, mv));
    THFHE_TRY(seam(1));
    THFHE_TRY(pack_boxes_enqueue(pc, cand, S * k * p, p, tab_a, tab_b, c->stream));
    THFHE_TRY(seam(2));
    return enqueue_pbs(c, hi, S * k, tab_b, tab_a, 1, nullptr, d_out);
}

// enqueue_tree_chain into stage.out as the shared call bodies (thfhe_pbs_host.h) call it; w, mv_p: the taps of a multi-value level 1 (null: rows)
auto tree_chain_of(thfhe_ctx *c, thfhe_poly_ctx *pc) {
    return [=](const auto &lo, const int32_t *d_tv1, int theta_lo, const auto &hi, size_t S, int p, auto seam, const int32_t *w, int mv_p, size_t k) {
        const MvArgs mv{w, mv_p};
        return enqueue_tree_chain(c, pc, lo, d_tv1, theta_lo, hi, S, p, c->stage.out_ptr(), seam, w ? &mv : nullptr, k);
    };
}

// ---- gate-DAG entry points: what thfhe_dag_run_batch, thfhe_dag_run_lut_batch and thfhe_dag_run_tree_batch share ----
int sk_dag_classify(int op) { return op == THFHE_NOT || op == THFHE_COPY ? kDagLinear : (op == THFHE_MUX ? kDagMux : (op >= THFHE_NAND && op <= THFHE_ORYN ? kDagGate2 : -1)); }

// dag_execute's ensure (dag_ensure, thfhe_pbs_host.h) on this engine's workspace
int sk_dag_ensure(thfhe_ctx *c, size_t max_gates, int theta_max, int32_t **in, int32_t **out) {
    return dag_ensure(c, max_gates, theta_max, in, out, [&](size_t jobs, int theta) { return ensure_workspace(c, jobs, theta); });
}

// The level-2 side of a run whose plan holds CB groups (thfhe_dag_cb.h): the context the gate context's stream is lent to, and its ring degree.
struct DagCbRun {
    thfhe_mk_ctx *l2 = nullptr;
    int N2 = 0;
};
int sk_dag_cb_reserve(thfhe_ctx *c, const DagPlan &plan, const DagFamilies &T, const DagCbRun &cbr, size_t instances);
int sk_dag_cb_group(thfhe_ctx *c, const DagCbRun &cbr, const DagPlan &plan, const DagFamilies &T, const DagExtGroup &g, size_t instances);
int cb_level2_begin(thfhe_ctx *c, thfhe_mk_ctx *l2, int mode, int *N2);
int cb_level2_end(thfhe_mk_ctx *l2);

// the leveled groups of a run (thfhe_dag_lhe.h, after the leveled kernels)
int sk_dag_lhe_check_sets(const thfhe_ctx *c, const DagPlan &plan, const DagFamilies &T, size_t instances);
int sk_dag_lhe_reserve(thfhe_ctx *c, const DagPlan &plan, const DagFamilies &T, size_t instances, size_t &w_cand);
int sk_dag_lhe_group(thfhe_ctx *c, thfhe_poly_ctx *pc, const DagPlan &plan, const DagFamilies &T, const DagExtGroup &g, size_t instances);

// The device side of the six-column entries, both contexts locked by the caller (T: the run's families, checked by dag_families_check; pc: null in a
// run without SELECT / TREE groups).  Gate classes run as in thfhe_dag_run_batch.  A LUT group is one PBS stage on the wire table over the run's plaintext tables
// (DESIGN 4.9), a LUT_ENC group the same over its encrypted tables.  TREE, TREE_MV and MV groups are dag_run_group's (thfhe_pbs_host.h) on this
// engine's chain and PBS stage, sized by dag_reserve_groups.  A SELECT group gathers its candidates into the buffer the box packing reads and runs
// the tree chain from there.  A leveled group is sk_dag_lhe_group's, a DENSE group dag_run_dense_group's on this
// engine's PBS stage.  Everything is enqueued on the gate context's stream.
int sk_dag_run_luts(thfhe_ctx *c, thfhe_poly_ctx *pc, const DagPlan &plan, const DagFamilies &T, const DagCall &A, size_t instances, const DagCbRun &cbr = {}) {
    const int words = c->rec_words();
    hipStream_t st = c->stream;
    if (cbr.l2) THFHE_TRY(sk_dag_cb_reserve(c, plan, T, cbr, instances));   // first: it refuses a run that does not fit (THFHE_E_NOMEM) with nothing done
    size_t w_cand = 0;   // the most candidates one packing takes
    THFHE_TRY(dag_reserve_groups(c, plan, T, instances, &thfhe_ctx::tree_slice, w_cand, [&](auto... a) { return tree_workspace(c, a...); },
                                 [&](size_t jobs, int theta) { return ensure_workspace(c, jobs, theta); }));
    for (const DagBatch &b : plan.batches) {   // a SELECT group's candidates are gathered: the selection rotation alone
        if (b.cls != kDagSelect) continue;
        const size_t p = (size_t)T.trees[b.tree].p_hi, S = dag_group_slice(c, T, b.cls, b.tree, b.count * instances, &thfhe_ctx::tree_slice);
        THFHE_TRY(tree_workspace(c, S, p, 1, 1));
        w_cand = std::max(w_cand, S * p);
    }
    if (T.lhe) THFHE_TRY(sk_dag_lhe_reserve(c, plan, T, instances, w_cand));
    if (w_cand) {
        THFHE_TRY(pack_boxes_reserve(pc, w_cand));
        THFHE_HIP(hipStreamSynchronize(pack_ctx_stream(pc)));   // the packing context's own stream is idle; from here on its buffers are used on `st`
    }
    THFHE_TRY(dag_upload_families<int32_t>(c, st, T));
    // one SELECT / TREE / MV / TREE_MV / leveled group of a level
    auto ext_group = [&](const DagExtGroup &g) -> int {
        int32_t *const dst = c->stage.out_ptr();
        if (g.cls == kDagDense) return dag_run_dense_group<int32_t>(c, T, g, &thfhe_ctx::tree_slice, [&](auto &&...a) { return enqueue_pbs(c, a...); });
        if (g.cls == kDagCb) return sk_dag_cb_group(c, cbr, plan, T, g, instances);
        if (g.cls >= kDagLheLookup) return sk_dag_lhe_group(c, pc, plan, T, g, instances);
        if (g.cls != kDagSelect)
            return dag_run_group<int32_t>(c, T, g, &thfhe_ctx::tree_slice, tree_chain_of(c, pc), [&](const auto &lo, size_t S, const int32_t *tv0, const int32_t *w, int mv_p, int q) {
                const MvArgs mv{w, mv_p};
                return enqueue_pbs(c, lo, S, tv0, nullptr, q, nullptr, dst, false, &mv);
            });
        const thfhe_tree_spec ts = T.trees[g.tree];   // t_y = first candidate wire
        const int p = ts.p_hi;
        return dag_group_slices(g, dag_group_slice(c, T, g.cls, g.tree, (size_t)g.all, &thfhe_ctx::tree_slice), 1, dst, words, st, [&](long first, long S) {
            const LutWireSrc<LutSpecByValue, LutIdx::job> hi{g.wires, g.t0, g.t1, g.t2, {ts.hi}, nullptr, first, g.cnt, g.n_wires, 1};
            hipLaunchKernelGGL(dag_select_gather_kernel, dim3((unsigned)((words + 255) / 256), (unsigned)std::min<long>(S * p, 65535)), dim3(256), 0, st,
                               (const int32_t *)g.wires, g.t_y, c->d_tree_lwe.as<int32_t>(), first, S, g.cnt, g.n_wires, words, p);
            return enqueue_tree_chain(c, pc, nullptr, nullptr, 1, hi, (size_t)S, p, dst, [](int) { return (int)THFHE_OK; });
        });
    };
    c->grp_valid = false;
    c->dag.timed = c->profiling;   // thfhe_dag_last_stage_ms
    return dag_execute(
        plan, c->dag, st, words, A, instances, c->dag_slice,
        [&](size_t max_gates, int32_t **in, int32_t **out) { return sk_dag_ensure(c, max_gates, plan.max_theta, in, out); },
        [&](int cls, const int32_t *d_ops, size_t m) { return dag_gate_class(c, cls, d_ops, m); },
        [&](int theta, const DagLutSlice &s) {
            return enqueue_pbs(c, s.src(c->dag.specs.as<thfhe_lut_spec>()), (size_t)s.total, (s.enc ? c->d_dag_enc_b : c->d_tv).as<int32_t>(),
                               s.enc ? c->d_dag_enc_a.as<int32_t>() : nullptr, theta, nullptr, c->stage.out_ptr());
        },
        [&](const DagExtGroup &g) -> int {
            // profiling (thfhe_set_profiling): a pair of events of the group's own around it, first launch to last scatter, for thfhe_dag_last_group_ms;
            // a later group of the run records over them, a gate level or a stage's ev[] does not touch them
            if (!c->profiling) return ext_group(g);
            for (hipEvent_t &e : c->grp_ev)
                if (!e) THFHE_HIP(hipEventCreate(&e));
            c->grp_valid = false;
            THFHE_HIP(hipEventRecord(c->grp_ev[0], st));
            THFHE_TRY(ext_group(g));
            THFHE_HIP(hipEventRecord(c->grp_ev[1], st));
            c->grp_valid = true;
            return THFHE_OK;
        });
}

// ---- what thfhe_tree_lut_bootstrap and thfhe_tree_lut_bootstrap_mv share ----
// what tree_validate (thfhe_pbs_host.h) admits here: p_hi up to N / 2
constexpr TreeRules kTreeRules{512, "tree: p_hi must be a power of two in 2 .. N/2", "tree: n_tables must be 1 .. 262144 / (p_hi / theta)"};

// Two-digit tree PBS: both locks and the packing key's checks, then ctx_tree_bootstrap (thfhe_pbs_host.h) on this engine's
// tree workspace and chain, ev[0] on the call's first slice.  The arguments have passed the entry's host checks.
int tree_bootstrap(thfhe_ctx *c, thfhe_poly_ctx *pc, const thfhe_lut_spec &lo, const thfhe_lut_spec &hi, int p_hi, const int32_t *tv, size_t tv_rows,
                   const int32_t *factors, int mv_p, int mv_tables, const int32_t *table_index, const int32_t *lo0, const int32_t *lo1, const int32_t *lo2,
                   const int32_t *hi0, const int32_t *hi1, const int32_t *hi2, int32_t *out, size_t count, int k = 1) {
    if (!c || !pc) return thfhe_fail(THFHE_E_INVALID, "null ctx");
    if (pack_ctx_device(pc) != c->device) return thfhe_fail(THFHE_E_INVALID, "tree: the gate context and the packing context must be on the same device");
    DevLock lk(*c);
    if (lk.rc) return lk.rc;
    std::lock_guard<std::mutex> pg(pack_ctx_mutex(pc));   // always after the gate context's: nothing else takes both
    if (!pack_key_n(pc)) return thfhe_fail(THFHE_E_INVALID, "tree: no packing key set (thfhe_pack_key_set)");
    if (pack_key_n(pc) != c->p.n) return thfhe_fail(THFHE_E_INVALID, "tree: the packing key's LWE dimension differs from the gate context's n");
    if (count) THFHE_HIP(hipStreamSynchronize(pack_ctx_stream(pc)));   // the packing context's own stream is idle (its calls drain it); from here on its buffers are used on c->stream
    return ctx_tree_bootstrap(c, lo, hi, p_hi, tv, tv_rows, factors, mv_p, mv_tables, table_index, lo0, lo1, lo2, hi0, hi1, hi2, out, count, k, true,
                              [&](auto... a) { return tree_workspace(c, a...); }, tree_chain_of(c, pc));
}

// thfhe_mv_lut_bootstrap(_wo_keyswitch): ctx_mv_lut_bootstrap (thfhe_pbs_host.h) in slices of at most tree_slice records, one kLutMv
// stage of theta = q records per slice
int mv_lut_bootstrap(thfhe_ctx *c, const thfhe_lut_spec *sp, const int32_t *tv0, const int32_t *factors, int p, int q, int n_tables,
                     const int32_t *table_index, const int32_t *in0, const int32_t *in1, const int32_t *in2, int32_t *out, size_t count, bool keyswitch) {
    return ctx_mv_lut_bootstrap(c, sp, tv0, factors, p, q, n_tables, table_index, in0, in1, in2, out, count, keyswitch, &thfhe_ctx::tree_slice,
                                [&](size_t jobs, int theta) { return ensure_workspace(c, jobs, theta); },
                                [&](const auto &src, size_t S, const int32_t *d_idx, int32_t *ks_dst, bool last) {
                                    const MvArgs mv{c->d_mv_w.as<int32_t>(), p};
                                    return enqueue_pbs(c, src, S, c->d_tv.as<int32_t>(), nullptr, q, d_idx, ks_dst, last, &mv);
                                });
}

// What the six-column entries share (T: the entry's families and the generations of node kinds it admits): the host checks and the plan, the two
// locks, the run in sk_dag_run_luts (a plan with CB groups: between cb_level2_begin and cb_level2_end, the level-2 context enqueueing on the gate
// context's stream; stats is then int64[5]).  Both contexts stay locked for the run.  The LUT entry has plaintext tables only, so its plans
// hold no group that needs the packing context; from thfhe_dag_run_tree_batch on every family may be absent.
int sk_dag_run(thfhe_ctx *c, thfhe_poly_ctx *pc, const DagCall &A, DagFamilies T, size_t instances, int64_t *stats, thfhe_mk_ctx *l2 = nullptr) {
    const bool ext = T.gens & kDagGenTree;
    DagPlan plan;
    THFHE_TRY(dag_checked_plan(A, T, sk_dag_classify, plan));
    if (stats && ext) plan.fill_stats(stats);   // the plan's figures need no device
    const bool packs = plan.has_tree_groups(), cbs = plan.has_cb_groups();
    if (stats && T.cb) stats[4] = T.cb->mode == THFHE_CB_ONE_ROTATION ? (int64_t)plan.cb_bits : 0;
    if (T.lhe && !plan.has_lhe_groups()) T.lhe = nullptr;
    if (T.lhe) THFHE_TRY(sk_dag_lhe_check_sets(c, plan, T, instances));   // the sets, then the context
    if (!c || (packs && !pc)) return thfhe_fail(THFHE_E_INVALID, "null ctx");
    if (cbs && !l2) return thfhe_fail(THFHE_E_INVALID, "null ctx: the plan holds CB nodes, which need the level-2 context");
    if (stats && cbs && T.cb->mode == THFHE_CB_PER_LEVEL) stats[4] = (int64_t)plan.cb_bits * c->p.l;
    if (stats && !ext) plan.fill_stats(stats);   // thfhe_dag_run_lut_batch gives them to a caller with a context only
    if (packs && pack_ctx_device(pc) != c->device)
        return thfhe_fail(THFHE_E_INVALID, "tree: the gate context and the packing context must be on the same device");
    DevLock lk(*c);
    if (lk.rc) return lk.rc;
    std::unique_lock<std::mutex> pg;   // always after the gate context's: nothing else takes both
    if (packs) {
        pg = std::unique_lock<std::mutex>(pack_ctx_mutex(pc));
        if (!pack_key_n(pc)) return thfhe_fail(THFHE_E_INVALID, "tree: no packing key set (thfhe_pack_key_set)");
        if (pack_key_n(pc) != c->p.n) return thfhe_fail(THFHE_E_INVALID, "tree: the packing key's LWE dimension differs from the gate context's n");
    }
    if (ext) {   // the LUT entry uploads its tables for an empty run too, and leaves the instance count to dag_execute
        if (instances == 0 || A.n_nodes == 0) return THFHE_OK;
        if (instances > (size_t)INT32_MAX / 16) return thfhe_fail(THFHE_E_INVALID, "too many instances");
    }
    if (!cbs) return sk_dag_run_luts(c, packs ? pc : nullptr, plan, T, A, instances);
    DagCbRun cbr{l2, 0};
    THFHE_TRY(cb_level2_begin(c, l2, T.cb->mode, &cbr.N2));
    const int rc = sk_dag_run_luts(c, packs ? pc : nullptr, plan, T, A, instances, cbr);
    const int rc2 = cb_level2_end(l2);   // drains the stream first
    return rc ? rc : rc2;
}

#include "thfhe_lhe.h"
#include "thfhe_dag_lhe.h"
#include "thfhe_cb_host.h"
#include "thfhe_dag_cb.h"

}  // namespace

extern "C" {

int thfhe_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int thfhe_device_pci_bus_id(int device, char *buf, int len) {
    if (!buf || len < 16) return thfhe_fail(THFHE_E_INVALID, "buffer of at least 16 bytes expected");
    THFHE_HIP(hipDeviceGetPCIBusId(buf, len, device));
    return THFHE_OK;
}

int thfhe_ctx_create(const thfhe_params *p, const int32_t *bk_coeff, const int32_t *ksk, int device, thfhe_ctx **out) {
    if (!p || !bk_coeff || !ksk || !out) return thfhe_fail(THFHE_E_INVALID, "null argument");
    *out = nullptr;
    if (p->torus_bits != 32 || p->parties != 1) return thfhe_fail(THFHE_E_UNSUPPORTED, "thfhe_ctx_create is the single-key Torus32 path; use thfhe_mk_ctx_create");
    if (p->N != 1024 || p->k != 1) return thfhe_fail(THFHE_E_UNSUPPORTED, "only N = 1024, k = 1 is implemented");
    if (p->l < 1 || p->l > 4 || p->Bgbit < 1 || p->Bgbit > 10 || p->l * p->Bgbit > 32)
        return thfhe_fail(THFHE_E_UNSUPPORTED, "need 1 <= l <= 4, Bgbit <= 10 (FP64 exactness bound), l*Bgbit <= 32");
    if (p->n < 1 || p->n > 1407) return thfhe_fail(THFHE_E_UNSUPPORTED, "need 1 <= n <= 1407");
    if (p->ks_t < 1 || p->ks_basebit < 1 || p->ks_t * p->ks_basebit > 31) return thfhe_fail(THFHE_E_INVALID, "bad key-switch parameters");
    std::unique_ptr<thfhe_ctx> c(new (std::nothrow) thfhe_ctx);
    if (!c) return thfhe_fail(THFHE_E_NOMEM, "out of host memory");
    THFHE_TRY(c->open(device, true));
    c->p = *p;
    c->n_pad = (p->n + 3) & ~3;
    THFHE_TRY(c->upload_twiddles(1024));
    // bootstrapping key: upload coefficients, transform on device
    DevBuf coeff;  // upload staging
    const long npolys = (long)p->n * 2 * p->l * 2;
    THFHE_TRY(coeff.grow((size_t)npolys * 1024 * sizeof(int32_t)));
    THFHE_HIP(hipMemcpyAsync(coeff.as<int32_t>(), bk_coeff, (size_t)npolys * 1024 * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    THFHE_TRY(c->d_bk.grow((size_t)npolys * 1024 * sizeof(cplx)));
    THFHE_TRY((launch_torus_transform<1024, 32>(c->stream, coeff.as<int32_t>(), npolys, c->d_tw.as<cplx>(), c->d_bk.as<cplx>())));
    THFHE_TRY(c->d_bk_ring.grow((size_t)npolys * 1024 * sizeof(cplx)));
    THFHE_TRY((launch_torus_transform<1024, 32, MapPhased>(c->stream, coeff.as<int32_t>(), npolys, c->d_tw.as<cplx>(), c->d_bk_ring.as<cplx>())));
    THFHE_TRY(c->ksk.upload(ksk, 1, p->N, p->n, p->ks_t, p->ks_basebit, true, c->stream));   // (synchronises: the transform is done too)
    *out = c.release();
    return THFHE_OK;
}

void thfhe_ctx_destroy(thfhe_ctx *c) { ctx_destroy(c); }

int thfhe_ctx_params(const thfhe_ctx *c, thfhe_params *out) {
    if (!c || !out) return thfhe_fail(THFHE_E_INVALID, "null argument");
    *out = c->p;
    return THFHE_OK;
}

void *thfhe_dev_alloc(thfhe_ctx *c, size_t bytes) { return ctx_dev_alloc(c, bytes); }
void thfhe_dev_free(thfhe_ctx *c, void *p) { ctx_dev_free(c, p); }
int thfhe_copy_h2d(thfhe_ctx *c, void *dst, const void *src, size_t bytes) { return ctx_copy(c, dst, src, bytes, hipMemcpyHostToDevice); }
int thfhe_copy_d2h(thfhe_ctx *c, void *dst, const void *src, size_t bytes) { return ctx_copy(c, dst, src, bytes, hipMemcpyDeviceToHost); }
int thfhe_reserve(thfhe_ctx *c, size_t max_count) {
    if (!c) return thfhe_fail(THFHE_E_INVALID, "null ctx");
    DevLock lk(*c);
    if (lk.rc) return lk.rc;
    return ensure_workspace(c, max_count * 2);
}
int thfhe_sync(thfhe_ctx *c) { return ctx_sync(c); }
#ifdef THFHE_STAMPS
int thfhe_debug_read_stamps(unsigned long long *dst, size_t count) {
    return hipMemcpyFromSymbol(dst, HIP_SYMBOL(g_stamps), count * sizeof(unsigned long long)) == hipSuccess ? 0 : -1;
}
#endif
int thfhe_set_coop_threshold(thfhe_ctx *c, int max_jobs) {
    if (!c || max_jobs < 0) return thfhe_fail(THFHE_E_INVALID, "bad argument");
    std::lock_guard<std::mutex> g(c->mu);
    c->coop_max_jobs = max_jobs;
    return THFHE_OK;
}
int thfhe_set_ring4_threshold(thfhe_ctx *c, int max_jobs) {
    if (!c || max_jobs < 0) return thfhe_fail(THFHE_E_INVALID, "bad argument");
    std::lock_guard<std::mutex> g(c->mu);
    c->ring4_max_jobs = max_jobs;
    return THFHE_OK;
}
int thfhe_rotation_kernel_name(const thfhe_ctx *c, size_t rotations, char *buf, int len) {
    if (!c || !buf) return thfhe_fail(THFHE_E_INVALID, "null argument");
    std::lock_guard<std::mutex> g(const_cast<thfhe_ctx *>(c)->mu);   // the thresholds are set under it
    return kernel_name_result(len, launch_plan::sk_kernel_name(c->p.l, (long)rotations, c->coop_max_jobs, c->ring4_max_jobs, buf, len > 0 ? (size_t)len : 0));
}
int thfhe_set_profiling(thfhe_ctx *c, int enabled) {
    THFHE_TRY(ctx_set_profiling(c, enabled));
    std::lock_guard<std::mutex> g(c->mu);
    c->grp_valid = false;
    c->dag.st_valid = false;
    return THFHE_OK;
}
int thfhe_last_timings(thfhe_ctx *c, float ms[4]) { return ctx_last_timings(c, ms); }
int thfhe_dag_last_group_ms(thfhe_ctx *c, float *ms) {
    if (!c || !ms) return thfhe_fail(THFHE_E_INVALID, "null argument");
    std::lock_guard<std::mutex> g(c->mu);
    if (!c->profiling || !c->grp_valid) return thfhe_fail(THFHE_E_INVALID, "no profiled group recorded");
    THFHE_HIP(hipEventSynchronize(c->grp_ev[1]));
    THFHE_HIP(hipEventElapsedTime(ms, c->grp_ev[0], c->grp_ev[1]));
    return THFHE_OK;
}
// ms = {uploads, the levels, output gather + download} of the last six-column run made with profiling on (DagBuffers::st_ev)
int thfhe_dag_last_stage_ms(thfhe_ctx *c, float ms[3]) {
    if (!c || !ms) return thfhe_fail(THFHE_E_INVALID, "null argument");
    std::lock_guard<std::mutex> g(c->mu);
    if (!c->profiling || !c->dag.st_valid) return thfhe_fail(THFHE_E_INVALID, "no profiled run recorded");
    THFHE_HIP(hipEventSynchronize(c->dag.st_ev[3]));
    for (int k = 0; k < 3; k++) THFHE_HIP(hipEventElapsedTime(&ms[k], c->dag.st_ev[k], c->dag.st_ev[k + 1]));
    return THFHE_OK;
}

int thfhe_gates_dev(thfhe_ctx *c, int op, const int32_t *d0, const int32_t *d1, const int32_t *d2, int32_t *dout, size_t count) {
    if (!c || !d0 || !dout) return thfhe_fail(THFHE_E_INVALID, "null argument");
    std::lock_guard<std::mutex> g(c->mu);
    return gates_dev_locked(c, op, d0, d1, d2, dout, count);
}

int thfhe_gates(thfhe_ctx *c, int op, const int32_t *in0, const int32_t *in1, const int32_t *in2, int32_t *out, size_t count) {
    return ctx_gates(c, in0, in1, in2, out, count, [&](const int32_t *d0, const int32_t *d1, const int32_t *d2, int32_t *dout, size_t n) {
        return gates_dev_locked(c, op, d0, d1, d2, dout, n);
    });
}

int thfhe_gates_mixed(thfhe_ctx *c, const int32_t *ops, const int32_t *in0, const int32_t *in1, int32_t *out, size_t count) {
    if (!c || !ops || !in0 || !in1 || !out) return thfhe_fail(THFHE_E_INVALID, "null argument");
    if (count == 0) return THFHE_OK;
    for (size_t g = 0; g < count; g++)
        if (ops[g] < THFHE_NAND || ops[g] > THFHE_ORYN) return thfhe_fail(THFHE_E_INVALID, "thfhe_gates_mixed takes two-input bootstrapped gates only");
    return ctx_gates_mixed(c, ops, in0, in1, out, count, [&](const int32_t *d0, const int32_t *d1, const int32_t *d_ops, int32_t *dout) {
        int rc = enqueue_rotations(c, THFHE_NAND, d0, d1, nullptr, count, 1, 1 << 29, d_ops);
        return rc ? rc : enqueue_keyswitch(c, c->d_u.as<int32_t>(), dout, count, 1, true);
    });
}

// Gate-DAG evaluation: ASAP levelising scheduler (thfhe_dag.h) + device-resident executor.  The reference's
// applications issue these gates as sequential boots* calls (src/KNN_medical_data.cpp:127-489), once per test record (:676-691); here
// every level is one blind-rotate launch per gate class over ALL instances, the wire tables stay in HBM and nothing synchronises with
// the host between levels.
int thfhe_dag_run_batch(thfhe_ctx *c, const int32_t *inputs, size_t n_inputs, const int32_t *gates, size_t n_gates, size_t instances,
                        const int32_t *out_wires, size_t n_out, int32_t *outputs, int64_t *stats) {
    return dag_gates_run_batch(
        c, DagCall{inputs, n_inputs, gates, n_gates, out_wires, n_out, outputs}, instances, stats, sk_dag_classify,
        [&](size_t max_gates, int32_t **in, int32_t **out) { return sk_dag_ensure(c, max_gates, 0, in, out); },
        [&](int cls, const int32_t *d_ops, size_t n) { return dag_gate_class(c, cls, d_ops, n); });
}

// The six-column entries: each fills the families it has and the generations of node kinds it admits; the rest is sk_dag_run.
// LUT nodes among the gates: plaintext tables only -- no encrypted tables, no trees, no packing context.
int thfhe_dag_run_lut_batch(thfhe_ctx *c, const int32_t *inputs, size_t n_inputs, const int32_t *nodes, size_t n_nodes, const thfhe_lut_spec *specs,
                            int n_specs, const int32_t *tv, int n_luts, size_t instances, const int32_t *out_wires, size_t n_out, int32_t *outputs,
                            int64_t *stats) {
    const DagFamilies T{kDagGenLut, specs, n_specs, tv, n_luts};
    return sk_dag_run(c, nullptr, DagCall{inputs, n_inputs, nodes, n_nodes, out_wires, n_out, outputs}, T, instances, stats);
}

// encrypted-table, select and tree nodes among those.
int thfhe_dag_run_tree_batch(thfhe_ctx *c, thfhe_poly_ctx *pc, const int32_t *inputs, size_t n_inputs, const int32_t *nodes, size_t n_nodes,
                             const thfhe_lut_spec *specs, int n_specs, const int32_t *tv, int n_luts, const int32_t *enc_a, const int32_t *enc_b, int n_enc,
                             const thfhe_tree_spec *trees, int n_trees, const int32_t *tv1, int n_tv1_rows, size_t instances, const int32_t *out_wires,
                             size_t n_out, int32_t *outputs, int64_t *stats) {
    const DagFamilies T{kDagGenLut | kDagGenTree, specs, n_specs, tv, n_luts, enc_a, enc_b, n_enc, trees, n_trees, tv1, n_tv1_rows};
    return sk_dag_run(c, pc, DagCall{inputs, n_inputs, nodes, n_nodes, out_wires, n_out, outputs}, T, instances, stats);
}

// the multi-value nodes and their families.
int thfhe_dag_run_mv_batch(thfhe_ctx *c, thfhe_poly_ctx *pc, const int32_t *inputs, size_t n_inputs, const int32_t *nodes, size_t n_nodes,
                           const thfhe_lut_spec *specs, int n_specs, const int32_t *tv, int n_luts, const int32_t *enc_a, const int32_t *enc_b, int n_enc,
                           const thfhe_tree_spec *trees, int n_trees, const int32_t *tv1, int n_tv1_rows, const thfhe_mv_spec *mvs, int n_mvs,
                           const int32_t *mv_tv0, int n_bases, const int32_t *mv_factors, size_t n_factor_words, size_t instances, const int32_t *out_wires,
                           size_t n_out, int32_t *outputs, int64_t *stats) {
    const DagFamilies T{kDagGenLut | kDagGenTree | kDagGenMv, specs, n_specs, tv, n_luts, enc_a, enc_b, n_enc, trees, n_trees, tv1, n_tv1_rows,
                        mvs, n_mvs, mv_tv0, n_bases, mv_factors, n_factor_words};
    return sk_dag_run(c, pc, DagCall{inputs, n_inputs, nodes, n_nodes, out_wires, n_out, outputs}, T, instances, stats);
}

// the leveled nodes, when their families are given; without them (lhe NULL) the call is thfhe_dag_run_mv_batch.
int thfhe_dag_run_lhe_batch(thfhe_ctx *c, thfhe_poly_ctx *pc, const int32_t *inputs, size_t n_inputs, const int32_t *nodes, size_t n_nodes,
                            const thfhe_lut_spec *specs, int n_specs, const int32_t *tv, int n_luts, const int32_t *enc_a, const int32_t *enc_b, int n_enc,
                            const thfhe_tree_spec *trees, int n_trees, const int32_t *tv1, int n_tv1_rows, const thfhe_mv_spec *mvs, int n_mvs,
                            const int32_t *mv_tv0, int n_bases, const int32_t *mv_factors, size_t n_factor_words, const thfhe_dag_lhe_families *lhe,
                            size_t instances, const int32_t *out_wires, size_t n_out, int32_t *outputs, int64_t *stats) {
    const DagFamilies T{kDagGenLut | kDagGenTree | kDagGenMv | (lhe ? kDagGenLhe : 0u), specs, n_specs, tv, n_luts, enc_a, enc_b, n_enc, trees, n_trees, tv1, n_tv1_rows,
                        mvs, n_mvs, mv_tv0, n_bases, mv_factors, n_factor_words, lhe};
    return sk_dag_run(c, pc, DagCall{inputs, n_inputs, nodes, n_nodes, out_wires, n_out, outputs}, T, instances, stats);
}

// the circuit-bootstrap nodes, when their family is given; without it (cb NULL) the call is thfhe_dag_run_lhe_batch.
int thfhe_dag_run_cb_batch(thfhe_ctx *c, thfhe_poly_ctx *pc, thfhe_mk_ctx *level2, const int32_t *inputs, size_t n_inputs, const int32_t *nodes, size_t n_nodes,
                           const thfhe_lut_spec *specs, int n_specs, const int32_t *tv, int n_luts, const int32_t *enc_a, const int32_t *enc_b, int n_enc,
                           const thfhe_tree_spec *trees, int n_trees, const int32_t *tv1, int n_tv1_rows, const thfhe_mv_spec *mvs, int n_mvs,
                           const int32_t *mv_tv0, int n_bases, const int32_t *mv_factors, size_t n_factor_words, const thfhe_dag_lhe_families *lhe,
                           const thfhe_dag_cb_families *cb, size_t instances, const int32_t *out_wires, size_t n_out, int32_t *outputs, int64_t *stats) {
    if (stats) stats[4] = 0;
    const DagFamilies T{kDagGenLut | kDagGenTree | kDagGenMv | (lhe ? kDagGenLhe : 0u) | (cb ? kDagGenCb : 0u), specs, n_specs, tv, n_luts, enc_a, enc_b, n_enc, trees,
                        n_trees, tv1, n_tv1_rows, mvs, n_mvs, mv_tv0, n_bases, mv_factors, n_factor_words, lhe, cb};
    return sk_dag_run(c, pc, DagCall{inputs, n_inputs, nodes, n_nodes, out_wires, n_out, outputs}, T, instances, stats, level2);
}

// the dense-layer nodes, when their family is given; without it (dense NULL) the call is thfhe_dag_run_cb_batch.
int thfhe_dag_run_dense_batch(thfhe_ctx *c, thfhe_poly_ctx *pc, thfhe_mk_ctx *level2, const int32_t *inputs, size_t n_inputs, const int32_t *nodes, size_t n_nodes,
                              const thfhe_lut_spec *specs, int n_specs, const int32_t *tv, int n_luts, const int32_t *enc_a, const int32_t *enc_b, int n_enc,
                              const thfhe_tree_spec *trees, int n_trees, const int32_t *tv1, int n_tv1_rows, const thfhe_mv_spec *mvs, int n_mvs,
                              const int32_t *mv_tv0, int n_bases, const int32_t *mv_factors, size_t n_factor_words, const thfhe_dag_lhe_families *lhe,
                              const thfhe_dag_cb_families *cb, const thfhe_dag_dense_families *dense, size_t instances, const int32_t *out_wires, size_t n_out,
                              int32_t *outputs, int64_t *stats) {
    if (stats) stats[4] = 0;
    const DagFamilies T{kDagGenLut | kDagGenTree | kDagGenMv | (lhe ? kDagGenLhe : 0u) | (cb ? kDagGenCb : 0u) | (dense ? kDagGenDense : 0u), specs, n_specs, tv, n_luts,
                        enc_a, enc_b, n_enc, trees, n_trees, tv1, n_tv1_rows, mvs, n_mvs, mv_tv0, n_bases, mv_factors, n_factor_words, lhe, cb, dense};
    return sk_dag_run(c, pc, DagCall{inputs, n_inputs, nodes, n_nodes, out_wires, n_out, outputs}, T, instances, stats, level2);
}

int thfhe_dag_cb_release(thfhe_ctx *c) {
    if (!c) return thfhe_fail(THFHE_E_INVALID, "null ctx");
    DevLock lk(*c);
    if (lk.rc) return lk.rc;
    THFHE_HIP(hipStreamSynchronize(c->stream));
    c->cb_sets.clear();
    c->dag_sets.clear();
    return THFHE_OK;
}

int thfhe_set_dag_slice(thfhe_ctx *c, size_t max_gates) { return ctx_set_dag_slice(c, max_gates); }

int thfhe_dag_run(thfhe_ctx *c, int32_t *wires, size_t n_inputs, const int32_t *gates, size_t n_gates, int64_t *stats) {
    return dag_gates_run(c, wires, n_inputs, gates, n_gates, stats, thfhe_dag_run_batch);
}

int thfhe_bootstrap_wo_keyswitch(thfhe_ctx *c, int32_t mu, const int32_t *x, int32_t *out_N1, size_t count) {
    if (!c || !x || !out_N1) return thfhe_fail(THFHE_E_INVALID, "null argument");
    if (count == 0) return THFHE_OK;
    const size_t words = count * c->rec_words();
    return ctx_staged(c, words, {x, nullptr, nullptr}, {words * sizeof(int32_t), 0, 0}, [&] {
        return enqueue_rotations(c, kOpIdentity, c->stage.in_ptr(0), c->stage.in_ptr(0), nullptr, count, 1, mu);
    }, c->d_u, out_N1, count * 1025 * sizeof(int32_t));
}

int thfhe_bootstrap(thfhe_ctx *c, int32_t mu, const int32_t *x, int32_t *out, size_t count) {
    if (!c || !x || !out) return thfhe_fail(THFHE_E_INVALID, "null argument");
    if (count == 0) return THFHE_OK;
    const size_t words = count * c->rec_words();
    return ctx_staged(c, words, {x, nullptr, nullptr}, {words * sizeof(int32_t), 0, 0}, [&] {
        int rc = enqueue_rotations(c, kOpIdentity, c->stage.in_ptr(0), c->stage.in_ptr(0), nullptr, count, 1, mu);
        return rc ? rc : enqueue_keyswitch(c, c->d_u.as<int32_t>(), c->stage.out_ptr(), count, 1, false);
    }, c->stage.out, out, words * sizeof(int32_t));
}

int thfhe_lut_bootstrap(thfhe_ctx *c, const thfhe_lut_spec *spec, const int32_t *tv, int n_luts, const int32_t *lut_index, const int32_t *in0,
                        const int32_t *in1, const int32_t *in2, int32_t *out, size_t count) {
    return lut_bootstrap(c, spec, tv, n_luts, lut_index, in0, in1, in2, out, count, true);
}

int thfhe_lut_bootstrap_wo_keyswitch(thfhe_ctx *c, const thfhe_lut_spec *spec, const int32_t *tv, int n_luts, const int32_t *lut_index,
                                     const int32_t *in0, const int32_t *in1, const int32_t *in2, int32_t *out_N1, size_t count) {
    return lut_bootstrap(c, spec, tv, n_luts, lut_index, in0, in1, in2, out_N1, count, false);
}

int thfhe_lut_bootstrap_enc(thfhe_ctx *c, const thfhe_lut_spec *spec, const int32_t *tv_a, const int32_t *tv_b, int n_luts, const int32_t *lut_index,
                            const int32_t *in0, const int32_t *in1, const int32_t *in2, int32_t *out, size_t count) {
    return lut_bootstrap(c, spec, tv_b, n_luts, lut_index, in0, in1, in2, out, count, true, true, tv_a);
}

int thfhe_lut_bootstrap_enc_wo_keyswitch(thfhe_ctx *c, const thfhe_lut_spec *spec, const int32_t *tv_a, const int32_t *tv_b, int n_luts,
                                         const int32_t *lut_index, const int32_t *in0, const int32_t *in1, const int32_t *in2, int32_t *out_N1,
                                         size_t count) {
    return lut_bootstrap(c, spec, tv_b, n_luts, lut_index, in0, in1, in2, out_N1, count, false, true, tv_a);
}

int thfhe_lwe_linear(thfhe_ctx *c, const int32_t *W, const int32_t *bias, int M, int K, const int32_t *in, int32_t *out, size_t count) {
    return linear(c, W, bias, M, K, false, 1, nullptr, 1, nullptr, in, out, count, false);
}

int thfhe_linear_lut_bootstrap(thfhe_ctx *c, const int32_t *W, const int32_t *bias, int M, int K, int theta, const int32_t *tv, int n_luts,
                               const int32_t *lut_index, const int32_t *in, int32_t *out, size_t count) {
    return linear(c, W, bias, M, K, true, theta, tv, n_luts, lut_index, in, out, count, true);
}

int thfhe_linear_lut_bootstrap_wo_keyswitch(thfhe_ctx *c, const int32_t *W, const int32_t *bias, int M, int K, int theta, const int32_t *tv, int n_luts,
                                            const int32_t *lut_index, const int32_t *in, int32_t *out_N1, size_t count) {
    return linear(c, W, bias, M, K, true, theta, tv, n_luts, lut_index, in, out_N1, count, false);
}

int thfhe_set_linear_slice(thfhe_ctx *c, size_t jobs) { return ctx_set_linear_slice(c, jobs); }

int thfhe_linear_last_timings(thfhe_ctx *c, float ms[3]) { return ctx_linear_last_timings(c, ms); }

int thfhe_linear_tile(int *tile_m, int *tile_k) { return linear_tile(tile_m, tile_k); }

int thfhe_set_tree_slice(thfhe_ctx *c, size_t max_candidates) {
    if (!c || max_candidates < 1 || max_candidates > ((size_t)1 << 20)) return thfhe_fail(THFHE_E_INVALID, "slice must be 1 .. 2^20 candidates");
    std::lock_guard<std::mutex> g(c->mu);
    c->tree_slice = max_candidates;
    return THFHE_OK;
}

int thfhe_tree_lut_bootstrap(thfhe_ctx *c, thfhe_poly_ctx *pc, const thfhe_lut_spec *spec_lo, const thfhe_lut_spec *spec_hi, int p_hi, const int32_t *tv1,
                             int n_tables, const int32_t *table_index, const int32_t *lo0, const int32_t *lo1, const int32_t *lo2, const int32_t *hi0,
                             const int32_t *hi1, const int32_t *hi2, int32_t *out, size_t count) {
    // host checks, before either context is looked at
    THFHE_TRY(tree_validate_rows(kTreeRules, spec_lo, spec_hi, p_hi, tv1, n_tables, table_index, lo0, lo1, lo2, hi0, hi1, hi2, out, count));
    return tree_bootstrap(c, pc, *spec_lo, *spec_hi, p_hi, tv1, (size_t)n_tables * (p_hi / spec_lo->theta), nullptr, 0, 0, table_index, lo0, lo1, lo2, hi0, hi1, hi2, out, count);
}

int thfhe_mv_lut_bootstrap(thfhe_ctx *c, const thfhe_lut_spec *spec, const int32_t *tv0, const int32_t *factors, int p, int q, int n_tables,
                           const int32_t *table_index, const int32_t *in0, const int32_t *in1, const int32_t *in2, int32_t *out, size_t count) {
    return mv_lut_bootstrap(c, spec, tv0, factors, p, q, n_tables, table_index, in0, in1, in2, out, count, true);
}

int thfhe_mv_lut_bootstrap_wo_keyswitch(thfhe_ctx *c, const thfhe_lut_spec *spec, const int32_t *tv0, const int32_t *factors, int p, int q, int n_tables,
                                        const int32_t *table_index, const int32_t *in0, const int32_t *in1, const int32_t *in2, int32_t *out_N1,
                                        size_t count) {
    return mv_lut_bootstrap(c, spec, tv0, factors, p, q, n_tables, table_index, in0, in1, in2, out_N1, count, false);
}

int thfhe_tree_lut_bootstrap_mv(thfhe_ctx *c, thfhe_poly_ctx *pc, const thfhe_lut_spec *spec_lo, const thfhe_lut_spec *spec_hi, int p_hi, int p_lo,
                                const int32_t *tv0, const int32_t *factors, int n_tables, const int32_t *table_index, const int32_t *lo0,
                                const int32_t *lo1, const int32_t *lo2, const int32_t *hi0, const int32_t *hi1, const int32_t *hi2, int32_t *out,
                                size_t count) {
    // host checks, before either context is looked at
    THFHE_TRY(tree_validate(kTreeRules, spec_lo, spec_hi, p_hi, tv0, lo0, lo1, lo2, hi0, hi1, hi2, out));
    if (!factors) return thfhe_fail(THFHE_E_INVALID, "null argument");
    THFHE_TRY(mv_validate(*spec_lo, p_lo, p_hi, n_tables));
    THFHE_TRY(tree_validate_index(table_index, n_tables, count));
    return tree_bootstrap(c, pc, *spec_lo, *spec_hi, p_hi, tv0, 1, factors, p_lo, n_tables, table_index, lo0, lo1, lo2, hi0, hi1, hi2, out, count);
}

int thfhe_tree_lut_bootstrap_mvk(thfhe_ctx *c, thfhe_poly_ctx *pc, const thfhe_lut_spec *spec_lo, const thfhe_lut_spec *spec_hi, int p_hi, int p_lo, int k,
                                 const int32_t *tv0, const int32_t *factors, int n_tables, const int32_t *table_index, const int32_t *lo0,
                                 const int32_t *lo1, const int32_t *lo2, const int32_t *hi0, const int32_t *hi1, const int32_t *hi2, int32_t *out,
                                 size_t count) {
    // host checks, before either context is looked at: those of thfhe_tree_lut_bootstrap_mv, then k and k p_hi
    THFHE_TRY(tree_validate(kTreeRules, spec_lo, spec_hi, p_hi, tv0, lo0, lo1, lo2, hi0, hi1, hi2, out));
    if (!factors) return thfhe_fail(THFHE_E_INVALID, "null argument");
    THFHE_TRY(mv_validate(*spec_lo, p_lo, p_hi, n_tables));
    THFHE_TRY(tree_validate_index(table_index, n_tables, count));
    THFHE_TRY(mvk_validate(p_hi, k));
    return tree_bootstrap(c, pc, *spec_lo, *spec_hi, p_hi, tv0, 1, factors, p_lo, n_tables, table_index, lo0, lo1, lo2, hi0, hi1, hi2, out, count, k);
}

int thfhe_keyswitch(thfhe_ctx *c, const int32_t *in_N1, int32_t *out, size_t count) {
    if (!c || !in_N1 || !out) return thfhe_fail(THFHE_E_INVALID, "null argument");
    if (count == 0) return THFHE_OK;
    DevLock lk(*c);
    if (lk.rc) return lk.rc;
    int rc = ensure_workspace(c, count);
    if (rc) return rc;
    rc = c->stage.grow(count * c->rec_words());
    if (rc) return rc;
    THFHE_HIP(hipMemcpyAsync(c->d_u.as<int32_t>(), in_N1, count * 1025 * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    rc = enqueue_keyswitch(c, c->d_u.as<int32_t>(), c->stage.out_ptr(), count, 1, false);
    if (rc) return rc;
    THFHE_HIP(hipMemcpyAsync(out, c->stage.out_ptr(), count * c->rec_words() * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    THFHE_HIP(hipStreamSynchronize(c->stream));
    return THFHE_OK;
}

int thfhe_tgsw_set_create(thfhe_ctx *c, const int32_t *tgsw, size_t count, int d, thfhe_tgsw_set **out) {
    return ctx_tgsw_set_create(c, tgsw, count, d, out, kLheRules, tgsw_set_fill);
}

void thfhe_tgsw_set_destroy(thfhe_tgsw_set *set) { ctx_tgsw_set_destroy(set); }

int thfhe_lhe_cmux(thfhe_ctx *c, const thfhe_tgsw_set *set, int bit, const int32_t *d1_a, const int32_t *d1_b, const int32_t *d0_a, const int32_t *d0_b,
                   int32_t *out_a, int32_t *out_b, size_t count) {
    return lhe_cmux(c, set, bit, d1_a, d1_b, d0_a, d0_b, out_a, out_b, count);
}

int thfhe_lhe_lookup(thfhe_ctx *c, const thfhe_tgsw_set *set, size_t first, size_t count, int d_tree, int d_rot, int theta, const int32_t *tab_a,
                     const int32_t *tab_b, int n_tables, const int32_t *table_index, int32_t *out) {
    return lhe_lookup(c, set, first, count, d_tree, d_rot, theta, tab_a, tab_b, n_tables, table_index, out, true);
}

int thfhe_lhe_lookup_wo_keyswitch(thfhe_ctx *c, const thfhe_tgsw_set *set, size_t first, size_t count, int d_tree, int d_rot, int theta,
                                  const int32_t *tab_a, const int32_t *tab_b, int n_tables, const int32_t *table_index, int32_t *out_N1) {
    return lhe_lookup(c, set, first, count, d_tree, d_rot, theta, tab_a, tab_b, n_tables, table_index, out_N1, false);
}

int thfhe_set_wfa_chunk(thfhe_ctx *c, int g) {
    if (!c || g < 0 || g > kWfaMaxStates) return thfhe_fail(THFHE_E_INVALID, "wfa chunk must be 0 (automatic) or 1 .. 64 states");
    std::lock_guard<std::mutex> lg(c->mu);
    c->wfa_chunk = g;
    return THFHE_OK;
}

int thfhe_lhe_wfa(thfhe_ctx *c, const thfhe_tgsw_set *const *sets, int n_sets, size_t first, size_t count, int n_steps, int n_states, const int32_t *trans,
                  const int32_t *step_bit, const int32_t *fin_a, const int32_t *fin_b, int n_tables, const int32_t *table_index, int theta,
                  const int32_t *start, int n_out, int32_t *out) {
    return lhe_wfa(c, sets, n_sets, first, count, n_steps, n_states, trans, step_bit, fin_a, fin_b, n_tables, table_index, theta, start, n_out, out, true);
}

int thfhe_lhe_wfa_wo_keyswitch(thfhe_ctx *c, const thfhe_tgsw_set *const *sets, int n_sets, size_t first, size_t count, int n_steps, int n_states,
                               const int32_t *trans, const int32_t *step_bit, const int32_t *fin_a, const int32_t *fin_b, int n_tables,
                               const int32_t *table_index, int theta, const int32_t *start, int n_out, int32_t *out_N1) {
    return lhe_wfa(c, sets, n_sets, first, count, n_steps, n_states, trans, step_bit, fin_a, fin_b, n_tables, table_index, theta, start, n_out, out_N1,
                   false);
}

int thfhe_lhe_demux(thfhe_ctx *c, const thfhe_tgsw_set *set, int bit, const int32_t *x_a, const int32_t *x_b, int32_t *out0_a, int32_t *out0_b,
                    int32_t *out1_a, int32_t *out1_b, size_t count) {
    return lhe_demux(c, set, bit, x_a, x_b, out0_a, out0_b, out1_a, out1_b, count);
}

int thfhe_lhe_scatter(thfhe_ctx *c, const thfhe_tgsw_set *set, size_t first, size_t count, int d_tree, int d_rot, const int32_t *val_a,
                      const int32_t *val_b, int n_vals, const int32_t *val_index, int n_tables, const int32_t *table_index, int32_t *tab_a,
                      int32_t *tab_b) {
    return lhe_scatter(c, set, first, count, d_tree, d_rot, val_a, val_b, n_vals, val_index, n_tables, table_index, tab_a, tab_b);
}

int thfhe_cb_key_set(thfhe_ctx *c, const int32_t *pks, int D, int t, int basebit) { return cb_key_set(c, pks, D, t, basebit); }

int thfhe_cb_private_keyswitch(thfhe_ctx *c, const int32_t *lwe2, size_t count, int32_t *tgsw) { return cb_private_keyswitch(c, lwe2, count, tgsw); }

int thfhe_cb_set_batch_threshold(thfhe_ctx *c, long min_inputs) {
    if (!c || min_inputs < 0) return thfhe_fail(THFHE_E_INVALID, "batch threshold must be 0 (the default) or a number of inputs");
    std::lock_guard<std::mutex> lg(c->mu);
    c->cb.batch_min = min_inputs ? min_inputs : kCbBatchMinInputs;
    return THFHE_OK;
}

int thfhe_circuit_bootstrap(thfhe_ctx *c, thfhe_mk_ctx *level2, const int32_t *lwe, size_t count, int d, int32_t *tgsw_words, thfhe_tgsw_set **out) {
    return circuit_bootstrap(c, level2, lwe, count, d, THFHE_CB_PER_LEVEL, tgsw_words, out);
}

int thfhe_circuit_bootstrap_mode(thfhe_ctx *c, thfhe_mk_ctx *level2, const int32_t *lwe, size_t count, int d, int mode, int32_t *tgsw_words,
                                 thfhe_tgsw_set **out) {
    return circuit_bootstrap(c, level2, lwe, count, d, mode, tgsw_words, out);
}

int thfhe_cb_stage_a(thfhe_ctx *c, thfhe_mk_ctx *level2, const int32_t *lwe, size_t count, int mode, int32_t *lwe2_out) {
    return cb_stage_a(c, level2, lwe, count, mode, lwe2_out);
}

}  // extern "C"
