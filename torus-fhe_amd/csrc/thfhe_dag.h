// thfhe_dag.h -- the gate-DAG front end shared by the single-key and the 3-gen multi-key engines:
// an ASAP levelising scheduler for the reference's circuits (src/KNN_medical_data.cpp:127-489, J/3gen_mk_gates.jl:183-362), and the
// gather / scatter kernels of the device-resident executor.
// The host side of an entry is three records and two functions.  DagCall: the inputs, the node rows, the wires to return.  DagFamilies: every table
// family a run can bring, with the generations of node kinds the entry admits (DagGen).  DagPlan: the schedule, launch groups of one DagClass each.
// dag_families_check: the checks that need no row; dag_plan: one row checker per node kind (DagRowChecks), then the levels and their groups.
//   kDagGenLut   LUT nodes (thfhe_dag_run_lut_batch, thfhe_mk_dag_run_lut_batch): programmable bootstraps among the gates, fed by the shared
//                prologue reading their operands from the wire table (LutWireSrc, thfhe_lut_prologue.h), their theta outputs scattered into consecutive wires
//   kDagGenTree  encrypted-table, select and tree nodes (thfhe_dag_run_tree_batch; single key)
//   kDagGenMv    multi-value nodes (thfhe_dag_run_mv_batch; thfhe_mk_dag_run_mv_batch): MV rows, and TREE_MV rows where the
//                entry has the tree generation too (single key)
//   kDagGenLhe   leveled nodes (thfhe_dag_run_lhe_batch; single key): LHE_LOOKUP, LHE_GATHER and LHE_WFA rows on the client's TGSW sets;
//                dag_lhe_gather_kernel stages a GATHER node's candidates for the box packing
//   kDagGenCb    circuit-bootstrap nodes (thfhe_dag_run_cb_batch; single key): CB rows, whose operands are a LIST of wires (a slice of the
//                run's wire pool) and whose result is a computed TGSW set that later leveled rows read (the group and its gather kernel: thfhe_dag_cb.h)
//   kDagGenDense dense-layer nodes (thfhe_dag_run_dense_batch, thfhe_mk_dag_run_dense_batch): DENSE rows, whose operands are a LIST of K
//                wires (a slice of the family's wire pool) and whose M theta records go to consecutive wires (the group: dag_run_dense_group,
//                thfhe_pbs_host.h; its kernel reads the wire table in place: LinWireSrc, thfhe_linear.h)
// The kinds from kDagGenTree on are planned here and run by the engine (thfhe_sk.hip: sk_dag_run_luts), a grouped kind in slices through dag_group_slices.
// dag_gates_run_batch / dag_gates_run are the four-column entries of both engines.
#ifndef THFHE_DAG_H
#define THFHE_DAG_H

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <initializer_list>
#include <map>
#include <set>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/thfhe_hip.h"
#include "thfhe_common.h"
#include "thfhe_devctx.h"
#include "thfhe_lut_prologue.h"

namespace {
using namespace thfhe;

// gate-DAG executor plumbing.  Wires live in one device table [instances][n_wires][words]: `instances` independent evaluations of
// the same gate list (the reference's loop over test records around one circuit, src/KNN_medical_data.cpp:676-691).  The gates of a
// level are numbered G = q * cnt + g (instance q, gate g of the level); a launch handles the slice [first, first + total) of them: its
// operands are gathered into the contiguous staging arrays the bootstrap kernels read, its outputs scattered back.
__global__ __launch_bounds__(256) void dag_gather_kernel(const int32_t *__restrict__ wires, const int32_t *__restrict__ idx, int32_t *__restrict__ dst,
                                                         long first, long total, long cnt, size_t n_wires, int words,
                                                         const int32_t *__restrict__ ops, int32_t *__restrict__ ops_out) {
    const long j = blockIdx.x;
    const int i = blockIdx.y * 256 + threadIdx.x;
    if (j >= total || i >= words) return;
    const long G = first + j, q = G / cnt, g = G - q * cnt;
    dst[j * words + i] = wires[((size_t)q * n_wires + idx[g]) * words + i];
    if (ops_out && i == 0) ops_out[j] = ops[g];   // per-gate opcodes of the slice, in staging order
}
__global__ __launch_bounds__(256) void dag_scatter_kernel(const int32_t *__restrict__ src, const int32_t *__restrict__ idx, int32_t *__restrict__ wires,
                                                          long first, long total, long cnt, size_t n_wires, int words) {
    const long j = blockIdx.x;
    const int i = blockIdx.y * 256 + threadIdx.x;
    if (j >= total || i >= words) return;
    const long G = first + j, q = G / cnt, g = G - q * cnt;
    wires[((size_t)q * n_wires + idx[g]) * words + i] = src[j * words + i];
}
// NOT / COPY gates of one sub-level (no gate of the launch reads another's output), every instance
__global__ __launch_bounds__(256) void dag_wire_linear_kernel(int32_t *__restrict__ wires, const int32_t *__restrict__ in_idx,
                                                              const int32_t *__restrict__ out_idx, const int32_t *__restrict__ ops, long total, long cnt,
                                                              size_t n_wires, int words) {
    const long G = blockIdx.x;
    const int i = blockIdx.y * 256 + threadIdx.x;
    if (G >= total || i >= words) return;
    const long q = G / cnt, g = G - q * cnt;
    const size_t base = (size_t)q * n_wires;
    const uint32_t v = (uint32_t)wires[(base + in_idx[g]) * words + i];
    wires[(base + out_idx[g]) * words + i] = (int32_t)(ops[g] == THFHE_NOT ? 0u - v : v);
}
// theta-record scatter of a LUT launch group: key-switched record r = j theta + t of the slice -> wire idx[g] + t of instance q
__global__ __launch_bounds__(256) void dag_scatter_theta_kernel(const int32_t *__restrict__ src, const int32_t *__restrict__ idx, int32_t *__restrict__ wires,
                                                                long first, long total, long cnt, size_t n_wires, int words, int theta) {
    const long r = blockIdx.x;
    const int i = blockIdx.y * 256 + threadIdx.x;
    if (r >= total * theta || i >= words) return;
    const long j = r / theta, t = r - j * theta, G = first + j, q = G / cnt, g = G - q * cnt;
    wires[((size_t)q * n_wires + idx[g] + t) * words + i] = src[r * words + i];
}
// Candidate gather of a SELECT group: candidate r = j p + k of the slice is wire t_first[g] + k of instance q -> dst[r], the [jobs p][words] buffer
// the box packing reads.  grid.y strides over the candidates.
__global__ __launch_bounds__(256) void dag_select_gather_kernel(const int32_t *__restrict__ wires, const int32_t *__restrict__ t_first, int32_t *__restrict__ dst,
                                                                long first, long total, long cnt, size_t n_wires, int words, int p) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= words) return;
    for (long r = blockIdx.y; r < total * p; r += gridDim.y) {
        const long j = r / p, k = r - j * p, G = first + j, q = G / cnt, g = G - q * cnt;
        dst[(size_t)r * words + i] = wires[((size_t)q * n_wires + t_first[g] + k) * words + i];
    }
}
// Candidate gather of one LHE_GATHER node over a slice of instances: candidate r = j P + k is wire first_wire + k of instance q0 + j -> dst[r], the
// [jobs P][words] buffer the box packing reads.  The P candidates of a job are consecutive wires, so a job is one contiguous copy of P records.
__global__ __launch_bounds__(256) void dag_lhe_gather_kernel(const int32_t *__restrict__ wires, int32_t *__restrict__ dst, long q0, long total, size_t n_wires,
                                                             int words, int first_wire, int P) {
    const long j = blockIdx.y;
    const size_t len = (size_t)P * words;
    if (j >= total) return;
    const int32_t *const src = wires + ((size_t)(q0 + j) * n_wires + first_wire) * words;
    int32_t *const out = dst + (size_t)j * len;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < len; i += (size_t)gridDim.x * 256) out[i] = src[i];
}

// The launch classes of the schedule.  0 .. 3 are the engine's gate classes, what its classify(op) returns.
enum DagClass : int32_t {
    kDagGate2 = 0,       // two-input bootstrapped gates, per-gate opcodes in one launch
    kDagMux = 1,         // MUX: two rotations per gate
    kDagLinear = 2,      // NOT / COPY: no bootstrap
    kDagGate3 = 3,       // three-input bootstrapped gates
    kDagLut1 = 4, kDagLut2 = 5, kDagLut4 = 6,     // LUT nodes of theta 1 / 2 / 4, index columns + [spec | lut]
    kDagLutOut = 7,      // LUT_OUT row: no launch, its wire is written by its head's scatter
    kDagEnc1 = 8, kDagEnc2 = 9, kDagEnc4 = 10,    // LUT_ENC nodes of theta 1 / 2 / 4: [spec | etab]
    // the grouped kinds: one launch group per entry of the family and level
    kDagSelect = 11,     // [tree | first], per trees[] entry
    kDagTree = 12,       // [tree | row0]
    kDagMv = 13,         // [mv | t], per mvs[] entry
    kDagTreeMv = 14,
    kDagLheLookup = 15,  // [lk | row0], per lks[] entry
    kDagLheGather = 16,  // [lk | first]
    kDagLheWfa = 17,     // [wfa | fin_row0], per wfas[] entry
    kDagCb = 18,         // [cbset | -], ONE group per level (entry -1), before the level's leveled groups; then int32[count][4] = (base, off, d, out wire)
    kDagDense = 19,      // [layer | -], per layers[] entry; the in0 column holds each node's wire_off, the out column its head wire
};
inline bool dag_class_leveled(int cls) { return cls >= kDagLheLookup && cls <= kDagLheWfa; }
// theta of a LUT / LUT_ENC class, 0 for every other class
inline int dag_class_theta(int cls) {
    switch (cls) {
    case kDagLut1: case kDagEnc1: return 1;
    case kDagLut2: case kDagEnc2: return 2;
    case kDagLut4: case kDagEnc4: return 4;
    default: return 0;
    }
}
inline int dag_lut_class(int theta, bool enc) { return theta == 1 ? (enc ? kDagEnc1 : kDagLut1) : (theta == 2 ? (enc ? kDagEnc2 : kDagLut2) : (enc ? kDagEnc4 : kDagLut4)); }

// One launch group of the schedule: `count` gates of one class whose operands are all available.
struct DagBatch {
    int32_t depth, sub, cls;  // cls: a DagClass
    size_t off, count;        // index table slice: [ops | in0 | in1 | in2 | out], classes from kDagLut1 on + [spec | lut], `count` entries each, at tab[off]
    int32_t tree = -1;        // the grouped kinds: the trees[] / mvs[] / lks[] / wfas[] entry the whole group shares
    size_t ext = 0, bits = 0; // a CB group: its node table int32[count][4] at tab[ext], and the d of its nodes together
};

// The arguments every thfhe_dag_run_*_batch entry has: the inputs, the node rows, the wires to return.
struct DagCall {
    const int32_t *inputs;      // int32[instances][n_inputs][words]
    size_t n_inputs;
    const int32_t *nodes;       // int32[n_nodes][4 or 6]
    size_t n_nodes;
    const int32_t *out_wires;   // wire ids to return (n_out of them) or null = every node's wire
    size_t n_out;
    int32_t *outputs;           // int32[instances][n_out or n_nodes][words]
};

// The generations of node kinds an entry admits.  An opcode of a generation the entry does not have is a gate opcode the engine does not define.
enum DagGen : unsigned {
    kDagGenLut = 1,    // six-column rows; THFHE_LUT and THFHE_LUT_OUT (thfhe_dag_run_lut_batch, thfhe_mk_dag_run_lut_batch)
    kDagGenTree = 2,   // THFHE_LUT_ENC, THFHE_SELECT, THFHE_TREE; every family may be absent (thfhe_dag_run_tree_batch)
    kDagGenMv = 4,     // THFHE_MV; with kDagGenTree also THFHE_TREE_MV (thfhe_dag_run_mv_batch; thfhe_mk_dag_run_mv_batch has no tree generation)
    kDagGenLhe = 8,    // THFHE_LHE_LOOKUP, THFHE_LHE_GATHER, THFHE_LHE_WFA (thfhe_dag_run_lhe_batch with its families)
    kDagGenCb = 16,    // THFHE_CB (thfhe_dag_run_cb_batch with its family)
    kDagGenDense = 32, // THFHE_DENSE (thfhe_dag_run_dense_batch, thfhe_mk_dag_run_dense_batch with their family)
};
// Everything a run can bring besides its DagCall: the table families (host pointers) with their counts.  An entry fills the families it has and the
// generations it admits; none (gens = 0) is a run of four-column gate rows.  After dag_families_check a family without a pointer has count 0.
struct DagFamilies {
    unsigned gens = 0;   // DagGen bits; the members below in the order of the entries' arguments
    const thfhe_lut_spec *specs = nullptr;
    int n_specs = 0;
    const void *tv = nullptr;                           // [n_luts][N] test vectors of the ring's torus: int32 single key, int64 multi key
    int n_luts = 0;
    const int32_t *enc_a = nullptr, *enc_b = nullptr;   // [n_enc][N] encrypted tables: masks, bodies
    int n_enc = 0;
    const thfhe_tree_spec *trees = nullptr;
    int n_trees = 0;
    const int32_t *tv1 = nullptr;                       // [n_tv1_rows][N] level-1 rows
    int n_tv1_rows = 0;
    const thfhe_mv_spec *mvs = nullptr;
    int n_mvs = 0;
    const void *mv_tv0 = nullptr;                       // [n_bases][N] base vectors of the ring's torus, as tv
    int n_bases = 0;
    const int32_t *mv_factors = nullptr;                // the taps of every mvs[] entry
    size_t n_factor_words = 0;
    const thfhe_dag_lhe_families *lhe = nullptr;        // the leveled families, with kDagGenLhe
    const thfhe_dag_cb_families *cb = nullptr;          // the computed sets, with kDagGenCb
    const thfhe_dag_dense_families *dense = nullptr;    // the dense layers, with kDagGenDense
    int n_client_sets() const { return lhe ? lhe->n_sets : 0; }
    int n_computed_sets() const { return cb ? cb->n_sets : 0; }
    // d of set `s` of the run when the host knows it: a computed set's; -1 for a client set
    int computed_d(int s) const { return s >= n_client_sets() ? cb->sets[s - n_client_sets()].d : -1; }
};

// the rules a multi-value rotation adds to lut_spec_check's: theta 1, p taps, q outputs, the table count (thfhe_mv_lut_bootstrap)
inline int mv_validate(const thfhe_lut_spec &sp, int p, int q, int n_tables) {
    if (sp.theta != 1) return thfhe_fail(THFHE_E_INVALID, "multi-value: the spec's theta must be 1");
    if (p < 2 || p > 64 || (p & (p - 1))) return thfhe_fail(THFHE_E_INVALID, "multi-value: p must be a power of two in 2 .. 64");
    if (q < 1 || q > 64) return thfhe_fail(THFHE_E_INVALID, "multi-value: q must be 1 .. 64");
    if (n_tables < 1 || n_tables > 1024) return thfhe_fail(THFHE_E_INVALID, "multi-value: n_tables must be 1 .. 1024");
    return THFHE_OK;
}
// ... and a k-output tree on it (thfhe_tree_lut_bootstrap_mvk): p_hi a power of two within the rotation's 64 outputs (the flat entry's
// tree_validate and mv_validate have refused a bad one before; the DAG planner comes here first), k tables per sample, k p_hi outputs in all
inline int mvk_validate(int p_hi, int k) {
    if (p_hi < 2 || p_hi > 64 || (p_hi & (p_hi - 1))) return thfhe_fail(THFHE_E_INVALID, "multi-value tree: p_hi must be a power of two in 2 .. 64");
    if (k < 1) return thfhe_fail(THFHE_E_INVALID, "multi-value tree: k must be at least 1");
    if ((long)k * p_hi > 64) return thfhe_fail(THFHE_E_INVALID, "multi-value tree: k p_hi must be at most 64 (the outputs of one rotation)");
    return THFHE_OK;
}
// One mvs[] entry as an MV row (tree = false) or a TREE_MV row uses it: the flat entries' rules, then its base row and its slice of the factor array.
inline int dag_mv_spec_check(const DagFamilies &F, const thfhe_mv_spec &m, bool tree) {
    THFHE_TRY(lut_spec_check(m.lo));
    if (tree) {
        THFHE_TRY(lut_spec_check(m.hi));
        if (m.hi.theta != 1) return thfhe_fail(THFHE_E_INVALID, "tree: spec_hi theta must be 1 (the packed table holds one function)");
        THFHE_TRY(mvk_validate(m.q, m.k));
        THFHE_TRY(mv_validate(m.lo, m.p, m.k * m.q, m.n_tables));
    } else {
        if (m.k != 1) return thfhe_fail(THFHE_E_INVALID, "MV node: the spec's k must be 1");
        THFHE_TRY(mv_validate(m.lo, m.p, m.q, m.n_tables));
    }
    if (F.n_bases < 1) return thfhe_fail(THFHE_E_INVALID, "MV / TREE_MV node: no base vectors given (null table family)");
    if (m.base < 0 || m.base >= F.n_bases) return thfhe_fail(THFHE_E_INVALID, "MV / TREE_MV node: base out of range (0 .. n_bases-1)");
    if (F.n_factor_words < 1) return thfhe_fail(THFHE_E_INVALID, "MV / TREE_MV node: no factors given (null table family)");
    if (m.factors_off < 0 || (size_t)m.factors_off + (size_t)m.n_tables * m.k * m.q * m.p > F.n_factor_words)
        return thfhe_fail(THFHE_E_INVALID, "MV / TREE_MV node: factors_off + n_tables k q p out of range (0 .. n_factor_words)");
    return THFHE_OK;
}

// One lks[] entry as a LOOKUP row (gather = false) or a GATHER row uses it: the rules of thfhe_lhe_lookup that need no set, then the node kind's own.
inline int dag_lhe_spec_check(const thfhe_dag_lhe_families &F, const thfhe_dag_lhe_spec &k, bool gather, int n_computed = 0) {
    if (k.d_tree < 0 || k.d_tree > 6) return thfhe_fail(THFHE_E_INVALID, "leveled node: d_tree must be 0 .. 6");
    if (k.d_rot < 0 || k.d_rot > 10) return thfhe_fail(THFHE_E_INVALID, "leveled node: d_rot must be 0 .. 10");
    if (k.theta != 1 && k.theta != 2 && k.theta != 4) return thfhe_fail(THFHE_E_INVALID, "leveled node: theta must be 1, 2 or 4");
    if (k.theta > (1024 >> k.d_rot)) return thfhe_fail(THFHE_E_INVALID, "leveled node: theta must not exceed box = N >> d_rot");
    if (gather && k.theta != 1) return thfhe_fail(THFHE_E_INVALID, "LHE_GATHER node: the spec's theta must be 1 (a packed box holds one value)");
    if (gather && (k.d_rot < 1 || k.d_rot > 9)) return thfhe_fail(THFHE_E_INVALID, "LHE_GATHER node: d_rot must be 1 .. 9 (the box packing's p = 2^d_rot)");
    if (F.n_sets + n_computed < 1) return thfhe_fail(THFHE_E_INVALID, "leveled node: no tgsw sets given (null family)");
    if (k.set < 0 || k.set >= F.n_sets + n_computed) return thfhe_fail(THFHE_E_INVALID, "leveled node: the spec's set is out of range (0 .. n_sets-1)");
    return THFHE_OK;
}
// One wfas[] entry: the rules of thfhe_lhe_wfa that need no set, its sets within sets[], its three slices of the word pool and their entries.
inline int dag_wfa_spec_check(const thfhe_dag_lhe_families &F, const thfhe_dag_wfa_spec &a, int n_computed = 0) {
    if (a.n_sets < 1 || a.n_sets > 64) return thfhe_fail(THFHE_E_INVALID, "LHE_WFA node: the spec's n_sets must be 1 .. 64");
    if (a.n_steps < 1 || a.n_steps > 4096) return thfhe_fail(THFHE_E_INVALID, "LHE_WFA node: n_steps must be 1 .. 4096");
    if (a.n_states < 1 || a.n_states > 64) return thfhe_fail(THFHE_E_INVALID, "LHE_WFA node: n_states must be 1 .. 64");
    if (a.n_out < 1 || a.n_out > 64) return thfhe_fail(THFHE_E_INVALID, "LHE_WFA node: n_out must be 1 .. 64");
    if (a.theta != 1 && a.theta != 2 && a.theta != 4) return thfhe_fail(THFHE_E_INVALID, "LHE_WFA node: theta must be 1, 2 or 4");
    if (F.n_sets + n_computed < 1) return thfhe_fail(THFHE_E_INVALID, "leveled node: no tgsw sets given (null family)");
    if (a.set0 < 0 || (long)a.set0 + a.n_sets > F.n_sets + n_computed) return thfhe_fail(THFHE_E_INVALID, "LHE_WFA node: set0 + n_sets out of range (0 .. n_sets)");
    if (!F.wfa_words) return thfhe_fail(THFHE_E_INVALID, "LHE_WFA node: no word pool given (null family)");
    const size_t n_trans = (size_t)a.n_steps * a.n_states * 2;
    if (a.trans_off < 0 || (size_t)a.trans_off + n_trans > F.n_wfa_words || a.step_off < 0 || (size_t)a.step_off + a.n_steps > F.n_wfa_words ||
        a.start_off < 0 || (size_t)a.start_off + a.n_out > F.n_wfa_words)
        return thfhe_fail(THFHE_E_INVALID, "LHE_WFA node: a pool offset runs past n_wfa_words");
    for (size_t i = 0; i < n_trans; i++)
        if (F.wfa_words[a.trans_off + i] < 0 || F.wfa_words[a.trans_off + i] >= a.n_states)
            return thfhe_fail(THFHE_E_INVALID, "LHE_WFA node: trans entry out of range (0 .. n_states-1)");
    for (int o = 0; o < a.n_out; o++)
        if (F.wfa_words[a.start_off + o] < 0 || F.wfa_words[a.start_off + o] >= a.n_states)
            return thfhe_fail(THFHE_E_INVALID, "LHE_WFA node: start entry out of range (0 .. n_states-1)");
    return THFHE_OK;
}

// One layers[] entry: the limits of thfhe_lwe_linear and of theta, and its three slices of the word pool.
inline int dag_dense_spec_check(const thfhe_dag_dense_families &D, const thfhe_dag_dense_spec &l) {
    if (l.M < 1 || l.M > 65536 || l.K < 1 || l.K > 65536) return thfhe_fail(THFHE_E_INVALID, "dense: M and K must be 1 .. 65536");
    if (l.theta != 1 && l.theta != 2 && l.theta != 4) return thfhe_fail(THFHE_E_INVALID, "dense: theta must be 1, 2 or 4");
    if (l.w_off < 0 || (size_t)l.w_off + (size_t)l.M * l.K > D.n_words) return thfhe_fail(THFHE_E_INVALID, "dense: w_off + M K runs past n_words");
    if (l.bias_off < -1 || (l.bias_off >= 0 && (size_t)l.bias_off + l.M > D.n_words)) return thfhe_fail(THFHE_E_INVALID, "dense: bias_off + M runs past n_words");
    if (l.lut_off < -1 || (l.lut_off >= 0 && (size_t)l.lut_off + l.M > D.n_words)) return thfhe_fail(THFHE_E_INVALID, "dense: lut_off + M runs past n_words");
    return THFHE_OK;
}

// One family of a run: whether its pointer is given, its count, and the range of the count when it is.
struct DagFamilyRule {
    bool have;
    long long n, min, max;
    const char *range_msg;
};
// The families of one generation: a count without its pointer first, whichever family has it, then every count against its range in order.
inline int dag_family_rules(std::initializer_list<DagFamilyRule> rules, const char *null_msg) {
    for (const DagFamilyRule &r : rules)
        if (!r.have && r.n) return thfhe_fail(THFHE_E_INVALID, null_msg);
    for (const DagFamilyRule &r : rules)
        if (r.have && (r.n < r.min || r.n > r.max)) return thfhe_fail(THFHE_E_INVALID, r.range_msg);
    return THFHE_OK;
}
// The host checks of a six-column entry that need no row, before any device work and before a context is looked at: the call's pointers; per
// generation of families a count without its pointer, then the counts (a family without a pointer has count 0 from here on); every spec (the rules
// of lut_validate) and every tree spec's `hi` half and p_hi (the rules of thfhe_tree_lut_bootstrap; the `lo` half, and an mvs[] / lks[] / wfas[]
// entry, when a row uses it); the output wire ids.  The LUT entries (kDagGenLut alone) require specs and tv; from thfhe_dag_run_tree_batch and
// thfhe_mk_dag_run_mv_batch on every family may be absent.
inline int dag_families_check(const DagCall &A, const DagFamilies &F) {
    const bool strict = !(F.gens & (kDagGenTree | kDagGenMv));
    if ((!A.inputs && A.n_inputs) || (!A.nodes && A.n_nodes) || (!A.outputs && A.n_nodes) || (!A.out_wires && A.n_out) || (strict && (!F.specs || !F.tv)))
        return thfhe_fail(THFHE_E_INVALID, "null argument");
    const char *const null_msg = "null argument: a table family with a count but no pointer";
    THFHE_TRY(dag_family_rules({{F.specs != nullptr, F.n_specs, 1, 1024, strict ? "n_specs must be 1 .. 1024" : "n_specs must be 1 .. 1024 (0 with specs = NULL)"},
                                {F.tv != nullptr, F.n_luts, 1, 1024, strict ? "n_luts must be 1 .. 1024" : "n_luts must be 1 .. 1024 (0 with tv = NULL)"},
                                {F.enc_a && F.enc_b, F.n_enc, 0, 1 << 18, "n_enc must be 1 .. 262144 (0 with enc_a = enc_b = NULL)"},
                                {F.trees != nullptr, F.n_trees, 1, 1024, "n_trees must be 1 .. 1024 (0 with trees = NULL)"},
                                {F.tv1 != nullptr, F.n_tv1_rows, 1, 1 << 18, "n_tv1_rows must be 1 .. 262144 (0 with tv1 = NULL)"}},
                               null_msg));
    THFHE_TRY(dag_family_rules({{F.mvs != nullptr, F.n_mvs, 1, 1024, "n_mvs must be 1 .. 1024 (0 with mvs = NULL)"},
                                {F.mv_tv0 != nullptr, F.n_bases, 1, 1024, "n_bases must be 1 .. 1024 (0 with mv_tv0 = NULL)"},
                                {F.mv_factors != nullptr, (long long)F.n_factor_words, 1, 1 << 28, "n_factor_words must be 1 .. 2^28 (0 with mv_factors = NULL)"}},
                               null_msg));
    if (const thfhe_dag_lhe_families *const L = F.lhe) {
        const char *const lhe_null_msg = "null argument: a leveled family with a count but no pointer";
        if ((!L->tab_b && L->tab_a) || (!L->fin_b && L->fin_a)) return thfhe_fail(THFHE_E_INVALID, lhe_null_msg);   // masks without bodies
        THFHE_TRY(dag_family_rules({{L->sets != nullptr, L->n_sets, 1, 64, "lhe: n_sets must be 1 .. 64 (0 with sets = NULL)"},
                                    {L->lks != nullptr, L->n_lks, 1, 1024, "lhe: n_lks must be 1 .. 1024 (0 with lks = NULL)"},
                                    {L->wfas != nullptr, L->n_wfas, 1, 1024, "lhe: n_wfas must be 1 .. 1024 (0 with wfas = NULL)"},
                                    {L->tab_b != nullptr, L->n_tab_rows, 1, 1 << 18, "lhe: n_tab_rows must be 1 .. 262144 (0 with tab_b = NULL)"},
                                    {L->fin_b != nullptr, L->n_fin_rows, 1, 1 << 18, "lhe: n_fin_rows must be 1 .. 262144 (0 with fin_b = NULL)"},
                                    {L->wfa_words != nullptr, (long long)L->n_wfa_words, 1, 1 << 28, "lhe: n_wfa_words must be 1 .. 2^28 (0 with wfa_words = NULL)"}},
                                   lhe_null_msg));
    }
    if (const thfhe_dag_cb_families *const B = F.cb) {
        if (B->mode != THFHE_CB_PER_LEVEL && B->mode != THFHE_CB_ONE_ROTATION)
            return thfhe_fail(THFHE_E_INVALID, "circuit bootstrap: mode must be THFHE_CB_PER_LEVEL or THFHE_CB_ONE_ROTATION");
        if (!B->sets || B->n_sets < 1 || B->n_sets > 64) return thfhe_fail(THFHE_E_INVALID, "cb: n_sets must be 1 .. 64");
        if (F.n_client_sets() + B->n_sets > 64) return thfhe_fail(THFHE_E_INVALID, "cb: client sets + computed sets must be at most 64");
        if (!B->cb_wires && B->n_cb_wires) return thfhe_fail(THFHE_E_INVALID, "null argument: a wire pool with a count but no pointer");
        for (int s = 0; s < B->n_sets; s++) {
            if (B->sets[s].d < 1 || B->sets[s].d > 16) return thfhe_fail(THFHE_E_INVALID, "cb: d must be 1 .. 16");
            if (B->sets[s].wire_off < 0 || (size_t)B->sets[s].wire_off + B->sets[s].d > B->n_cb_wires)
                return thfhe_fail(THFHE_E_INVALID, "cb: wire_off + d runs past the wire pool");
        }
    }
    if (const thfhe_dag_dense_families *const D = F.dense) {
        THFHE_TRY(dag_family_rules({{D->layers != nullptr, D->n_layers, 1, 1024, "dense: n_layers must be 1 .. 1024"},
                                    {D->words != nullptr, (long long)D->n_words, 1, 1 << 28, "dense: n_words must be 1 .. 2^28"},
                                    {D->wires != nullptr, (long long)D->n_wires, 0, INT32_MAX, "dense: n_wires out of range"}},
                                   "null argument: a dense family with a count but no pointer"));
        if (!D->layers) return thfhe_fail(THFHE_E_INVALID, "dense: n_layers must be 1 .. 1024");
        if (!D->words) return thfhe_fail(THFHE_E_INVALID, "dense: n_words must be 1 .. 2^28");
        for (int t = 0; t < D->n_layers; t++) THFHE_TRY(dag_dense_spec_check(*D, D->layers[t]));
    }
    for (int s = 0; s < F.n_specs; s++)
        THFHE_TRY(lut_spec_check(F.specs[s]));
    for (int t = 0; t < F.n_trees; t++) {
        THFHE_TRY(lut_spec_check(F.trees[t].hi));
        if (F.trees[t].hi.theta != 1) return thfhe_fail(THFHE_E_INVALID, "tree: spec_hi theta must be 1 (the packed table holds one function)");
        const int p_hi = F.trees[t].p_hi;
        if (p_hi < 2 || p_hi > 512 || (p_hi & (p_hi - 1))) return thfhe_fail(THFHE_E_INVALID, "tree: p_hi must be a power of two in 2 .. N/2");
    }
    for (size_t s = 0; s < A.n_out; s++)
        if (A.out_wires[s] < 0 || (size_t)A.out_wires[s] >= A.n_inputs + A.n_nodes) return thfhe_fail(THFHE_E_INVALID, "output wire id out of range");
    return THFHE_OK;
}

// What a row checker makes of its row.
struct DagRow {
    int cls = kDagLutOut;
    int32_t entry = -1;                       // the grouped kinds: the family entry the row's group shares (row field 4)
    int nin = 0;                              // wire operands, row fields 1 .. nin
    int32_t cand_first = 0, cand_count = 0;   // SELECT / GATHER: the candidate wires; they count for the depth as operands do
    int outs = 0;                             // LUT_OUT rows due after the row
    const int32_t *list = nullptr;            // CB: the operand list, list_count pool wires; they count for the depth as candidates do
    int32_t list_count = 0;
    int32_t set_first = 0, set_count = 0;     // leveled rows: the sets of the run the row reads; a computed one gives the row its depth.  CB: the set it defines
};

// The row checks of a run, one checker per node kind; each fills the DagRow of a row it accepts.
struct DagRowChecks {
    const DagFamilies &F;
    std::set<std::pair<int, int32_t>> checked;   // (class, entry): the family entries that have had the checks a kind makes once per entry

    bool first_use(int cls, int32_t entry) { return checked.insert({cls, entry}).second; }
    static int operands_match(const int32_t *row, int nin, const char *msg) {
        for (int q = 0; q < 3; q++)
            if ((q < nin) != (row[1 + q] != -1)) return thfhe_fail(THFHE_E_INVALID, msg);
        return THFHE_OK;
    }
    static int no_operands(const int32_t *row) {
        if (row[1] != -1 || row[2] != -1 || row[3] != -1) return thfhe_fail(THFHE_E_INVALID, "leveled node: the operand fields must be -1");
        return THFHE_OK;
    }
    static int candidates(DagRow &r, int32_t first, int32_t count, int32_t w, const char *msg) {
        if (first < 0 || (long)first + count > (long)w) return thfhe_fail(THFHE_E_INVALID, msg);
        r.cand_first = first, r.cand_count = count;
        return THFHE_OK;
    }

    template <typename Classify>
    int gate(const int32_t *row, Classify classify, DagRow &r) const {
        r.cls = classify(row[0]);
        if (r.cls < 0) return thfhe_fail(THFHE_E_INVALID, "gate opcode not defined for this engine");
        if (F.gens && (row[4] != -1 || row[5] != -1)) return thfhe_fail(THFHE_E_INVALID, "gate row: spec and lut must be -1");
        r.nin = r.cls == kDagLinear ? 1 : (r.cls == kDagGate2 ? 2 : 3);
        return THFHE_OK;
    }
    // (LUT_OUT, head, -1, -1, -1, -1): one of the `pending` rows due after the node of wire `head`
    static int lut_out(const int32_t *row, int32_t head, int pending) {
        if (pending == 0) return thfhe_fail(THFHE_E_INVALID, "LUT_OUT row without a LUT node before it (extra or misplaced LUT_OUT row)");
        if (row[1] != head) return thfhe_fail(THFHE_E_INVALID, "LUT_OUT row names the wrong head (it must name its LUT node's wire)");
        if (row[2] != -1 || row[3] != -1 || row[4] != -1 || row[5] != -1) return thfhe_fail(THFHE_E_INVALID, "LUT_OUT row: fields after the head must be -1");
        return THFHE_OK;
    }
    // (LUT | LUT_ENC, operands, spec, lut | etab)
    int lut(const int32_t *row, bool enc, DagRow &r) const {
        if (!F.specs || (!enc && F.n_luts == 0))
            return thfhe_fail(THFHE_E_INVALID, enc ? "LUT_ENC node: no specs given (null table family)" : "LUT node: no specs or no tables given (null table family)");
        if (enc && F.n_enc < 1) return thfhe_fail(THFHE_E_INVALID, "LUT_ENC node: n_enc must be 1 .. 262144 (null table family)");
        if (row[4] < 0 || row[4] >= F.n_specs) return thfhe_fail(THFHE_E_INVALID, "LUT node: spec index out of range (0 .. n_specs-1)");
        if (!enc && (row[5] < 0 || row[5] >= F.n_luts)) return thfhe_fail(THFHE_E_INVALID, "LUT node: table index out of range (0 .. n_luts-1)");
        if (enc && (row[5] < 0 || row[5] >= F.n_enc)) return thfhe_fail(THFHE_E_INVALID, "LUT_ENC node: etab out of range (0 .. n_enc-1)");
        const thfhe_lut_spec &sp = F.specs[row[4]];
        THFHE_TRY(operands_match(row, sp.n_inputs, "LUT node: operands do not match the spec's n_inputs (unused ones are -1)"));
        r.cls = dag_lut_class(sp.theta, enc), r.nin = sp.n_inputs, r.outs = sp.theta - 1;
        return THFHE_OK;
    }
    // (SELECT, index operands, tree, first candidate wire) / (TREE, lo then hi operands, tree, row0); w: the row's own wire
    int tree(const int32_t *row, int32_t w, bool is_tree, DagRow &r) {
        if (!F.trees) return thfhe_fail(THFHE_E_INVALID, "SELECT / TREE node: no tree specs given (null table family)");
        if (row[4] < 0 || row[4] >= F.n_trees) return thfhe_fail(THFHE_E_INVALID, "SELECT / TREE node: tree index out of range (0 .. n_trees-1)");
        const thfhe_tree_spec &ts = F.trees[row[4]];
        r.cls = is_tree ? kDagTree : kDagSelect, r.entry = row[4], r.nin = ts.hi.n_inputs;
        if (is_tree) {
            if (first_use(kDagTree, row[4])) {   // the `lo` half: a SELECT ignores it
                THFHE_TRY(lut_spec_check(ts.lo));
                if (ts.p_hi % ts.lo.theta) return thfhe_fail(THFHE_E_INVALID, "tree: spec_lo theta must divide p_hi");
            }
            r.nin += ts.lo.n_inputs;
            if (r.nin > 3) return thfhe_fail(THFHE_E_INVALID, "TREE node: lo and hi operands exceed three");
            if (F.n_tv1_rows < 1) return thfhe_fail(THFHE_E_INVALID, "TREE node: no level-1 rows given (null table family)");
            if (row[5] < 0 || (long)row[5] + ts.p_hi / ts.lo.theta > F.n_tv1_rows)
                return thfhe_fail(THFHE_E_INVALID, "TREE node: row0 + R out of range (0 .. n_tv1_rows)");
        } else {
            THFHE_TRY(candidates(r, row[5], ts.p_hi, w, "SELECT node: candidate is not an earlier wire (first .. first + p - 1 must all be defined above)"));
        }
        return operands_match(row, r.nin, is_tree ? "TREE node: operands do not match lo.n_inputs + hi.n_inputs (unused ones are -1)"
                                                  : "SELECT node: operands do not match hi.n_inputs (unused ones are -1)");
    }
    // (MV, operands, mv, t) / (TREE_MV, lo then hi operands, mv, t)
    int mv(const int32_t *row, bool is_tree, DagRow &r) {
        if (!F.mvs) return thfhe_fail(THFHE_E_INVALID, "MV / TREE_MV node: no multi-value specs given (null table family)");
        if (row[4] < 0 || row[4] >= F.n_mvs) return thfhe_fail(THFHE_E_INVALID, "MV / TREE_MV node: mv index out of range (0 .. n_mvs-1)");
        const thfhe_mv_spec &m = F.mvs[row[4]];
        r.cls = is_tree ? kDagTreeMv : kDagMv, r.entry = row[4];
        if (first_use(r.cls, row[4])) THFHE_TRY(dag_mv_spec_check(F, m, is_tree));
        if (row[5] < 0 || row[5] >= m.n_tables) return thfhe_fail(THFHE_E_INVALID, "MV / TREE_MV node: table index out of range (0 .. n_tables-1)");
        r.nin = m.lo.n_inputs + (is_tree ? m.hi.n_inputs : 0), r.outs = (is_tree ? m.k : m.q) - 1;
        if (r.nin > 3) return thfhe_fail(THFHE_E_INVALID, "TREE_MV node: lo and hi operands exceed three");
        return operands_match(row, r.nin, is_tree ? "TREE_MV node: operands do not match lo.n_inputs + hi.n_inputs (unused ones are -1)"
                                                  : "MV node: operands do not match lo.n_inputs (unused ones are -1)");
    }
    // (LHE_LOOKUP, -1, -1, -1, lk, row0) / (LHE_GATHER, -1, -1, -1, lk, first candidate wire)
    int lookup(const int32_t *row, int32_t w, bool gather, DagRow &r) {
        const thfhe_dag_lhe_families &L = *F.lhe;
        THFHE_TRY(no_operands(row));
        if (!L.lks) return thfhe_fail(THFHE_E_INVALID, "LHE_LOOKUP / LHE_GATHER node: no lookup specs given (null family)");
        if (row[4] < 0 || row[4] >= L.n_lks) return thfhe_fail(THFHE_E_INVALID, "LHE_LOOKUP / LHE_GATHER node: lk out of range (0 .. n_lks-1)");
        const thfhe_dag_lhe_spec &ls = L.lks[row[4]];
        r.cls = gather ? kDagLheGather : kDagLheLookup, r.entry = row[4];
        if (first_use(r.cls, row[4])) {
            THFHE_TRY(dag_lhe_spec_check(L, ls, gather, F.n_computed_sets()));
            if (F.computed_d(ls.set) >= 0 && ls.d_tree + ls.d_rot != F.computed_d(ls.set))
                return thfhe_fail(THFHE_E_INVALID, "leveled node: d_tree + d_rot must equal the set's d");
        }
        r.set_first = ls.set, r.set_count = 1;
        if (gather)
            return candidates(r, row[5], (int32_t)1 << (ls.d_tree + ls.d_rot), w,
                              "LHE_GATHER node: candidate is not an earlier wire (first .. first + 2^d - 1 must all be defined above)");
        if (!L.tab_b || L.n_tab_rows < 1) return thfhe_fail(THFHE_E_INVALID, "LHE_LOOKUP node: no table rows given (null family)");
        if (row[5] < 0 || (long)row[5] + (1L << ls.d_tree) > L.n_tab_rows)
            return thfhe_fail(THFHE_E_INVALID, "LHE_LOOKUP node: row0 + 2^d_tree out of range (0 .. n_tab_rows)");
        r.outs = ls.theta - 1;
        return THFHE_OK;
    }
    // (LHE_WFA, -1, -1, -1, wfa, fin_row0)
    int wfa(const int32_t *row, DagRow &r) {
        const thfhe_dag_lhe_families &L = *F.lhe;
        THFHE_TRY(no_operands(row));
        if (!L.wfas) return thfhe_fail(THFHE_E_INVALID, "LHE_WFA node: no automaton specs given (null family)");
        if (row[4] < 0 || row[4] >= L.n_wfas) return thfhe_fail(THFHE_E_INVALID, "LHE_WFA node: wfa out of range (0 .. n_wfas-1)");
        const thfhe_dag_wfa_spec &a = L.wfas[row[4]];
        r.cls = kDagLheWfa, r.entry = row[4];
        if (first_use(kDagLheWfa, row[4])) THFHE_TRY(dag_wfa_spec_check(L, a, F.n_computed_sets()));
        r.set_first = a.set0, r.set_count = a.n_sets;
        if (!L.fin_b || L.n_fin_rows < 1) return thfhe_fail(THFHE_E_INVALID, "LHE_WFA node: no final weights given (null family)");
        if (row[5] < 0 || (long)row[5] + a.n_states > L.n_fin_rows)
            return thfhe_fail(THFHE_E_INVALID, "LHE_WFA node: fin_row0 + n_states out of range (0 .. n_fin_rows)");
        r.outs = a.n_out * a.theta - 1;
        return THFHE_OK;
    }
    // (CB, -1, -1, -1, cbset, -1); w: the row's own wire
    int cb(const int32_t *row, int32_t w, DagRow &r) const {
        const thfhe_dag_cb_families &B = *F.cb;
        if (row[1] != -1 || row[2] != -1 || row[3] != -1 || row[5] != -1) return thfhe_fail(THFHE_E_INVALID, "CB node: the operand fields and field 5 must be -1");
        if (row[4] < 0 || row[4] >= B.n_sets) return thfhe_fail(THFHE_E_INVALID, "CB node: cbset out of range (0 .. n_sets-1)");
        const thfhe_dag_cb_spec &cs = B.sets[row[4]];
        r.cls = kDagCb, r.list = B.cb_wires + cs.wire_off, r.list_count = cs.d, r.set_first = row[4], r.set_count = 1;
        for (int i = 0; i < cs.d; i++)
            if (r.list[i] < 0 || r.list[i] >= w) return thfhe_fail(THFHE_E_INVALID, "CB node: a pool wire is not an earlier wire");
        return THFHE_OK;
    }
    // (DENSE, wire_off, -1, -1, layer, -1); w: the row's own wire
    int dense(const int32_t *row, int32_t w, DagRow &r) {
        const thfhe_dag_dense_families &D = *F.dense;
        if (row[2] != -1 || row[3] != -1 || row[5] != -1) return thfhe_fail(THFHE_E_INVALID, "DENSE node: operand fields 2, 3 and field 5 must be -1");
        if (row[4] < 0 || row[4] >= D.n_layers) return thfhe_fail(THFHE_E_INVALID, "DENSE node: layer out of range (0 .. n_layers-1)");
        const thfhe_dag_dense_spec &l = D.layers[row[4]];
        if (!F.tv || F.n_luts < 1) return thfhe_fail(THFHE_E_INVALID, "DENSE node: no tables given (null table family)");
        if (first_use(kDagDense, row[4]) && l.lut_off >= 0)
            for (int m = 0; m < l.M; m++)
                if (D.words[l.lut_off + m] < 0 || D.words[l.lut_off + m] >= F.n_luts)
                    return thfhe_fail(THFHE_E_INVALID, "DENSE node: a lut_off entry is out of range (0 .. n_luts-1)");
        if (row[1] < 0 || (size_t)row[1] + (size_t)l.K > D.n_wires) return thfhe_fail(THFHE_E_INVALID, "DENSE node: wire_off + K runs past the wire pool");
        r.cls = kDagDense, r.entry = row[4], r.list = D.wires + row[1], r.list_count = l.K, r.outs = l.M * l.theta - 1;
        for (int i = 0; i < l.K; i++)
            if (r.list[i] < 0 || r.list[i] >= w) return thfhe_fail(THFHE_E_INVALID, "DENSE node: a pool wire is not an earlier wire");
        return THFHE_OK;
    }
    // a row other than LUT_OUT: the checker of its kind; an opcode of a generation the run does not admit goes to the engine's gates
    template <typename Classify>
    int node(const int32_t *row, int32_t w, Classify classify, DagRow &r) {
        const int32_t op = row[0];
        if ((F.gens & kDagGenLut) && op == THFHE_LUT) return lut(row, false, r);
        if ((F.gens & kDagGenTree) && op == THFHE_LUT_ENC) return lut(row, true, r);
        if ((F.gens & kDagGenTree) && (op == THFHE_SELECT || op == THFHE_TREE)) return tree(row, w, op == THFHE_TREE, r);
        if ((F.gens & kDagGenMv) && (op == THFHE_MV || (op == THFHE_TREE_MV && (F.gens & kDagGenTree)))) return mv(row, op == THFHE_TREE_MV, r);
        if ((F.gens & kDagGenLhe) && (op == THFHE_LHE_LOOKUP || op == THFHE_LHE_GATHER)) return lookup(row, w, op == THFHE_LHE_GATHER, r);
        if ((F.gens & kDagGenLhe) && op == THFHE_LHE_WFA) return wfa(row, r);
        if ((F.gens & kDagGenCb) && op == THFHE_CB) return cb(row, w, r);
        if ((F.gens & kDagGenDense) && op == THFHE_DENSE) return dense(row, w, r);
        return gate(row, classify, r);
    }
};

struct DagPlan {
    std::vector<DagBatch> batches;
    std::vector<int32_t> tab;
    size_t max_width = 0, max_rot = 0;
    int max_theta = 1;   // most records per node of any launch group (LUT groups: theta); sizes staging and workspace
    int64_t rotations = 0;
    int32_t max_depth = 0;
    size_t cb_pool = 0;          // plans with CB groups: the run's wire pool in tab, after the groups
    size_t cb_bits = 0;          // the d of every CB node of the run: its level-2 rotations per instance in one-rotation mode, 1 / l of them per level
    size_t cb_max_bits = 0;      // ... of the widest CB group
    void fill_stats(int64_t *stats) const {
        stats[0] = max_depth, stats[1] = 0, stats[2] = rotations, stats[3] = (int64_t)max_width;
        // a TREE / TREE_MV group: level-1 and selection launch
        for (const auto &b : batches) stats[1] += b.cls == kDagTree || b.cls == kDagTreeMv ? 2 : (b.cls != kDagLinear);
    }
    bool has_tree_groups() const {
        for (const auto &b : batches)
            if (b.cls == kDagSelect || b.cls == kDagTree || b.cls == kDagTreeMv || b.cls == kDagLheGather) return true;
        return false;
    }
    bool has_lhe_groups() const {
        for (const auto &b : batches)
            if (dag_class_leveled(b.cls)) return true;
        return false;
    }
    bool has_cb_groups() const { return cb_max_bits != 0; }
};

// the blind rotations of a launch group of `count` nodes: a MUX takes two, a TREE node its R level-1 rotations and the selection, a TREE_MV node one
// multi-value rotation and k selections; a linear gate and a leveled node none
inline size_t dag_group_rotations(const DagFamilies &F, int cls, int32_t entry, size_t count) {
    if (cls == kDagDense) return count * (size_t)F.dense->layers[entry].M;   // one rotation per output
    if (cls == kDagLinear || cls >= kDagLheLookup) return 0;   // a CB node: level-2 rotations only (DagPlan::cb_bits)
    if (cls == kDagMux) return 2 * count;
    if (cls == kDagTree) return count * (size_t)(F.trees[entry].p_hi / F.trees[entry].lo.theta + 1);
    if (cls == kDagTreeMv) return count * (size_t)(1 + F.mvs[entry].k);
    return count;
}

// ASAP schedule of A.nodes: int32[n_nodes][4] = (opcode, in0, in1, in2) in topological order, or, with any generation of F, rows of 6 words
// (opcode, in0, in1, in2, spec, lut); node g defines wire n_inputs + g.  F has passed dag_families_check.
// classify(op) -> kDagGate2, kDagMux, kDagLinear or kDagGate3, or -1.
// Every bootstrapped gate and every node adds one level above its operands (a SELECT's and a GATHER's candidates included; LHE_LOOKUP and LHE_WFA
// nodes have no wire operands and sit on the first); NOT / COPY ride on their operand's level as sub-levels (a NOT may read a NOT of the same
// depth).  The LUT_OUT rows a head is due -- theta - 1 (LUT, LUT_ENC, LHE_LOOKUP), q - 1 (MV), k - 1 (TREE_MV), n_out theta - 1 (LHE_WFA), M theta - 1 (DENSE) -- take
// its depth with sub-level 0 and launch nothing.
// Launch groups of a level, in this order: the gate classes kDagGate2, kDagGate3, kDagMux; the LUT classes by theta; the LUT_ENC classes by theta;
// the grouped kinds by ascending (class, entry), one group per entry; the linear sub-levels.
template <typename Classify>
int dag_plan(const DagCall &A, const DagFamilies &F, Classify classify, DagPlan &plan) {
    const size_t n_inputs = A.n_inputs, n_gates = A.n_nodes, n_wires = n_inputs + n_gates, stride = F.gens ? 6 : 4;
    const int32_t *const gates = A.nodes;
    if (n_wires > (size_t)INT32_MAX / 2) return thfhe_fail(THFHE_E_INVALID, "too many wires");
    std::vector<int32_t> depth(n_wires, 0), sub(n_wires, 0);
    std::vector<DagRow> rows(n_gates);
    DagRowChecks checks{F, {}};
    int32_t max_depth = 0;
    int32_t head = -1, pending = 0;   // the node whose LUT_OUT rows are still due, and how many
    const int n_client = F.n_client_sets();
    std::vector<int32_t> set_depth((size_t)F.n_computed_sets(), -1);   // the depth a computed set is defined at, -1 before its CB row
    for (size_t g = 0; g < n_gates; g++) {
        const int32_t *row = gates + stride * g;
        const int32_t w = (int32_t)(n_inputs + g);
        DagRow &r = rows[g];
        if (F.gens && row[0] == THFHE_LUT_OUT) {
            THFHE_TRY(DagRowChecks::lut_out(row, head, pending));
            pending--;
            depth[w] = depth[head], sub[w] = 0;
            continue;
        }
        if (pending) return thfhe_fail(THFHE_E_INVALID, "LUT node: missing LUT_OUT row (theta - 1 of them must follow it)");
        THFHE_TRY(checks.node(row, w, classify, r));
        head = w, pending = r.outs;
        int32_t d = 0, s = 0;
        auto above = [&](int32_t in) {
            if (depth[in] > d || (depth[in] == d && sub[in] > s)) d = depth[in], s = sub[in];
        };
        for (int q = 0; q < r.nin; q++) {
            const int32_t in = row[1 + q];
            if (in < 0 || in >= w) return thfhe_fail(THFHE_E_INVALID, "gate operand is not an earlier wire (gates must be in topological order)");
            above(in);
        }
        for (int32_t in = r.cand_first; in < r.cand_first + r.cand_count; in++) above(in);
        for (int32_t i = 0; i < r.list_count; i++) above(r.list[i]);
        if (r.cls != kDagCb)   // a leveled row inherits the depth of the computed sets it reads
            for (int32_t t = std::max(r.set_first, n_client); t < r.set_first + r.set_count; t++) {
                if (set_depth[t - n_client] < 0) return thfhe_fail(THFHE_E_INVALID, "leveled node: it reads a computed set before the set's CB row");
                if (set_depth[t - n_client] >= d) d = set_depth[t - n_client], s = 0;
            }
        if (r.cls == kDagLinear) s += 1; else d += 1, s = 0;
        if (r.cls == kDagCb) {
            if (set_depth[r.set_first] >= 0) return thfhe_fail(THFHE_E_INVALID, "CB node: the set has a CB row already (exactly one per computed set)");
            set_depth[r.set_first] = d;
        }
        depth[w] = d, sub[w] = s;
        if (d > max_depth) max_depth = d;
    }
    if (pending) return thfhe_fail(THFHE_E_INVALID, "LUT node: missing LUT_OUT row (theta - 1 of them must follow it)");
    for (int32_t sd : set_depth)
        if (sd < 0) return thfhe_fail(THFHE_E_INVALID, "cb: a computed set has no CB row (exactly one per computed set)");
    plan.max_depth = max_depth;
    // per level: the bootstrapped groups by (class, entry) -- entry -1 for the classes that are one group --, and the linear sub-levels in order
    struct Level {
        std::map<std::pair<int, int32_t>, std::vector<int32_t>> boot;
        std::vector<std::vector<int32_t>> lin;
    };
    std::vector<Level> levels(max_depth + 1);
    for (size_t g = 0; g < n_gates; g++) {
        const int32_t w = (int32_t)(n_inputs + g);
        if (rows[g].cls == kDagLutOut) continue;
        if (rows[g].cls == kDagLinear) {
            auto &L = levels[depth[w]].lin;
            if ((int)L.size() < sub[w]) L.resize(sub[w]);
            L[sub[w] - 1].push_back((int32_t)g);
        } else {
            levels[depth[w]].boot[{rows[g].cls, rows[g].entry}].push_back((int32_t)g);
        }
    }
    plan.tab.reserve(5 * n_gates);
    auto emit = [&](int32_t d, int32_t s, int32_t k, const std::vector<int32_t> &G, int32_t entry) {
        static constexpr int kField[7] = {0, 1, 2, 3, -1, 4, 5};   // [ops | in0 | in1 | in2 | out | spec | lut] from the row's fields; out: the node's wire
        plan.batches.push_back(DagBatch{d, s, k, plan.tab.size(), G.size(), entry});
        for (int col = 0; col < (k >= kDagLut1 ? 7 : 5); col++)   // an unused field (-1) reads as 0
            for (int32_t g : G) plan.tab.push_back(kField[col] < 0 ? (int32_t)(n_inputs + g) : std::max(gates[stride * g + kField[col]], 0));
        const size_t rot = dag_group_rotations(F, k, entry, G.size());
        plan.max_width = std::max(plan.max_width, G.size()), plan.max_rot = std::max(plan.max_rot, rot), plan.max_theta = std::max(plan.max_theta, dag_class_theta(k));
        plan.rotations += (int64_t)rot;
    };
    for (int32_t d = 0; d <= max_depth; d++) {
        const auto &boot = levels[d].boot;
        for (int32_t k : {kDagGate2, kDagGate3, kDagMux, kDagLut1, kDagLut2, kDagLut4, kDagEnc1, kDagEnc2, kDagEnc4})
            if (const auto it = boot.find({k, -1}); it != boot.end()) emit(d, 0, k, it->second, -1);
        // the level's CB nodes: one group, its node table after its columns
        auto emit_cb = [&]() {
            const auto it = boot.find({kDagCb, -1});
            if (it == boot.end()) return;
            emit(d, 0, kDagCb, it->second, -1);
            plan.batches.back().ext = plan.tab.size();
            int32_t base = 0;
            for (int32_t g : it->second) {
                const thfhe_dag_cb_spec &cs = F.cb->sets[gates[stride * g + 4]];
                for (int32_t v : {base, cs.wire_off, cs.d, (int32_t)(n_inputs + g)}) plan.tab.push_back(v);
                base += cs.d;
            }
            plan.batches.back().bits = (size_t)base;
            plan.cb_bits += (size_t)base, plan.cb_max_bits = std::max(plan.cb_max_bits, (size_t)base);
        };
        bool cb_done = false;
        for (auto it = boot.lower_bound({kDagSelect, INT32_MIN}); it != boot.end(); ++it) {
            if (it->first.first == kDagCb) continue;
            if (it->first.first >= kDagLheLookup && !cb_done) emit_cb(), cb_done = true;
            emit(d, 0, it->first.first, it->second, it->first.second);
        }
        if (!cb_done) emit_cb();
        for (size_t q = 0; q < levels[d].lin.size(); q++) emit(d, (int32_t)q + 1, kDagLinear, levels[d].lin[q], -1);
    }
    if (plan.cb_max_bits) {
        plan.cb_pool = plan.tab.size();
        plan.tab.insert(plan.tab.end(), F.cb->cb_wires, F.cb->cb_wires + F.cb->n_cb_wires);
    }
    return THFHE_OK;
}

// The host side of a six-column entry, before any device work and before a context is looked at: the family checks, then the row checks and the plan.
template <typename Classify>
int dag_checked_plan(const DagCall &A, const DagFamilies &F, Classify classify, DagPlan &plan) {
    THFHE_TRY(dag_families_check(A, F));
    return dag_plan(A, F, classify, plan);
}

// Device buffers of the executor (grow-only, owned by the engine's context and reused by every run on it).
struct DagBuffers {
    DevBuf wires, tab, ops, pack;
    DevBuf specs;   // thfhe_lut_spec[n_specs] of a LUT run
    // stage events of a run (thfhe_dag_last_stage_ms): the engine sets `timed` from its profiling switch before dag_execute, which then records
    // before the input upload | after the uploads (inputs, index table, output wire list) | after the last level | after the output gather and
    // the download are enqueued
    bool timed = false, st_valid = false;
    hipEvent_t st_ev[4] = {nullptr, nullptr, nullptr, nullptr};
    DagBuffers() = default;
    DagBuffers(const DagBuffers &) = delete;
    DagBuffers &operator=(const DagBuffers &) = delete;
    ~DagBuffers() {
        for (hipEvent_t e : st_ev)
            if (e) (void)hipEventDestroy(e);
    }
    // event k of a timed run on `stream`; an untimed run records nothing
    hipError_t stamp(int k, hipStream_t stream) {
        if (!timed) return hipSuccess;
        if (!st_ev[k]) {
            const hipError_t e = hipEventCreate(&st_ev[k]);
            if (e != hipSuccess) return e;
        }
        return hipEventRecord(st_ev[k], stream);
    }
};

// The slice of a LUT or LUT_ENC launch group that DagExecute hands to the engine: wire table, the group's index columns, jobs
// [first, first + total) of cnt nodes per instance; enc: t_lut names the run's encrypted tables.  The engine runs the prologue on src(), its LUT
// rotation and the key switch of total x theta records into its staging output.
struct DagLutSlice {
    const int32_t *wires, *t0, *t1, *t2, *t_spec, *t_lut;
    long first, total, cnt;
    size_t n_wires;
    bool enc;
    LutWireSrc<LutSpecPerNode, LutIdx::table> src(const thfhe_lut_spec *d_specs) const {
        return {wires, t0, t1, t2, {d_specs, t_spec}, t_lut, first, cnt, n_wires, 1};
    }
};

// A SELECT or TREE launch group as DagExecute hands it to the engine (thfhe_dag_run_tree_batch): the wire table, the group's index columns
// (t_y = a SELECT's first candidate wire, a TREE's row0), `all` = cnt nodes x instances jobs.  MV and TREE_MV groups (thfhe_dag_run_mv_batch): tree =
// the group's mvs[] entry, t_y = each node's table t.  The engine cuts it into slices, runs the chain of
// each and scatters the results into the wires t_out.
struct DagExtGroup {
    int cls, tree;
    int32_t *wires;
    const int32_t *t0, *t1, *t2, *t_out, *t_y;
    long all, cnt;
    size_t n_wires;
    size_t off = 0;   // the group's index columns in plan.tab, for an engine that walks the nodes on the host (the leveled groups)
    const int32_t *tab = nullptr;   // the device's copy of plan.tab
    size_t ext = 0;                 // a CB group: its node table at tab[ext] (DagBatch::ext)
};

// Device-resident executor.  Level by level, each class of a level as slices of at most `slice_cap` gates over ALL instances: gather ->
// run(cls, d_ops, n) (the engine's prologue + blind rotations + key switch from its staging arrays stage_in[0..2] into stage_out) ->
// scatter.  Nothing synchronises with the host between levels.
//   A.inputs     int32[instances][n_inputs][words]
//   A.out_wires  wire ids to return (n_out of them) or null = every gate wire [n_inputs, n_wires)
//   A.outputs    int32[instances][n_out or n_nodes][words]
// ensure(max_gates_per_slice) sizes the engine's workspace and staging and returns its staging pointers through the out-parameters.
// LUT and LUT_ENC launch groups: run_lut(theta, DagLutSlice) -> prologue + LUT rotation + key switch of the slice's nodes x theta records into
// the staging output, then the theta-record scatter into wires out[g] + j.  ensure sizes for plan.max_theta records per node.  SELECT / TREE
// groups (plans of thfhe_dag_run_tree_batch): run_ext(DagExtGroup) slices, runs and scatters the whole group.  An engine without run_ext
// rejects all three kinds.
template <typename Ensure, typename Run, typename RunLut = std::nullptr_t, typename RunExt = std::nullptr_t>
int dag_execute(const DagPlan &plan, DagBuffers &B, hipStream_t stream, int words, const DagCall &A, size_t instances, size_t slice_cap, Ensure ensure, Run run,
                RunLut run_lut = nullptr, RunExt run_ext = nullptr) {
    const size_t n_inputs = A.n_inputs, n_gates = A.n_nodes, n_sel = A.n_out, n_wires = n_inputs + n_gates;
    const int32_t *const h_inputs = A.inputs, *const h_sel = A.out_wires;
    int32_t *const h_out = A.outputs;
    if (instances == 0 || n_gates == 0) return THFHE_OK;
    if (n_wires * instances > ((size_t)1 << 40) / (size_t)words) return thfhe_fail(THFHE_E_INVALID, "wire table too large");
    for (size_t s = 0; s < n_sel; s++)
        if (h_sel[s] < 0 || (size_t)h_sel[s] >= n_wires) return thfhe_fail(THFHE_E_INVALID, "output wire id out of range");
    const size_t widest = plan.max_width * instances, slice = widest < slice_cap ? widest : slice_cap;
    int32_t *stage_in[3] = {nullptr, nullptr, nullptr}, *stage_out = nullptr;
    int rc = ensure(slice ? slice : 1, stage_in, &stage_out);
    if (rc) return rc;
    const size_t rec = (size_t)words * sizeof(int32_t);
    rc = B.wires.grow(instances * n_wires * rec);
    if (!rc) rc = B.tab.grow((plan.tab.size() + n_sel) * sizeof(int32_t));
    if (!rc) rc = B.ops.grow((slice ? slice : 1) * sizeof(int32_t));
    if (!rc && h_sel) rc = B.pack.grow(instances * n_sel * rec);
    if (rc) return rc;
    int32_t *const d_wires = B.wires.as<int32_t>(), *const d_tab = B.tab.as<int32_t>(), *const d_sel = d_tab + plan.tab.size();
    int32_t *const d_ops = B.ops.as<int32_t>(), *const d_pack = B.pack.as<int32_t>();
    B.st_valid = false;
    hipError_t e = B.stamp(0, stream);
    if (e == hipSuccess && n_inputs) e = hipMemcpy2DAsync(d_wires, n_wires * rec, h_inputs, n_inputs * rec, n_inputs * rec, instances, hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_tab, plan.tab.data(), plan.tab.size() * sizeof(int32_t), hipMemcpyHostToDevice, stream);
    if (e == hipSuccess && n_sel) e = hipMemcpyAsync(d_sel, h_sel, n_sel * sizeof(int32_t), hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) e = B.stamp(1, stream);
    rc = e == hipSuccess ? THFHE_OK : thfhe_fail_hip(e, "gate-DAG executor: upload");
    const unsigned wb = (unsigned)((words + 255) / 256);
    const dim3 block(256);
    for (size_t b = 0; b < plan.batches.size() && rc == THFHE_OK; b++) {
        const long cnt = (long)plan.batches[b].count, all = cnt * (long)instances;
        const int cls = plan.batches[b].cls;
        const int32_t *t_ops = d_tab + plan.batches[b].off, *t0 = t_ops + cnt, *t1 = t0 + cnt, *t2 = t1 + cnt, *t_out = t2 + cnt;
        if (cls == kDagLinear) {
            hipLaunchKernelGGL(dag_wire_linear_kernel, dim3((unsigned)all, wb), block, 0, stream, d_wires, t0, t_out, t_ops, all, cnt, n_wires, words);
            continue;
        }
        if (cls >= kDagEnc1 && std::is_same_v<RunExt, std::nullptr_t>) {
            rc = thfhe_fail(THFHE_E_INVALID, "encrypted-table, select or tree node in a run without them");
            continue;
        }
        if (cls >= kDagSelect) {
            if constexpr (!std::is_same_v<RunExt, std::nullptr_t>)
                rc = run_ext(DagExtGroup{cls, plan.batches[b].tree, d_wires, t0, t1, t2, t_out, t_out + 2 * cnt, all, cnt, n_wires, plan.batches[b].off, d_tab,
                                             plan.batches[b].ext});
            continue;
        }
        if (cls >= kDagLut1) {   // LUT groups, and LUT_ENC groups over the run's encrypted tables
            if constexpr (std::is_same_v<RunLut, std::nullptr_t>) {
                rc = thfhe_fail(THFHE_E_INVALID, "LUT node in a gate-only run");
            } else {
                const bool enc = cls >= kDagEnc1;
                const int theta = dag_class_theta(cls);
                const int32_t *t_spec = t_out + cnt, *t_lut = t_spec + cnt;
                for (long first = 0; first < all && rc == THFHE_OK; first += (long)slice) {
                    const long n = all - first < (long)slice ? all - first : (long)slice;
                    rc = run_lut(theta, DagLutSlice{d_wires, t0, t1, t2, t_spec, t_lut, first, n, cnt, n_wires, enc});
                    if (!rc)
                        hipLaunchKernelGGL(dag_scatter_theta_kernel, dim3((unsigned)(n * theta), wb), block, 0, stream, stage_out, t_out, d_wires, first, n, cnt,
                                           n_wires, words, theta);
                }
            }
            continue;
        }
        for (long first = 0; first < all && rc == THFHE_OK; first += (long)slice) {
            const long n = all - first < (long)slice ? all - first : (long)slice;
            const dim3 grid((unsigned)n, wb);
            hipLaunchKernelGGL(dag_gather_kernel, grid, block, 0, stream, d_wires, t0, stage_in[0], first, n, cnt, n_wires, words, t_ops, d_ops);
            hipLaunchKernelGGL(dag_gather_kernel, grid, block, 0, stream, d_wires, t1, stage_in[1], first, n, cnt, n_wires, words, nullptr, nullptr);
            if (cls != kDagGate2) hipLaunchKernelGGL(dag_gather_kernel, grid, block, 0, stream, d_wires, t2, stage_in[2], first, n, cnt, n_wires, words, nullptr, nullptr);
            rc = run(cls, d_ops, (size_t)n);
            if (!rc) hipLaunchKernelGGL(dag_scatter_kernel, grid, block, 0, stream, stage_out, t_out, d_wires, first, n, cnt, n_wires, words);
        }
    }
    if (rc == THFHE_OK) {
        e = hipGetLastError();
        if (e == hipSuccess) e = B.stamp(2, stream);
        if (e == hipSuccess && h_sel && n_sel) {
            const long all = (long)(n_sel * instances);
            hipLaunchKernelGGL(dag_gather_kernel, dim3((unsigned)all, wb), block, 0, stream, d_wires, d_sel, d_pack, 0L, all, (long)n_sel, n_wires, words, nullptr, nullptr);
            e = hipGetLastError();
            if (e == hipSuccess) e = hipMemcpyAsync(h_out, d_pack, instances * n_sel * rec, hipMemcpyDeviceToHost, stream);
        } else if (e == hipSuccess && !h_sel) {
            e = hipMemcpy2DAsync(h_out, n_gates * rec, d_wires + n_inputs * (size_t)words, n_wires * rec, n_gates * rec, instances, hipMemcpyDeviceToHost, stream);
        }
        if (e == hipSuccess) e = B.stamp(3, stream);
        if (e != hipSuccess) rc = thfhe_fail_hip(e, "gate-DAG executor");
    }
    e = hipStreamSynchronize(stream);
    if (rc == THFHE_OK && e != hipSuccess) rc = thfhe_fail_hip(e, "gate-DAG executor: sync");
    B.st_valid = B.timed && rc == THFHE_OK;
    return rc;
}

// One table family or spec array of a run into its grow-only device buffer, once per call; an absent family (bytes = 0) uploads nothing.
inline int dag_upload(DevBuf &d, hipStream_t stream, const void *h, size_t bytes) {
    if (!bytes) return THFHE_OK;
    THFHE_TRY(d.grow(bytes));
    THFHE_HIP(hipMemcpyAsync(d.as<void>(), h, bytes, hipMemcpyHostToDevice, stream));
    return THFHE_OK;
}

// A grouped launch group in slices of at most `slice` nodes over all instances: body(first, S) enqueues the chain of nodes [first, first + S) of
// g.all, `outs` records of `words` words per node into stage_out; then record j outs + t of the slice goes to wire t_out[g] + t of its instance.
template <typename Body>
int dag_group_slices(const DagExtGroup &g, size_t slice, int outs, const int32_t *stage_out, int words, hipStream_t stream, Body body) {
    const unsigned wb = (unsigned)((words + 255) / 256);
    for (long first = 0; first < g.all; first += (long)slice) {
        const long S = std::min((long)slice, g.all - first);
        THFHE_TRY(body(first, S));
        if (outs == 1)
            hipLaunchKernelGGL(dag_scatter_kernel, dim3((unsigned)S, wb), dim3(256), 0, stream, stage_out, g.t_out, g.wires, first, S, g.cnt, g.n_wires, words);
        else
            hipLaunchKernelGGL(dag_scatter_theta_kernel, dim3((unsigned)(S * outs), wb), dim3(256), 0, stream, stage_out, g.t_out, g.wires, first, S, g.cnt,
                               g.n_wires, words, outs);
        THFHE_HIP(hipGetLastError());
    }
    return THFHE_OK;
}

// thfhe_dag_run_batch / thfhe_mk_dag_run_batch: four-column gate rows only.  classify, ensure and run are dag_plan's and dag_execute's.
template <typename Ctx, typename Classify, typename Ensure, typename Run>
int dag_gates_run_batch(Ctx *c, const DagCall &A, size_t instances, int64_t *stats, Classify classify, Ensure ensure, Run run) {
    if (!c || (!A.inputs && A.n_inputs) || (!A.nodes && A.n_nodes) || (!A.outputs && A.n_nodes) || (!A.out_wires && A.n_out))
        return thfhe_fail(THFHE_E_INVALID, "null argument");
    DagPlan plan;
    THFHE_TRY(dag_plan(A, DagFamilies{}, classify, plan));
    if (stats) plan.fill_stats(stats);
    DevLock lk(*c);
    if (lk.rc) return lk.rc;
    return dag_execute(plan, c->dag, c->stream, c->rec_words(), A, instances, c->dag_slice, ensure, run);
}
// thfhe_dag_run / thfhe_mk_dag_run: one instance in place, every gate's wire written after the inputs; run_batch is the engine's entry above
template <typename Ctx, typename RunBatch>
int dag_gates_run(Ctx *c, int32_t *wires, size_t n_inputs, const int32_t *gates, size_t n_gates, int64_t *stats, RunBatch run_batch) {
    if (!wires) return thfhe_fail(THFHE_E_INVALID, "null argument");
    return run_batch(c, wires, n_inputs, gates, n_gates, 1, nullptr, 0, wires + n_inputs * (size_t)(c ? c->rec_words() : 0), stats);
}

}  // namespace

#endif  // THFHE_DAG_H
