// thfhe_dag.h -- the gate-DAG front end shared by the single-key and the 3-gen multi-key engines:
// an ASAP levelising scheduler for the reference's circuits (src/KNN_medical_data.cpp:127-489, J/3gen_mk_gates.jl:183-362), and the
// gather / scatter kernels of the device-resident executor.  LUT nodes (thfhe_dag_run_lut_batch): programmable bootstraps among the
// gates, fed by the shared prologue reading their operands from the wire table (LutWireSrc, thfhe_lut_prologue.h), their theta outputs scattered
// into consecutive wires.
// Encrypted-table, select and tree nodes (thfhe_dag_run_tree_batch, DESIGN 4.12, single key): three more node kinds, planned here, run by the engine.
// Multi-value nodes (thfhe_dag_run_mv_batch, DESIGN 4.14, single key): MV and TREE_MV rows, planned here next to them.
// Leveled nodes (thfhe_dag_run_lhe_batch, DESIGN 4.18, single key): LHE_LOOKUP, LHE_GATHER and LHE_WFA rows on the client's TGSW sets, planned here;
// dag_lhe_gather_kernel stages a GATHER node's candidates for the box packing.
#ifndef THFHE_DAG_H
#define THFHE_DAG_H

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <map>
#include <type_traits>
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

// One launch group of the schedule: `count` gates of one class whose operands are all available.
struct DagBatch {
    int32_t depth, sub, cls;  // cls: engine-defined gate class; 2 = NOT / COPY (no bootstrap); 4 / 5 / 6 = LUT nodes of theta 1 / 2 / 4
    size_t off, count;        // index table slice: [ops | in0 | in1 | in2 | out], LUT classes + [spec | lut], `count` entries each, at tab[off]
    int32_t tree = -1;        // SELECT / TREE groups: the trees[] entry the whole group shares; MV / TREE_MV groups: the mvs[] entry; leveled groups: lks[] / wfas[]
};
constexpr int kDagLutOut = 7;                // LUT_OUT row: no launch, its wire is written by its head's scatter
inline int dag_lut_class(int theta) { return theta == 1 ? 4 : (theta == 2 ? 5 : 6); }
inline int dag_lut_theta(int cls) { return cls == 4 ? 1 : (cls == 5 ? 2 : 4); }
// thfhe_dag_run_tree_batch: LUT_ENC nodes of theta 1 / 2 / 4 = 8 / 9 / 10 (index columns as the LUT classes: [spec | etab]); SELECT groups = 11
// ([tree | first]), TREE groups = 12 ([tree | row0]), one group per trees[] entry
constexpr int kDagEnc = 8, kDagSelect = 11, kDagTree = 12;
inline int dag_enc_theta(int cls) { return cls == 8 ? 1 : (cls == 9 ? 2 : 4); }
// thfhe_dag_run_mv_batch: MV groups = 13, TREE_MV groups = 14 ([mv | t]), one group per mvs[] entry
constexpr int kDagMv = 13, kDagTreeMv = 14;
// thfhe_dag_run_lhe_batch: LHE_LOOKUP groups = 15 ([lk | row0]), LHE_GATHER groups = 16 ([lk | first]), one group per lks[] entry; LHE_WFA groups = 17
// ([wfa | fin_row0]), one group per wfas[] entry
constexpr int kDagLheLookup = 15, kDagLheGather = 16, kDagLheWfa = 17;

// The LUT side of a run (thfhe_dag_run_lut_batch): node rows of 6 words, the run's specs and its table count.
struct DagLuts {
    const thfhe_lut_spec *specs;
    int n_specs, n_luts;
    // thfhe_dag_run_tree_batch only (ext): the encrypted-table count, the tree specs and the level-1 row count
    bool ext = false;
    int n_enc = 0;
    const thfhe_tree_spec *trees = nullptr;
    int n_trees = 0, n_tv1_rows = 0;
    // thfhe_dag_run_mv_batch only (mv): the multi-value specs, the base-vector count and the words of the factor array
    bool mv = false;
    const thfhe_mv_spec *mvs = nullptr;
    int n_mvs = 0, n_bases = 0;
    size_t n_factor_words = 0;
    // thfhe_dag_run_lhe_batch only: the leveled families (host pointers; a family the run does not have is null / 0)
    const thfhe_dag_lhe_families *lhe = nullptr;
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
inline int dag_mv_spec_check(const DagLuts &L, const thfhe_mv_spec &m, bool tree) {
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
    if (L.n_bases < 1) return thfhe_fail(THFHE_E_INVALID, "MV / TREE_MV node: no base vectors given (null table family)");
    if (m.base < 0 || m.base >= L.n_bases) return thfhe_fail(THFHE_E_INVALID, "MV / TREE_MV node: base out of range (0 .. n_bases-1)");
    if (L.n_factor_words < 1) return thfhe_fail(THFHE_E_INVALID, "MV / TREE_MV node: no factors given (null table family)");
    if (m.factors_off < 0 || (size_t)m.factors_off + (size_t)m.n_tables * m.k * m.q * m.p > L.n_factor_words)
        return thfhe_fail(THFHE_E_INVALID, "MV / TREE_MV node: factors_off + n_tables k q p out of range (0 .. n_factor_words)");
    return THFHE_OK;
}

// One lks[] entry as a LOOKUP row (gather = false) or a GATHER row uses it: the rules of thfhe_lhe_lookup that need no set, then the node kind's own.
inline int dag_lhe_spec_check(const thfhe_dag_lhe_families &F, const thfhe_dag_lhe_spec &k, bool gather) {
    if (k.d_tree < 0 || k.d_tree > 6) return thfhe_fail(THFHE_E_INVALID, "leveled node: d_tree must be 0 .. 6");
    if (k.d_rot < 0 || k.d_rot > 10) return thfhe_fail(THFHE_E_INVALID, "leveled node: d_rot must be 0 .. 10");
    if (k.theta != 1 && k.theta != 2 && k.theta != 4) return thfhe_fail(THFHE_E_INVALID, "leveled node: theta must be 1, 2 or 4");
    if (k.theta > (1024 >> k.d_rot)) return thfhe_fail(THFHE_E_INVALID, "leveled node: theta must not exceed box = N >> d_rot");
    if (gather && k.theta != 1) return thfhe_fail(THFHE_E_INVALID, "LHE_GATHER node: the spec's theta must be 1 (a packed box holds one value)");
    if (gather && (k.d_rot < 1 || k.d_rot > 9)) return thfhe_fail(THFHE_E_INVALID, "LHE_GATHER node: d_rot must be 1 .. 9 (the box packing's p = 2^d_rot)");
    if (!F.sets || F.n_sets < 1) return thfhe_fail(THFHE_E_INVALID, "leveled node: no tgsw sets given (null family)");
    if (k.set < 0 || k.set >= F.n_sets) return thfhe_fail(THFHE_E_INVALID, "leveled node: the spec's set is out of range (0 .. n_sets-1)");
    return THFHE_OK;
}
// One wfas[] entry: the rules of thfhe_lhe_wfa that need no set, its sets within sets[], its three slices of the word pool and their entries.
inline int dag_wfa_spec_check(const thfhe_dag_lhe_families &F, const thfhe_dag_wfa_spec &a) {
    if (a.n_sets < 1 || a.n_sets > 64) return thfhe_fail(THFHE_E_INVALID, "LHE_WFA node: the spec's n_sets must be 1 .. 64");
    if (a.n_steps < 1 || a.n_steps > 4096) return thfhe_fail(THFHE_E_INVALID, "LHE_WFA node: n_steps must be 1 .. 4096");
    if (a.n_states < 1 || a.n_states > 64) return thfhe_fail(THFHE_E_INVALID, "LHE_WFA node: n_states must be 1 .. 64");
    if (a.n_out < 1 || a.n_out > 64) return thfhe_fail(THFHE_E_INVALID, "LHE_WFA node: n_out must be 1 .. 64");
    if (a.theta != 1 && a.theta != 2 && a.theta != 4) return thfhe_fail(THFHE_E_INVALID, "LHE_WFA node: theta must be 1, 2 or 4");
    if (!F.sets || F.n_sets < 1) return thfhe_fail(THFHE_E_INVALID, "leveled node: no tgsw sets given (null family)");
    if (a.set0 < 0 || (long)a.set0 + a.n_sets > F.n_sets) return thfhe_fail(THFHE_E_INVALID, "LHE_WFA node: set0 + n_sets out of range (0 .. n_sets)");
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

struct DagPlan {
    std::vector<DagBatch> batches;
    std::vector<int32_t> tab;
    size_t max_width = 0, max_rot = 0;
    int max_theta = 1;   // most records per node of any launch group (LUT groups: theta); sizes staging and workspace
    int64_t rotations = 0;
    int32_t max_depth = 0;
    void fill_stats(int64_t *stats) const {
        stats[0] = max_depth, stats[1] = 0, stats[2] = rotations, stats[3] = (int64_t)max_width;
        for (const auto &b : batches) stats[1] += b.cls == kDagTree || b.cls == kDagTreeMv ? 2 : (b.cls != 2);   // a TREE / TREE_MV group: level-1 and selection launch
    }
    bool has_tree_groups() const {
        for (const auto &b : batches)
            if (b.cls == kDagSelect || b.cls == kDagTree || b.cls == kDagTreeMv || b.cls == kDagLheGather) return true;
        return false;
    }
    bool has_lhe_groups() const {
        for (const auto &b : batches)
            if (b.cls >= kDagLheLookup) return true;
        return false;
    }
};

// ASAP schedule.  gates: int32[n_gates][4] = (opcode, in0, in1, in2) in topological order; gate g defines wire n_inputs + g.
// classify(op) -> class id (0 = two-input bootstrapped gate, 1 = MUX, 2 = NOT / COPY, 3 = three-input bootstrapped gate) or -1.
// Bootstrapped gates add one level; NOT / COPY ride on their operand's level as sub-levels (a NOT may read a NOT of the same depth).
// luts (thfhe_dag_run_lut_batch): rows of 6 words (opcode, in0, in1, in2, spec, lut); a THFHE_LUT node adds one level like a bootstrapped
// gate and joins the launch group of its theta; its theta - 1 THFHE_LUT_OUT rows take its depth with sub-level 0 and launch nothing.
// luts->ext (thfhe_dag_run_tree_batch): THFHE_LUT_ENC rows are LUT rows over the encrypted tables (classes 8 / 9 / 10); THFHE_SELECT and THFHE_TREE
// rows add one level above their operands (a SELECT's candidates included) and form one group per trees[] entry, emitted after the other classes.
// luts->mv (thfhe_dag_run_mv_batch): THFHE_MV and THFHE_TREE_MV rows (mv, t) add one level and form one group per mvs[] entry, emitted after those;
// q - 1 (MV) or k - 1 (TREE_MV) LUT_OUT rows follow the head.
// luts->lhe (thfhe_dag_run_lhe_batch): LHE_LOOKUP, LHE_GATHER and LHE_WFA rows (no wire operands; lk / wfa, row0 / first / fin_row0) add one level --
// a GATHER above its candidates, the two others on the first -- and form one group per lks[] / wfas[] entry, emitted after those; theta - 1 (LOOKUP) or
// n_out theta - 1 (WFA) LUT_OUT rows follow the head.
template <typename Classify>
int dag_plan(const int32_t *gates, size_t n_inputs, size_t n_gates, Classify classify, DagPlan &plan, const DagLuts *luts = nullptr) {
    const size_t n_wires = n_inputs + n_gates, stride = luts ? 6 : 4;
    if (n_wires > (size_t)INT32_MAX / 2) return thfhe_fail(THFHE_E_INVALID, "too many wires");
    std::vector<int32_t> depth(n_wires, 0), sub(n_wires, 0), cls(n_gates, 0);
    const bool ext = luts && luts->ext;
    std::vector<char> tree_lo_ok(ext ? (size_t)luts->n_trees : 0, 0);   // trees[] entries whose `lo` half a TREE row has had checked
    const bool mvx = ext && luts->mv;
    std::vector<char> mv_ok(mvx ? (size_t)luts->n_mvs : 0, 0);          // mvs[] entries checked as an MV (bit 0) / a TREE_MV (bit 1) row uses them
    const thfhe_dag_lhe_families *const lhe = mvx ? luts->lhe : nullptr;
    std::vector<char> lk_ok(lhe && lhe->lks ? (size_t)lhe->n_lks : 0, 0), wfa_ok(lhe && lhe->wfas ? (size_t)lhe->n_wfas : 0, 0);   // as mv_ok: LOOKUP bit 0, GATHER bit 1
    int32_t max_depth = 0;
    int32_t head = -1, pending = 0;   // the LUT node whose LUT_OUT rows are still due, and how many
    for (size_t g = 0; g < n_gates; g++) {
        const int32_t *row = gates + stride * g;
        const int32_t op = row[0], w = (int32_t)(n_inputs + g);
        if (luts && op == THFHE_LUT_OUT) {
            if (pending == 0) return thfhe_fail(THFHE_E_INVALID, "LUT_OUT row without a LUT node before it (extra or misplaced LUT_OUT row)");
            if (row[1] != head) return thfhe_fail(THFHE_E_INVALID, "LUT_OUT row names the wrong head (it must name its LUT node's wire)");
            if (row[2] != -1 || row[3] != -1 || row[4] != -1 || row[5] != -1) return thfhe_fail(THFHE_E_INVALID, "LUT_OUT row: fields after the head must be -1");
            pending--;
            cls[g] = kDagLutOut;
            depth[w] = depth[head], sub[w] = 0;
            continue;
        }
        if (pending) return thfhe_fail(THFHE_E_INVALID, "LUT node: missing LUT_OUT row (theta - 1 of them must follow it)");
        int k, nin;
        int32_t cand_first = 0, cand_count = 0;   // SELECT: its candidate wires
        if (luts && (op == THFHE_LUT || (ext && op == THFHE_LUT_ENC))) {
            const bool enc = op == THFHE_LUT_ENC;
            if (ext && (!luts->specs || (!enc && luts->n_luts == 0)))
                return thfhe_fail(THFHE_E_INVALID, enc ? "LUT_ENC node: no specs given (null table family)" : "LUT node: no specs or no tables given (null table family)");
            if (enc && luts->n_enc < 1) return thfhe_fail(THFHE_E_INVALID, "LUT_ENC node: n_enc must be 1 .. 262144 (null table family)");
            if (row[4] < 0 || row[4] >= luts->n_specs) return thfhe_fail(THFHE_E_INVALID, "LUT node: spec index out of range (0 .. n_specs-1)");
            if (!enc && (row[5] < 0 || row[5] >= luts->n_luts)) return thfhe_fail(THFHE_E_INVALID, "LUT node: table index out of range (0 .. n_luts-1)");
            if (enc && (row[5] < 0 || row[5] >= luts->n_enc)) return thfhe_fail(THFHE_E_INVALID, "LUT_ENC node: etab out of range (0 .. n_enc-1)");
            const thfhe_lut_spec &sp = luts->specs[row[4]];
            nin = sp.n_inputs;
            for (int q = 0; q < 3; q++)
                if ((q < nin) != (row[1 + q] != -1)) return thfhe_fail(THFHE_E_INVALID, "LUT node: operands do not match the spec's n_inputs (unused ones are -1)");
            k = enc ? kDagEnc + (dag_lut_class(sp.theta) - 4) : dag_lut_class(sp.theta);
            head = w, pending = sp.theta - 1;
        } else if (ext && (op == THFHE_SELECT || op == THFHE_TREE)) {
            const bool is_tree = op == THFHE_TREE;
            if (!luts->trees) return thfhe_fail(THFHE_E_INVALID, "SELECT / TREE node: no tree specs given (null table family)");
            if (row[4] < 0 || row[4] >= luts->n_trees) return thfhe_fail(THFHE_E_INVALID, "SELECT / TREE node: tree index out of range (0 .. n_trees-1)");
            const thfhe_tree_spec &ts = luts->trees[row[4]];
            nin = ts.hi.n_inputs;
            if (is_tree) {
                if (!tree_lo_ok[row[4]]) {
                    THFHE_TRY(lut_spec_check(ts.lo));
                    if (ts.p_hi % ts.lo.theta) return thfhe_fail(THFHE_E_INVALID, "tree: spec_lo theta must divide p_hi");
                    tree_lo_ok[row[4]] = 1;
                }
                nin += ts.lo.n_inputs;
                if (nin > 3) return thfhe_fail(THFHE_E_INVALID, "TREE node: lo and hi operands exceed three");
                if (luts->n_tv1_rows < 1) return thfhe_fail(THFHE_E_INVALID, "TREE node: no level-1 rows given (null table family)");
                if (row[5] < 0 || (long)row[5] + ts.p_hi / ts.lo.theta > luts->n_tv1_rows)
                    return thfhe_fail(THFHE_E_INVALID, "TREE node: row0 + R out of range (0 .. n_tv1_rows)");
            } else {
                cand_first = row[5], cand_count = ts.p_hi;
                if (cand_first < 0 || (long)cand_first + cand_count > (long)w)
                    return thfhe_fail(THFHE_E_INVALID, "SELECT node: candidate is not an earlier wire (first .. first + p - 1 must all be defined above)");
            }
            for (int q = 0; q < 3; q++)
                if ((q < nin) != (row[1 + q] != -1))
                    return thfhe_fail(THFHE_E_INVALID, is_tree ? "TREE node: operands do not match lo.n_inputs + hi.n_inputs (unused ones are -1)"
                                                               : "SELECT node: operands do not match hi.n_inputs (unused ones are -1)");
            k = is_tree ? kDagTree : kDagSelect;
        } else if (mvx && (op == THFHE_MV || op == THFHE_TREE_MV)) {
            const bool is_tree = op == THFHE_TREE_MV;
            if (!luts->mvs) return thfhe_fail(THFHE_E_INVALID, "MV / TREE_MV node: no multi-value specs given (null table family)");
            if (row[4] < 0 || row[4] >= luts->n_mvs) return thfhe_fail(THFHE_E_INVALID, "MV / TREE_MV node: mv index out of range (0 .. n_mvs-1)");
            const thfhe_mv_spec &m = luts->mvs[row[4]];
            if (!(mv_ok[row[4]] & (is_tree ? 2 : 1))) {
                THFHE_TRY(dag_mv_spec_check(*luts, m, is_tree));
                mv_ok[row[4]] |= is_tree ? 2 : 1;
            }
            if (row[5] < 0 || row[5] >= m.n_tables) return thfhe_fail(THFHE_E_INVALID, "MV / TREE_MV node: table index out of range (0 .. n_tables-1)");
            nin = m.lo.n_inputs + (is_tree ? m.hi.n_inputs : 0);
            if (nin > 3) return thfhe_fail(THFHE_E_INVALID, "TREE_MV node: lo and hi operands exceed three");
            for (int q = 0; q < 3; q++)
                if ((q < nin) != (row[1 + q] != -1))
                    return thfhe_fail(THFHE_E_INVALID, is_tree ? "TREE_MV node: operands do not match lo.n_inputs + hi.n_inputs (unused ones are -1)"
                                                               : "MV node: operands do not match lo.n_inputs (unused ones are -1)");
            k = is_tree ? kDagTreeMv : kDagMv;
            head = w, pending = (is_tree ? m.k : m.q) - 1;
        } else if (lhe && (op == THFHE_LHE_LOOKUP || op == THFHE_LHE_GATHER)) {
            const bool gather = op == THFHE_LHE_GATHER;
            if (row[1] != -1 || row[2] != -1 || row[3] != -1) return thfhe_fail(THFHE_E_INVALID, "leveled node: the operand fields must be -1");
            if (!lhe->lks) return thfhe_fail(THFHE_E_INVALID, "LHE_LOOKUP / LHE_GATHER node: no lookup specs given (null family)");
            if (row[4] < 0 || row[4] >= lhe->n_lks) return thfhe_fail(THFHE_E_INVALID, "LHE_LOOKUP / LHE_GATHER node: lk out of range (0 .. n_lks-1)");
            const thfhe_dag_lhe_spec &ls = lhe->lks[row[4]];
            if (!(lk_ok[row[4]] & (gather ? 2 : 1))) {
                THFHE_TRY(dag_lhe_spec_check(*lhe, ls, gather));
                lk_ok[row[4]] |= gather ? 2 : 1;
            }
            if (gather) {
                cand_first = row[5], cand_count = (int32_t)1 << (ls.d_tree + ls.d_rot);
                if (cand_first < 0 || (long)cand_first + cand_count > (long)w)
                    return thfhe_fail(THFHE_E_INVALID, "LHE_GATHER node: candidate is not an earlier wire (first .. first + 2^d - 1 must all be defined above)");
            } else {
                if (!lhe->tab_b || lhe->n_tab_rows < 1) return thfhe_fail(THFHE_E_INVALID, "LHE_LOOKUP node: no table rows given (null family)");
                if (row[5] < 0 || (long)row[5] + (1L << ls.d_tree) > lhe->n_tab_rows)
                    return thfhe_fail(THFHE_E_INVALID, "LHE_LOOKUP node: row0 + 2^d_tree out of range (0 .. n_tab_rows)");
                head = w, pending = ls.theta - 1;
            }
            nin = 0;
            k = gather ? kDagLheGather : kDagLheLookup;
        } else if (lhe && op == THFHE_LHE_WFA) {
            if (row[1] != -1 || row[2] != -1 || row[3] != -1) return thfhe_fail(THFHE_E_INVALID, "leveled node: the operand fields must be -1");
            if (!lhe->wfas) return thfhe_fail(THFHE_E_INVALID, "LHE_WFA node: no automaton specs given (null family)");
            if (row[4] < 0 || row[4] >= lhe->n_wfas) return thfhe_fail(THFHE_E_INVALID, "LHE_WFA node: wfa out of range (0 .. n_wfas-1)");
            const thfhe_dag_wfa_spec &a = lhe->wfas[row[4]];
            if (!wfa_ok[row[4]]) {
                THFHE_TRY(dag_wfa_spec_check(*lhe, a));
                wfa_ok[row[4]] = 1;
            }
            if (!lhe->fin_b || lhe->n_fin_rows < 1) return thfhe_fail(THFHE_E_INVALID, "LHE_WFA node: no final weights given (null family)");
            if (row[5] < 0 || (long)row[5] + a.n_states > lhe->n_fin_rows)
                return thfhe_fail(THFHE_E_INVALID, "LHE_WFA node: fin_row0 + n_states out of range (0 .. n_fin_rows)");
            head = w, pending = a.n_out * a.theta - 1;
            nin = 0;
            k = kDagLheWfa;
        } else {
            k = classify(op);
            if (k < 0) return thfhe_fail(THFHE_E_INVALID, "gate opcode not defined for this engine");
            if (luts && (row[4] != -1 || row[5] != -1)) return thfhe_fail(THFHE_E_INVALID, "gate row: spec and lut must be -1");
            nin = k == 2 ? 1 : (k == 0 ? 2 : 3);
        }
        cls[g] = k;
        int32_t d = 0, s = 0;
        for (int q = 0; q < nin; q++) {
            const int32_t in = row[1 + q];
            if (in < 0 || in >= w) return thfhe_fail(THFHE_E_INVALID, "gate operand is not an earlier wire (gates must be in topological order)");
            if (depth[in] > d || (depth[in] == d && sub[in] > s)) d = depth[in], s = sub[in];
        }
        for (int32_t in = cand_first; in < cand_first + cand_count; in++)
            if (depth[in] > d || (depth[in] == d && sub[in] > s)) d = depth[in], s = sub[in];
        if (k == 2) s += 1; else d += 1, s = 0;
        depth[w] = d, sub[w] = s;
        if (d > max_depth) max_depth = d;
    }
    if (pending) return thfhe_fail(THFHE_E_INVALID, "LUT node: missing LUT_OUT row (theta - 1 of them must follow it)");
    plan.max_depth = max_depth;
    // bucket: (depth, sub, class); bootstrapped classes first (sub 0), then the linear sub-levels in order
    std::vector<std::vector<std::vector<int32_t>>> boot(max_depth + 1, std::vector<std::vector<int32_t>>(kDagSelect)), lin(max_depth + 1);
    std::vector<std::map<int32_t, std::vector<int32_t>>> sel(ext ? max_depth + 1 : 0), tre(ext ? max_depth + 1 : 0);   // per level, by trees[] index
    std::vector<std::map<int32_t, std::vector<int32_t>>> mvn(mvx ? max_depth + 1 : 0), tmv(mvx ? max_depth + 1 : 0);   // per level, by mvs[] index
    std::vector<std::map<int32_t, std::vector<int32_t>>> lhg[3];   // LOOKUP / GATHER / WFA nodes per level, by lks[] / wfas[] index
    for (auto &v : lhg) v.resize(lhe ? max_depth + 1 : 0);
    for (size_t g = 0; g < n_gates; g++) {
        const int32_t w = (int32_t)(n_inputs + g);
        if (cls[g] == kDagLutOut) continue;
        if (cls[g] == kDagSelect || cls[g] == kDagTree) {
            (cls[g] == kDagTree ? tre : sel)[depth[w]][gates[stride * g + 4]].push_back((int32_t)g);
        } else if (cls[g] == kDagMv || cls[g] == kDagTreeMv) {
            (cls[g] == kDagTreeMv ? tmv : mvn)[depth[w]][gates[stride * g + 4]].push_back((int32_t)g);
        } else if (cls[g] >= kDagLheLookup) {
            lhg[cls[g] - kDagLheLookup][depth[w]][gates[stride * g + 4]].push_back((int32_t)g);
        } else if (cls[g] == 2) {
            auto &L = lin[depth[w]];
            if ((int)L.size() < sub[w]) L.resize(sub[w]);
            L[sub[w] - 1].push_back((int32_t)g);
        } else {
            boot[depth[w]][cls[g]].push_back((int32_t)g);
        }
    }
    plan.tab.reserve(5 * n_gates);
    auto emit = [&](int32_t d, int32_t s, int32_t k, const std::vector<int32_t> &G, int32_t tree = -1) {
        if (G.empty()) return;
        DagBatch b{d, s, k, plan.tab.size(), G.size(), tree};
        const int cols = k >= 4 ? 7 : 5;   // LUT groups: + spec, lut
        for (int col = 0; col < cols; col++)
            for (int32_t g : G) {
                const int32_t *row = gates + stride * g;   // columns 5, 6 = row fields 4, 5 (spec, lut)
                plan.tab.push_back(col == 4 ? (int32_t)(n_inputs + g) : (col == 0 ? row[0] : (row[col < 4 ? col : col - 1] < 0 ? 0 : row[col < 4 ? col : col - 1])));
            }
        plan.batches.push_back(b);
        if (G.size() > plan.max_width) plan.max_width = G.size();
        size_t rot = k == 2 || k >= kDagLheLookup ? 0 : (k == 1 ? 2 * G.size() : G.size());   // a leveled node counts no blind rotation
        if (k == kDagTree) rot = G.size() * (size_t)(luts->trees[tree].p_hi / luts->trees[tree].lo.theta + 1);   // R level-1 rotations + the selection
        if (k == kDagTreeMv) rot = G.size() * (size_t)(1 + luts->mvs[tree].k);   // one multi-value rotation + k selections
        if (rot > plan.max_rot) plan.max_rot = rot;
        if (k >= 4 && k < kDagSelect && dag_lut_theta(k < kDagEnc ? k : k - 4) > plan.max_theta) plan.max_theta = dag_lut_theta(k < kDagEnc ? k : k - 4);
        plan.rotations += (int64_t)rot;
    };
    for (int32_t d = 0; d <= max_depth; d++) {
        for (int32_t k : {0, 3, 1, 4, 5, 6}) emit(d, 0, k, boot[d][k]);
        if (ext) {
            for (int32_t k : {8, 9, 10}) emit(d, 0, k, boot[d][k]);
            for (const auto &kv : sel[d]) emit(d, 0, kDagSelect, kv.second, kv.first);
            for (const auto &kv : tre[d]) emit(d, 0, kDagTree, kv.second, kv.first);
        }
        if (mvx) {
            for (const auto &kv : mvn[d]) emit(d, 0, kDagMv, kv.second, kv.first);
            for (const auto &kv : tmv[d]) emit(d, 0, kDagTreeMv, kv.second, kv.first);
        }
        if (lhe)
            for (int q = 0; q < 3; q++)
                for (const auto &kv : lhg[q][d]) emit(d, 0, kDagLheLookup + q, kv.second, kv.first);
        for (size_t q = 0; q < lin[d].size(); q++) emit(d, (int32_t)q + 1, 2, lin[d][q]);
    }
    return THFHE_OK;
}

// Host-side checks and plan of thfhe_dag_run_lut_batch / thfhe_mk_dag_run_lut_batch, before any device work and before the context is looked
// at: null pointers, the spec and table counts, every spec (the rules of lut_validate), the output wire ids, then dag_plan's row checks.
template <typename Classify>
int dag_lut_plan(const int32_t *inputs, size_t n_inputs, const int32_t *nodes, size_t n_nodes, const thfhe_lut_spec *specs, int n_specs, const void *tv,
                 int n_luts, const int32_t *out_wires, size_t n_out, const int32_t *outputs, Classify classify, DagPlan &plan) {
    if ((!inputs && n_inputs) || (!nodes && n_nodes) || (!outputs && n_nodes) || (!out_wires && n_out) || !specs || !tv)
        return thfhe_fail(THFHE_E_INVALID, "null argument");
    if (n_specs < 1 || n_specs > 1024) return thfhe_fail(THFHE_E_INVALID, "n_specs must be 1 .. 1024");
    if (n_luts < 1 || n_luts > 1024) return thfhe_fail(THFHE_E_INVALID, "n_luts must be 1 .. 1024");
    for (int s = 0; s < n_specs; s++)
        THFHE_TRY(lut_spec_check(specs[s]));
    for (size_t s = 0; s < n_out; s++)
        if (out_wires[s] < 0 || (size_t)out_wires[s] >= n_inputs + n_nodes) return thfhe_fail(THFHE_E_INVALID, "output wire id out of range");
    const DagLuts luts{specs, n_specs, n_luts};
    return dag_plan(nodes, n_inputs, n_nodes, classify, plan, &luts);
}

// Host-side checks and plan of thfhe_dag_run_tree_batch, before any device work and before either context is looked at: what
// dag_lut_plan checks (specs / tv may both be absent), the encrypted-table and level-1 row counts, every tree spec's `hi` half and p_hi (the rules of
// thfhe_tree_lut_bootstrap; the `lo` half when a TREE row uses the entry), then dag_plan's row checks with the three node kinds.
// mv (thfhe_dag_run_mv_batch): the multi-value families too -- their counts here, every mvs[] entry when a row uses it (dag_mv_spec_check);
// null: a run without them, which rejects MV and TREE_MV rows as opcodes it does not define.
struct DagMvFamilies {
    const thfhe_mv_spec *mvs;
    int n_mvs;
    const int32_t *tv0;
    int n_bases;
    const int32_t *factors;
    size_t n_factor_words;
};
template <typename Classify>
int dag_tree_plan(const int32_t *inputs, size_t n_inputs, const int32_t *nodes, size_t n_nodes, const thfhe_lut_spec *specs, int n_specs, const int32_t *tv,
                  int n_luts, const int32_t *enc_a, const int32_t *enc_b, int n_enc, const thfhe_tree_spec *trees, int n_trees, const int32_t *tv1,
                  int n_tv1_rows, const int32_t *out_wires, size_t n_out, const int32_t *outputs, Classify classify, DagPlan &plan,
                  const DagMvFamilies *mv = nullptr, const thfhe_dag_lhe_families *lhe = nullptr) {
    if ((!inputs && n_inputs) || (!nodes && n_nodes) || (!outputs && n_nodes) || (!out_wires && n_out)) return thfhe_fail(THFHE_E_INVALID, "null argument");
    if ((!specs && n_specs) || (!tv && n_luts) || ((!enc_a || !enc_b) && n_enc) || (!trees && n_trees) || (!tv1 && n_tv1_rows))
        return thfhe_fail(THFHE_E_INVALID, "null argument: a table family with a count but no pointer");
    if (n_specs < 0 || n_specs > 1024 || (specs && n_specs < 1)) return thfhe_fail(THFHE_E_INVALID, "n_specs must be 1 .. 1024 (0 with specs = NULL)");
    if (n_luts < 0 || n_luts > 1024 || (tv && n_luts < 1)) return thfhe_fail(THFHE_E_INVALID, "n_luts must be 1 .. 1024 (0 with tv = NULL)");
    if (n_enc < 0 || n_enc > (1 << 18)) return thfhe_fail(THFHE_E_INVALID, "n_enc must be 1 .. 262144 (0 with enc_a = enc_b = NULL)");
    if (n_trees < 0 || n_trees > 1024 || (trees && n_trees < 1)) return thfhe_fail(THFHE_E_INVALID, "n_trees must be 1 .. 1024 (0 with trees = NULL)");
    if (n_tv1_rows < 0 || n_tv1_rows > (1 << 18) || (tv1 && n_tv1_rows < 1)) return thfhe_fail(THFHE_E_INVALID, "n_tv1_rows must be 1 .. 262144 (0 with tv1 = NULL)");
    if (mv) {
        if ((!mv->mvs && mv->n_mvs) || (!mv->tv0 && mv->n_bases) || (!mv->factors && mv->n_factor_words))
            return thfhe_fail(THFHE_E_INVALID, "null argument: a table family with a count but no pointer");
        if (mv->n_mvs < 0 || mv->n_mvs > 1024 || (mv->mvs && mv->n_mvs < 1)) return thfhe_fail(THFHE_E_INVALID, "n_mvs must be 1 .. 1024 (0 with mvs = NULL)");
        if (mv->n_bases < 0 || mv->n_bases > 1024 || (mv->tv0 && mv->n_bases < 1)) return thfhe_fail(THFHE_E_INVALID, "n_bases must be 1 .. 1024 (0 with mv_tv0 = NULL)");
        if (mv->n_factor_words > ((size_t)1 << 28) || (mv->factors && mv->n_factor_words < 1))
            return thfhe_fail(THFHE_E_INVALID, "n_factor_words must be 1 .. 2^28 (0 with mv_factors = NULL)");
    }
    if (lhe) {
        if ((!lhe->sets && lhe->n_sets) || (!lhe->lks && lhe->n_lks) || (!lhe->tab_b && (lhe->n_tab_rows || lhe->tab_a)) || (!lhe->wfas && lhe->n_wfas) ||
            (!lhe->wfa_words && lhe->n_wfa_words) || (!lhe->fin_b && (lhe->n_fin_rows || lhe->fin_a)))
            return thfhe_fail(THFHE_E_INVALID, "null argument: a leveled family with a count but no pointer");
        if (lhe->n_sets < 0 || lhe->n_sets > 64 || (lhe->sets && lhe->n_sets < 1)) return thfhe_fail(THFHE_E_INVALID, "lhe: n_sets must be 1 .. 64 (0 with sets = NULL)");
        if (lhe->n_lks < 0 || lhe->n_lks > 1024 || (lhe->lks && lhe->n_lks < 1)) return thfhe_fail(THFHE_E_INVALID, "lhe: n_lks must be 1 .. 1024 (0 with lks = NULL)");
        if (lhe->n_wfas < 0 || lhe->n_wfas > 1024 || (lhe->wfas && lhe->n_wfas < 1)) return thfhe_fail(THFHE_E_INVALID, "lhe: n_wfas must be 1 .. 1024 (0 with wfas = NULL)");
        if (lhe->n_tab_rows < 0 || lhe->n_tab_rows > (1 << 18) || (lhe->tab_b && lhe->n_tab_rows < 1))
            return thfhe_fail(THFHE_E_INVALID, "lhe: n_tab_rows must be 1 .. 262144 (0 with tab_b = NULL)");
        if (lhe->n_fin_rows < 0 || lhe->n_fin_rows > (1 << 18) || (lhe->fin_b && lhe->n_fin_rows < 1))
            return thfhe_fail(THFHE_E_INVALID, "lhe: n_fin_rows must be 1 .. 262144 (0 with fin_b = NULL)");
        if (lhe->n_wfa_words > ((size_t)1 << 28) || (lhe->wfa_words && lhe->n_wfa_words < 1))
            return thfhe_fail(THFHE_E_INVALID, "lhe: n_wfa_words must be 1 .. 2^28 (0 with wfa_words = NULL)");
    }
    for (int s = 0; s < n_specs; s++)
        THFHE_TRY(lut_spec_check(specs[s]));
    for (int t = 0; t < n_trees; t++) {
        THFHE_TRY(lut_spec_check(trees[t].hi));
        if (trees[t].hi.theta != 1) return thfhe_fail(THFHE_E_INVALID, "tree: spec_hi theta must be 1 (the packed table holds one function)");
        const int p_hi = trees[t].p_hi;
        if (p_hi < 2 || p_hi > 512 || (p_hi & (p_hi - 1))) return thfhe_fail(THFHE_E_INVALID, "tree: p_hi must be a power of two in 2 .. N/2");
    }
    for (size_t s = 0; s < n_out; s++)
        if (out_wires[s] < 0 || (size_t)out_wires[s] >= n_inputs + n_nodes) return thfhe_fail(THFHE_E_INVALID, "output wire id out of range");
    DagLuts luts{specs, n_specs, n_luts};
    luts.ext = true, luts.n_enc = enc_a ? n_enc : 0, luts.trees = trees, luts.n_trees = n_trees, luts.n_tv1_rows = tv1 ? n_tv1_rows : 0;
    if (mv) {
        luts.mv = true, luts.mvs = mv->mvs, luts.n_mvs = mv->mvs ? mv->n_mvs : 0, luts.n_bases = mv->tv0 ? mv->n_bases : 0;
        luts.n_factor_words = mv->factors ? mv->n_factor_words : 0;
        luts.lhe = lhe;
    }
    return dag_plan(nodes, n_inputs, n_nodes, classify, plan, &luts);
}

// Device buffers of the executor (grow-only, owned by the engine's context and reused by every run on it).
struct DagBuffers {
    DevBuf wires, tab, ops, pack;
    DevBuf specs;   // thfhe_lut_spec[n_specs] of a LUT run
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
};

// Device-resident executor.  Level by level, each class of a level as slices of at most `slice_cap` gates over ALL instances: gather ->
// run(cls, d_ops, n) (the engine's prologue + blind rotations + key switch from its staging arrays stage_in[0..2] into stage_out) ->
// scatter.  Nothing synchronises with the host between levels.
//   h_inputs  int32[instances][n_inputs][words]
//   h_sel     wire ids to return (n_sel of them) or null = every gate wire [n_inputs, n_wires)
//   h_out     int32[instances][n_sel or n_gates][words]
// ensure(max_gates_per_slice) sizes the engine's workspace and staging and returns its staging pointers through the out-parameters.
// LUT and LUT_ENC launch groups: run_lut(theta, DagLutSlice) -> prologue + LUT rotation + key switch of the slice's nodes x theta records into
// the staging output, then the theta-record scatter into wires out[g] + j.  ensure sizes for plan.max_theta records per node.  SELECT / TREE
// groups (plans of thfhe_dag_run_tree_batch): run_ext(DagExtGroup) slices, runs and scatters the whole group.  An engine without run_ext
// rejects all three kinds.
template <typename Ensure, typename Run, typename RunLut = std::nullptr_t, typename RunExt = std::nullptr_t>
int dag_execute(const DagPlan &plan, DagBuffers &B, hipStream_t stream, int words, size_t n_inputs, size_t n_gates, size_t instances,
                const int32_t *h_inputs, const int32_t *h_sel, size_t n_sel, int32_t *h_out, size_t slice_cap, Ensure ensure, Run run,
                RunLut run_lut = nullptr, RunExt run_ext = nullptr) {
    const size_t n_wires = n_inputs + n_gates;
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
    hipError_t e = hipSuccess;
    if (n_inputs) e = hipMemcpy2DAsync(d_wires, n_wires * rec, h_inputs, n_inputs * rec, n_inputs * rec, instances, hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_tab, plan.tab.data(), plan.tab.size() * sizeof(int32_t), hipMemcpyHostToDevice, stream);
    if (e == hipSuccess && n_sel) e = hipMemcpyAsync(d_sel, h_sel, n_sel * sizeof(int32_t), hipMemcpyHostToDevice, stream);
    rc = e == hipSuccess ? THFHE_OK : thfhe_fail_hip(e, "gate-DAG executor: upload");
    const unsigned wb = (unsigned)((words + 255) / 256);
    const dim3 block(256);
    for (size_t b = 0; b < plan.batches.size() && rc == THFHE_OK; b++) {
        const long cnt = (long)plan.batches[b].count, all = cnt * (long)instances;
        const int cls = plan.batches[b].cls;
        const int32_t *t_ops = d_tab + plan.batches[b].off, *t0 = t_ops + cnt, *t1 = t0 + cnt, *t2 = t1 + cnt, *t_out = t2 + cnt;
        if (cls == 2) {
            hipLaunchKernelGGL(dag_wire_linear_kernel, dim3((unsigned)all, wb), block, 0, stream, d_wires, t0, t_out, t_ops, all, cnt, n_wires, words);
            continue;
        }
        if (cls >= kDagEnc && std::is_same_v<RunExt, std::nullptr_t>) {
            rc = thfhe_fail(THFHE_E_INVALID, "encrypted-table, select or tree node in a run without them");
            continue;
        }
        if (cls >= kDagSelect) {
            if constexpr (!std::is_same_v<RunExt, std::nullptr_t>)
                rc = run_ext(DagExtGroup{cls, plan.batches[b].tree, d_wires, t0, t1, t2, t_out, t_out + 2 * cnt, all, cnt, n_wires, plan.batches[b].off});
            continue;
        }
        if (cls >= 4) {   // LUT groups, and LUT_ENC groups over the run's encrypted tables
            if constexpr (std::is_same_v<RunLut, std::nullptr_t>) {
                rc = thfhe_fail(THFHE_E_INVALID, "LUT node in a gate-only run");
            } else {
                const bool enc = cls >= kDagEnc;
                const int theta = enc ? dag_enc_theta(cls) : dag_lut_theta(cls);
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
            if (cls != 0) hipLaunchKernelGGL(dag_gather_kernel, grid, block, 0, stream, d_wires, t2, stage_in[2], first, n, cnt, n_wires, words, nullptr, nullptr);
            rc = run(cls, d_ops, (size_t)n);
            if (!rc) hipLaunchKernelGGL(dag_scatter_kernel, grid, block, 0, stream, stage_out, t_out, d_wires, first, n, cnt, n_wires, words);
        }
    }
    if (rc == THFHE_OK) {
        e = hipGetLastError();
        if (e == hipSuccess && h_sel && n_sel) {
            const long all = (long)(n_sel * instances);
            hipLaunchKernelGGL(dag_gather_kernel, dim3((unsigned)all, wb), block, 0, stream, d_wires, d_sel, d_pack, 0L, all, (long)n_sel, n_wires, words, nullptr, nullptr);
            e = hipGetLastError();
            if (e == hipSuccess) e = hipMemcpyAsync(h_out, d_pack, instances * n_sel * rec, hipMemcpyDeviceToHost, stream);
        } else if (e == hipSuccess && !h_sel) {
            e = hipMemcpy2DAsync(h_out, n_gates * rec, d_wires + n_inputs * (size_t)words, n_wires * rec, n_gates * rec, instances, hipMemcpyDeviceToHost, stream);
        }
        if (e != hipSuccess) rc = thfhe_fail_hip(e, "gate-DAG executor");
    }
    e = hipStreamSynchronize(stream);
    if (rc == THFHE_OK && e != hipSuccess) rc = thfhe_fail_hip(e, "gate-DAG executor: sync");
    return rc;
}

}  // namespace

#endif  // THFHE_DAG_H
