// thfhe_pbs_host.h -- the programmable-bootstrap call bodies the single-key (thfhe_sk.hip) and 3-gen multi-key (thfhe_mk.hip) engines have in
// common: the flat LUT / encrypted-LUT call, the flat multi-value call, the host checks, the body and the slice loop of a flat tree call,
// dag_execute's ensure, and the grouped TREE / TREE_MV / MV / DENSE part of a gate-DAG run (table uploads, slice rule, reserve loop, group bodies);
// the leveled call bodies (TGSW sets, CMux, lookup) are thfhe_lhe_host.h's.
// Function templates over the engine's context, like ctx_staged (thfhe_devctx.h); what differs per engine -- its workspace rules, its PBS
// stage, its tree chain with its multi-value record -- comes in as a callable.  The engine keeps its locks, key checks, refusals, SELECT /
// leveled / CB groups and profiling wrapper.  The table word (Torus32 / Torus64) follows the table pointer or is named (dag_upload_families<T>,
// dag_run_group<T>); the ring degree is c->p.N.  Host code only: no kernels.
#ifndef THFHE_PBS_HOST_H
#define THFHE_PBS_HOST_H

#include <algorithm>
#include <vector>

#include "thfhe_dag.h"
#include "thfhe_devctx.h"
#include "thfhe_linear.h"
#include "thfhe_lut_prologue.h"

namespace {
using namespace thfhe;

constexpr int kMaxEncLuts = 1 << 18;   // encrypted tables of one call (every sample may bring its own), rows of one tree call

// thfhe_lut_bootstrap (keyswitch) / thfhe_lut_bootstrap_wo_keyswitch and their thfhe_mk_ forms: out = count x theta records of rec_words()
// (resp. N + 1) words.  enc: thfhe_lut_bootstrap_enc(_wo_keyswitch), the tables are ring samples (tv_a, tv) and up to kMaxEncLuts of them.
// grow(jobs, theta): the engine's workspace of a PBS stage; pbs(src, jobs, d_tv, d_tva, theta, d_idx, ks_dst, timed): its enqueue_pbs.
template <typename Ctx, typename T, typename Grow, typename Pbs>
int ctx_lut_bootstrap(Ctx *c, const thfhe_lut_spec *sp, const T *tv, const T *tv_a, bool enc, int n_luts, const int32_t *lut_index, const int32_t *in0,
                      const int32_t *in1, const int32_t *in2, int32_t *out, size_t count, bool keyswitch, Grow grow, Pbs pbs) {
    if (enc && !tv_a) return thfhe_fail(THFHE_E_INVALID, "null argument");
    THFHE_TRY(lut_validate(sp, tv, n_luts, lut_index, in0, in1, in2, out, count, enc ? kMaxEncLuts : 1024));
    if (!c) return thfhe_fail(THFHE_E_INVALID, "null ctx");
    if (count == 0) return THFHE_OK;
    const thfhe_lut_spec s = *sp;
    const size_t rec = c->rec_words(), in_words = count * rec, outs = count * s.theta, N = c->p.N;
    const size_t in_bytes = in_words * sizeof(int32_t), tv_bytes = (size_t)n_luts * N * sizeof(T);
    const size_t out_bytes = outs * (keyswitch ? rec : N + 1) * sizeof(int32_t);
    const size_t stage_words = keyswitch ? outs * rec : in_words;   // the key switch writes count x theta records into stage.out
    return ctx_staged(c, stage_words, {in0, s.n_inputs > 1 ? in1 : nullptr, s.n_inputs > 2 ? in2 : nullptr}, {in_bytes, in_bytes, in_bytes}, [&] {
        int r = c->d_tv.grow(tv_bytes);
        if (!r && enc) r = c->d_tva.grow(tv_bytes);
        if (!r && lut_index) r = c->d_lut_idx.grow(count * sizeof(int32_t));
        if (r) return r;
        THFHE_HIP(hipMemcpyAsync(c->d_tv.template as<T>(), tv, tv_bytes, hipMemcpyHostToDevice, c->stream));
        if (enc) THFHE_HIP(hipMemcpyAsync(c->d_tva.template as<T>(), tv_a, tv_bytes, hipMemcpyHostToDevice, c->stream));
        if (lut_index) THFHE_HIP(hipMemcpyAsync(c->d_lut_idx.template as<int32_t>(), lut_index, count * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
        THFHE_TRY(grow(count, s.theta));
        return pbs(LutFlatSrc<LutIdx::none>{c->stage.in_ptr(0), c->stage.in_ptr(1), c->stage.in_ptr(2), s, 1, nullptr}, count, c->d_tv.template as<T>(),
                   enc ? c->d_tva.template as<T>() : nullptr, s.theta, lut_index ? c->d_lut_idx.template as<int32_t>() : nullptr,
                   keyswitch ? c->stage.out_ptr() : nullptr, true);
    }, keyswitch ? c->stage.out : c->d_u, out, out_bytes);
}

// thfhe_mv_lut_bootstrap (keyswitch) / thfhe_mv_lut_bootstrap_wo_keyswitch and their thfhe_mk_ forms: out = count x q records
// of rec_words() (resp. N + 1) words, in slices of at most c->*slice records (at least one sample): only a slice's inputs go up and only its
// records come down (ctx_sliced).  grow(jobs, q): the engine's workspace; pbs(src, S, d_idx, ks_dst, last): its multi-value PBS stage of S samples
// on the base vector in c->d_tv and the taps in c->d_mv_w.
template <typename Ctx, typename T, typename Grow, typename Pbs>
int ctx_mv_lut_bootstrap(Ctx *c, const thfhe_lut_spec *sp, const T *tv0, const int32_t *factors, int p, int q, int n_tables, const int32_t *table_index,
                         const int32_t *in0, const int32_t *in1, const int32_t *in2, int32_t *out, size_t count, bool keyswitch, size_t Ctx::*slice, Grow grow,
                         Pbs pbs) {
    if (!factors) return thfhe_fail(THFHE_E_INVALID, "null argument");
    THFHE_TRY(lut_validate(sp, tv0, n_tables, table_index, in0, in1, in2, out, count));
    THFHE_TRY(mv_validate(*sp, p, q, n_tables));
    if (!c) return thfhe_fail(THFHE_E_INVALID, "null ctx");
    if (count == 0) return THFHE_OK;
    DevLock lk(*c);
    if (lk.rc) return lk.rc;
    const thfhe_lut_spec s = *sp;
    const size_t words = c->rec_words(), N = c->p.N;
    const size_t S_max = std::min(count, std::max<size_t>(1, c->*slice / q));
    const size_t w_bytes = (size_t)n_tables * q * p * sizeof(int32_t);
    int rc = grow(S_max, q);
    if (!rc) rc = c->stage.grow(keyswitch ? S_max * q * words : S_max * words);   // the key switch writes S x q records into stage.out
    if (!rc) rc = c->d_tv.grow(N * sizeof(T));
    if (!rc) rc = c->d_mv_w.grow(w_bytes);
    if (!rc && table_index) rc = c->d_lut_idx.grow(S_max * sizeof(int32_t));
    if (rc) return rc;
    THFHE_HIP(hipMemcpyAsync(c->d_tv.template as<T>(), tv0, N * sizeof(T), hipMemcpyHostToDevice, c->stream));
    THFHE_HIP(hipMemcpyAsync(c->d_mv_w.template as<int32_t>(), factors, w_bytes, hipMemcpyHostToDevice, c->stream));
    int32_t *const d_idx = c->d_lut_idx.template as<int32_t>();
    return ctx_sliced(c, count, S_max, {in0, s.n_inputs > 1 ? in1 : nullptr, s.n_inputs > 2 ? in2 : nullptr}, table_index, d_idx, [&](size_t, size_t S, bool last) {
        return pbs(LutFlatSrc<LutIdx::none>{c->stage.in_ptr(0), c->stage.in_ptr(1), c->stage.in_ptr(2), s, 1, nullptr}, S, table_index ? d_idx : nullptr,
                   keyswitch ? c->stage.out_ptr() : nullptr, last);
    }, keyswitch ? c->stage.out_ptr() : c->d_u.template as<int32_t>(), out, q * (keyswitch ? words : N + 1));
}

// thfhe_lwe_linear, thfhe_linear_lut_bootstrap(_wo_keyswitch) and their thfhe_mk_ forms: x = W in + bias per sample, and (fused) the PBS
// of every x[s][m] on table lut_index[m], theta records each.  In slices of whole samples (linear_plan, at most c->lin.slice jobs): only a slice's
// K input records per sample go up, lwe_linear_kernel writes its S M sums into c->lin.x, the engine's PBS stage reads them there as a flat
// one-input source (weight 1, bias 0: the instantiation of the flat LUT call), and only the slice's records come down (ctx_sliced).  The table
// indices repeat with period M and a slice starts at a whole sample, so one expanded array serves every slice.  fused false: out = x, and tv,
// theta (1), n_luts, lut_index, keyswitch, grow and pbs are not looked at.
template <typename Ctx, typename T, typename Grow, typename Pbs>
int ctx_linear(Ctx *c, const int32_t *W, const int32_t *bias, int M, int K, bool fused, int theta, const T *tv, int n_luts, const int32_t *lut_index,
               const int32_t *in, int32_t *out, size_t count, bool keyswitch, Grow grow, Pbs pbs) {
    THFHE_TRY(linear_validate(W, M, K, in, out, count, fused, tv, theta, n_luts, lut_index));
    if (!c) return thfhe_fail(THFHE_E_INVALID, "null ctx");
    if (count == 0) return THFHE_OK;
    DevLock lk(*c);
    if (lk.rc) return lk.rc;
    const size_t rec = c->rec_words(), N = c->p.N, out_rec = fused && !keyswitch ? N + 1 : rec;
    const size_t S_max = linear_plan::samples_per_slice(count, (size_t)M, c->lin.slice), jobs_max = S_max * M;
    const size_t w_bytes = (size_t)M * K * sizeof(int32_t), tv_bytes = (size_t)n_luts * N * sizeof(T);
    int rc = c->lin.w.grow(w_bytes);
    if (!rc && bias) rc = c->lin.bias.grow(M * sizeof(int32_t));
    if (!rc) rc = c->lin.in.grow(S_max * K * rec * sizeof(int32_t));
    if (!rc) rc = c->lin.x.grow(jobs_max * rec * sizeof(int32_t));
    if (!rc && fused) rc = grow(jobs_max, theta);
    if (!rc && fused) rc = c->d_tv.grow(tv_bytes);
    if (!rc && fused && keyswitch) rc = c->stage.out.grow(jobs_max * theta * rec * sizeof(int32_t));
    if (!rc && fused && lut_index) rc = c->d_lut_idx.grow(jobs_max * sizeof(int32_t));
    if (rc) return rc;
    int32_t *const d_in = c->lin.in.template as<int32_t>(), *const d_x = c->lin.x.template as<int32_t>();
    int32_t *const d_w = c->lin.w.template as<int32_t>(), *const d_bias = bias ? c->lin.bias.template as<int32_t>() : nullptr;
    int32_t *const d_idx = fused && lut_index ? c->d_lut_idx.template as<int32_t>() : nullptr;
    THFHE_HIP(hipMemcpyAsync(d_w, W, w_bytes, hipMemcpyHostToDevice, c->stream));
    if (bias) THFHE_HIP(hipMemcpyAsync(d_bias, bias, M * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    std::vector<int32_t> idx;   // lives until ctx_sliced has drained the stream
    if (fused) THFHE_HIP(hipMemcpyAsync(c->d_tv.template as<T>(), tv, tv_bytes, hipMemcpyHostToDevice, c->stream));
    if (d_idx) {
        idx.resize(jobs_max);
        for (size_t j = 0; j < jobs_max; j++) idx[j] = lut_index[j % M];
        THFHE_HIP(hipMemcpyAsync(d_idx, idx.data(), jobs_max * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    }
    const int32_t *const res = !fused ? d_x : keyswitch ? c->stage.out_ptr() : c->d_u.template as<int32_t>();
    return ctx_sliced(c, count, S_max, {nullptr, nullptr, nullptr}, nullptr, nullptr, [&](size_t s0, size_t S, bool last) {
        const linear_plan::Slice sl = linear_plan::slice_at(s0 / S_max, count, S_max, M, K, theta, rec, out_rec);
        const bool ev = last && c->profiling;   // thfhe_linear_last_timings: the last slice's upload and kernel
        if (ev) THFHE_TRY(c->lin.events());
        if (ev) THFHE_HIP(hipEventRecord(c->lin.ev[0], c->stream));
        THFHE_HIP(hipMemcpyAsync(d_in, in + sl.in_off, S * K * rec * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
        if (ev) THFHE_HIP(hipEventRecord(c->lin.ev[1], c->stream));
        lwe_linear_launch(LinFlatSrc{d_in}, d_w, d_bias, d_x, S, M, K, (int)rec, c->stream);
        if (ev) THFHE_HIP(hipEventRecord(c->lin.ev[2], c->stream));
        if (ev) c->lin.ev_valid = true, c->lin.ev_whole = fused && keyswitch;
        THFHE_HIP(hipGetLastError());
        if (!fused) return (int)THFHE_OK;
        return pbs(LutFlatSrc<LutIdx::none>{d_x, d_x, d_x, thfhe_lut_spec{1, {1, 0, 0}, 0, theta}, 1, nullptr}, sl.jobs, c->d_tv.template as<T>(), (const T *)nullptr,
                   theta, d_idx, keyswitch ? c->stage.out_ptr() : nullptr, last);
    }, res, out, (size_t)M * theta * out_rec);
}

// ---- the two-digit tree ----
// what an engine's tree call admits: the largest p_hi and the texts of its p_hi and n_tables refusals
struct TreeRules {
    int p_hi_max;
    const char *p_hi_text, *n_tables_text;
};

// host checks of a tree call that need no context: pointers, both specs, p_hi
inline int tree_validate(const TreeRules &rules, const thfhe_lut_spec *spec_lo, const thfhe_lut_spec *spec_hi, int p_hi, const void *tv, const int32_t *lo0,
                         const int32_t *lo1, const int32_t *lo2, const int32_t *hi0, const int32_t *hi1, const int32_t *hi2, const int32_t *out) {
    if (!spec_lo || !spec_hi || !tv || !lo0 || !hi0 || !out) return thfhe_fail(THFHE_E_INVALID, "null argument");
    THFHE_TRY(lut_spec_check(*spec_lo));
    THFHE_TRY(lut_spec_check(*spec_hi));
    if ((spec_lo->n_inputs > 1 && !lo1) || (spec_lo->n_inputs > 2 && !lo2) || (spec_hi->n_inputs > 1 && !hi1) || (spec_hi->n_inputs > 2 && !hi2))
        return thfhe_fail(THFHE_E_INVALID, "null operand: the spec names more inputs");
    if (spec_hi->theta != 1) return thfhe_fail(THFHE_E_INVALID, "tree: spec_hi theta must be 1 (the packed table holds one function)");
    if (p_hi < 2 || p_hi > rules.p_hi_max || (p_hi & (p_hi - 1))) return thfhe_fail(THFHE_E_INVALID, rules.p_hi_text);
    return THFHE_OK;
}
inline int tree_validate_index(const int32_t *table_index, int n_tables, size_t count) {
    if (count > (size_t)INT32_MAX / 16) return thfhe_fail(THFHE_E_INVALID, "count too large");
    if (table_index)
        for (size_t g = 0; g < count; g++)
            if (table_index[g] < 0 || table_index[g] >= n_tables) return thfhe_fail(THFHE_E_INVALID, "table_index out of range (0 .. n_tables-1)");
    return THFHE_OK;
}
// ... of thfhe_tree_lut_bootstrap / thfhe_mk_tree_lut_bootstrap, whose level 1 rotates n_tables x p_hi / theta_lo plaintext rows: those, then
// theta_lo | p_hi, the tables and their indices
inline int tree_validate_rows(const TreeRules &rules, const thfhe_lut_spec *spec_lo, const thfhe_lut_spec *spec_hi, int p_hi, const void *tv1, int n_tables,
                              const int32_t *table_index, const int32_t *lo0, const int32_t *lo1, const int32_t *lo2, const int32_t *hi0, const int32_t *hi1,
                              const int32_t *hi2, const int32_t *out, size_t count) {
    THFHE_TRY(tree_validate(rules, spec_lo, spec_hi, p_hi, tv1, lo0, lo1, lo2, hi0, hi1, hi2, out));
    if (p_hi % spec_lo->theta) return thfhe_fail(THFHE_E_INVALID, "tree: spec_lo theta must divide p_hi");
    if (n_tables < 1 || (size_t)n_tables * (p_hi / spec_lo->theta) > (size_t)kMaxEncLuts) return thfhe_fail(THFHE_E_INVALID, rules.n_tables_text);
    return tree_validate_index(table_index, n_tables, count);
}

// The slice loop of a tree call, the caller having locked the context and sized every buffer for S_max samples: ctx_sliced on the `lo` operands
// and the slice's table indices (into d_tree_tab), with the engine's chain(S, first, last, upload_hi) as its run.  The chain enqueues level 1,
// packing and selection into stage.out -- k records per sample -- and calls upload_hi() at its seam, once level 1 is enqueued: the slice's `hi`
// operands replace the `lo` ones in the staging arrays.  first / last: the call's first / last slice (where the chain records its profiling events).
template <typename Ctx, typename Chain>
int ctx_tree_sliced(Ctx *c, size_t count, size_t S_max, const thfhe_lut_spec &lo, const thfhe_lut_spec &hi, const int32_t *table_index, const int32_t *lo0,
                    const int32_t *lo1, const int32_t *lo2, const int32_t *hi0, const int32_t *hi1, const int32_t *hi2, int32_t *out, size_t k, Chain chain) {
    const size_t words = c->rec_words();
    const int32_t *const hi_in[3] = {hi0, hi.n_inputs > 1 ? hi1 : nullptr, hi.n_inputs > 2 ? hi2 : nullptr};
    return ctx_sliced(c, count, S_max, {lo0, lo.n_inputs > 1 ? lo1 : nullptr, lo.n_inputs > 2 ? lo2 : nullptr}, table_index, c->d_tree_tab.template as<int32_t>(),
                      [&](size_t s0, size_t S, bool last) {
        return chain(S, s0 == 0, last, [&] {
            for (int q = 0; q < 3; q++)
                if (hi_in[q]) THFHE_HIP(hipMemcpyAsync(c->stage.in_ptr(q), hi_in[q] + s0 * words, S * words * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
            return (int)THFHE_OK;
        });
    }, c->stage.out_ptr(), out, k * words);
}

// The flat tree call (thfhe_tree_lut_bootstrap(_mv)(k) and their thfhe_mk_ forms), the engine having locked the context and checked its packing key:
// per slice of S samples one chain on contiguous operands -- level 1 on the rows tv[table[s]][r] (tv_rows rows of N words in all) and the `lo`
// operands, the selection on the `hi` operands.  Only a slice's inputs go up and its records come down.  factors: level 1 is one
// multi-value rotation per sample of the base vector tv with the k p_hi factors of p_lo taps of table[s], int32[n_tables][k][p_hi][p_lo]; k tables
// per sample, out int32[count][k][rec_words()].  ws(S, p, R, theta_lo, k): the engine's tree workspace rule;
// chain(lo, d_tv1, theta_lo, hi, S, p, seam, w, mv_p, k): its tree chain into stage.out, w the taps of a multi-value level 1 (null: rows).
// Profiling: level 1 | packing | selection of the last slice in ev[1..3]; ev[0] on the call's first slice (ev0_first) or on its last.
template <typename Ctx, typename T, typename Ws, typename Chain>
int ctx_tree_bootstrap(Ctx *c, const thfhe_lut_spec &lo, const thfhe_lut_spec &hi, int p_hi, const T *tv, size_t tv_rows, const int32_t *factors, int p_lo,
                       int n_tables, const int32_t *table_index, const int32_t *lo0, const int32_t *lo1, const int32_t *lo2, const int32_t *hi0,
                       const int32_t *hi1, const int32_t *hi2, int32_t *out, size_t count, int k, bool ev0_first, Ws ws, Chain chain) {
    if (count == 0) return THFHE_OK;
    const size_t words = c->rec_words(), K = (size_t)k;
    const int theta1 = factors ? k * p_hi : lo.theta, R = k * p_hi / theta1;   // level-1 records per rotation, rotations per sample
    const size_t S_max = std::min(count, std::max<size_t>(1, c->tree_slice / (K * p_hi)));
    const size_t tv_bytes = tv_rows * c->p.N * sizeof(T), w_bytes = factors ? (size_t)n_tables * K * p_hi * p_lo * sizeof(int32_t) : 0;
    int rc = c->d_tv.grow(tv_bytes);
    if (!rc && factors) rc = c->d_mv_w.grow(w_bytes);
    if (!rc) rc = ws(S_max, (size_t)p_hi, (size_t)R, (size_t)theta1, K);
    if (!rc) rc = c->stage.grow(S_max * K * words);
    if (!rc && table_index) rc = c->d_tree_tab.grow(S_max * sizeof(int32_t));
    if (rc) return rc;
    hipStream_t st = c->stream;
    THFHE_HIP(hipMemcpyAsync(c->d_tv.template as<T>(), tv, tv_bytes, hipMemcpyHostToDevice, st));
    if (factors) THFHE_HIP(hipMemcpyAsync(c->d_mv_w.template as<int32_t>(), factors, w_bytes, hipMemcpyHostToDevice, st));
    const int32_t *const in0 = c->stage.in_ptr(0), *const in1 = c->stage.in_ptr(1), *const in2 = c->stage.in_ptr(2);   // `lo`, then `hi` operands of the slice
    const LutFlatSrc<LutIdx::table> lo_src{in0, in1, in2, lo, R, table_index ? c->d_tree_tab.template as<int32_t>() : nullptr};
    const LutFlatSrc<LutIdx::job> hi_src{in0, in1, in2, hi, k, nullptr};
    return ctx_tree_sliced(c, count, S_max, lo, hi, table_index, lo0, lo1, lo2, hi0, hi1, hi2, out, K, [&](size_t S, bool first, bool last, auto upload_hi) {
        const bool ev = c->profiling && last;
        if (c->profiling && (ev0_first ? first : last)) THFHE_HIP(hipEventRecord(c->ev[0], st));
        auto seam = [&](int stage) {
            if (ev) THFHE_HIP(hipEventRecord(c->ev[stage], st));
            return stage == 2 ? upload_hi() : (int)THFHE_OK;
        };
        THFHE_TRY(chain(lo_src, c->d_tv.template as<T>(), theta1, hi_src, S, p_hi, seam, factors ? c->d_mv_w.template as<int32_t>() : nullptr, p_lo, K));
        if (ev) {
            THFHE_HIP(hipEventRecord(c->ev[3], st));
            c->ev_valid = true;
        }
        return (int)THFHE_OK;
    });
}

// ---- the grouped TREE / TREE_MV / MV kinds of a gate-DAG run ----
// The run's tables and specs into their grow-only device buffers, once per call (T: the table word; F.enc_a / enc_b / tv1 are words of T too).
template <typename T, typename Ctx>
int dag_upload_families(Ctx *c, hipStream_t st, const DagFamilies &F) {
    const size_t row = c->p.N * sizeof(T);
    THFHE_TRY(dag_upload(c->d_tv, st, F.tv, F.n_luts * row));
    THFHE_TRY(dag_upload(c->dag.specs, st, F.specs, (size_t)F.n_specs * sizeof(thfhe_lut_spec)));
    THFHE_TRY(dag_upload(c->d_dag_enc_a, st, F.enc_a, F.n_enc * row));
    THFHE_TRY(dag_upload(c->d_dag_enc_b, st, F.enc_b, F.n_enc * row));
    THFHE_TRY(dag_upload(c->d_dag_tv1, st, F.tv1, F.n_tv1_rows * row));
    THFHE_TRY(dag_upload(c->d_dag_mv_tv0, st, F.mv_tv0, F.n_bases * row));
    if (F.dense) {   // the dense layers' word pool and operand wire ids
        THFHE_TRY(dag_upload(c->lin.dag_words, st, F.dense->words, F.dense->n_words * sizeof(int32_t)));
        THFHE_TRY(dag_upload(c->lin.dag_wires, st, F.dense->wires, F.dense->n_wires * sizeof(int32_t)));
    }
    return dag_upload(c->d_dag_mv_w, st, F.mv_factors, F.n_factor_words * sizeof(int32_t));
}

// A slice of a grouped kind's `all` nodes over all instances: at most dag_slice of them, and the flat calls' workspace rules -- tree_slice / p_hi
// nodes of a SELECT / TREE group, tree_slice / (k q) of a TREE_MV group, c->*mv_slice / q of an MV group, lin.slice / M samples of a DENSE group
// (a sample = one node of one instance: M PBS jobs, thfhe_set_linear_slice's cap).
template <typename Ctx>
size_t dag_group_slice(const Ctx *c, const DagFamilies &F, int cls, int entry, size_t all, size_t Ctx::*mv_slice) {
    if (cls == kDagDense) return std::min({all, c->dag_slice, std::max<size_t>(1, c->lin.slice / (size_t)F.dense->layers[entry].M)});
    const bool mv = cls == kDagMv || cls == kDagTreeMv;
    const size_t per = cls == kDagMv ? c->*mv_slice / (size_t)F.mvs[entry].q : c->tree_slice / (mv ? (size_t)F.mvs[entry].k * F.mvs[entry].q : (size_t)F.trees[entry].p_hi);
    return std::min({all, c->dag_slice, std::max<size_t>(1, per)});
}

// Every buffer the slices of the plan's TREE / TREE_MV / MV / DENSE groups use, the staging output included, before dag_execute takes pointers.
// tree_ws(S, p, R, theta_lo, k) / pbs_ws(jobs, theta): the engine's workspace rules; w_cand: raised to the most candidates (S k p) a slice packs.
template <typename Ctx, typename TreeWs, typename PbsWs>
int dag_reserve_groups(Ctx *c, const DagPlan &plan, const DagFamilies &F, size_t instances, size_t Ctx::*mv_slice, size_t &w_cand, TreeWs tree_ws, PbsWs pbs_ws) {
    for (const DagBatch &b : plan.batches) {
        if (b.cls != kDagTree && b.cls != kDagTreeMv && b.cls != kDagMv && b.cls != kDagDense) continue;
        const size_t S = dag_group_slice(c, F, b.cls, b.tree, b.count * instances, mv_slice);
        size_t outs = 1;
        if (b.cls == kDagDense) {   // S samples: S M sums in lin.x, as many PBS jobs of theta records, their table indices
            const thfhe_dag_dense_spec &l = F.dense->layers[b.tree];
            const size_t jobs = S * (size_t)l.M;
            THFHE_TRY(c->lin.x.grow(jobs * c->rec_words() * sizeof(int32_t)));
            THFHE_TRY(pbs_ws(jobs, l.theta));
            THFHE_TRY(c->d_lut_idx.grow(jobs * sizeof(int32_t)));
            THFHE_TRY(c->stage.out.grow(jobs * l.theta * c->rec_words() * sizeof(int32_t)));
            continue;
        }
        if (b.cls == kDagMv) {
            outs = (size_t)F.mvs[b.tree].q;
            THFHE_TRY(pbs_ws(S, (int)outs));
            THFHE_TRY(c->d_lut_idx.grow(S * sizeof(int32_t)));
        } else {
            const bool mv = b.cls == kDagTreeMv;
            const size_t k = mv ? (size_t)F.mvs[b.tree].k : 1, p = mv ? (size_t)F.mvs[b.tree].q : (size_t)F.trees[b.tree].p_hi;
            const size_t theta_lo = mv ? k * p : (size_t)F.trees[b.tree].lo.theta;
            THFHE_TRY(tree_ws(S, p, k * p / theta_lo, theta_lo, k));
            w_cand = std::max(w_cand, S * k * p), outs = k;
        }
        THFHE_TRY(c->stage.out.grow(S * outs * c->rec_words() * sizeof(int32_t)));
    }
    return THFHE_OK;
}

// One TREE / TREE_MV / MV group of a level, in slices (dag_group_slice) with every prologue reading the wire table.  A TREE group runs the flat
// tree's chain on the run's level-1 rows (t_y = row0), the index operands of a node following its lo.n_inputs level-1 operands.  An MV group is one
// multi-value PBS stage on its base vector (t_y = each node's table), its q records per node scattered into consecutive wires; a TREE_MV group the
// k-table chain, record [first + s][j] going to wire head + j.  chain: as ctx_tree_bootstrap's; mv_pbs(lo, S, tv0, w, mv_p, q): the engine's
// multi-value PBS stage of S nodes into stage.out.
template <typename T, typename Ctx, typename Chain, typename MvPbs>
int dag_run_group(Ctx *c, const DagFamilies &F, const DagExtGroup &g, size_t Ctx::*mv_slice, Chain chain, MvPbs mv_pbs) {
    const int words = c->rec_words();
    const size_t slice = dag_group_slice(c, F, g.cls, g.tree, (size_t)g.all, mv_slice);
    auto no_seam = [](int) { return (int)THFHE_OK; };
    const int32_t *col[5] = {g.t0, g.t1, g.t2, g.t2, g.t2};
    if (g.cls == kDagTree) {
        const thfhe_tree_spec ts = F.trees[g.tree];
        const int p = ts.p_hi, hi0 = ts.lo.n_inputs;
        return dag_group_slices(g, slice, 1, c->stage.out_ptr(), words, c->stream, [&](long first, long S) {
            const LutWireSrc<LutSpecByValue, LutIdx::table> lo{g.wires, g.t0, g.t1, g.t2, {ts.lo}, g.t_y, first, g.cnt, g.n_wires, p / ts.lo.theta};
            const LutWireSrc<LutSpecByValue, LutIdx::job> hi{g.wires, col[hi0], col[hi0 + 1], col[hi0 + 2], {ts.hi}, nullptr, first, g.cnt, g.n_wires, 1};
            return chain(lo, c->d_dag_tv1.template as<T>(), ts.lo.theta, hi, (size_t)S, p, no_seam, (const int32_t *)nullptr, 0, (size_t)1);
        });
    }
    const thfhe_mv_spec m = F.mvs[g.tree];
    const bool is_tree = g.cls == kDagTreeMv;
    const int hi0 = m.lo.n_inputs;
    const T *const tv0 = c->d_dag_mv_tv0.template as<T>() + (size_t)m.base * c->p.N;
    const int32_t *const w = c->d_dag_mv_w.template as<int32_t>() + m.factors_off;
    return dag_group_slices(g, slice, is_tree ? m.k : m.q, c->stage.out_ptr(), words, c->stream, [&](long first, long S) {
        const LutWireSrc<LutSpecByValue, LutIdx::table> lo{g.wires, g.t0, g.t1, g.t2, {m.lo}, g.t_y, first, g.cnt, g.n_wires, 1};
        if (!is_tree) return mv_pbs(lo, (size_t)S, tv0, w, m.p, m.q);
        const LutWireSrc<LutSpecByValue, LutIdx::job> hi{g.wires, col[hi0], col[hi0 + 1], col[hi0 + 2], {m.hi}, nullptr, first, g.cnt, g.n_wires, m.k};
        return chain(lo, tv0, m.k * m.q, hi, (size_t)S, m.q, no_seam, w, m.p, (size_t)m.k);
    });
}

// One DENSE group of a level, in slices of whole samples (dag_group_slice): lwe_linear_kernel reads the K operand records of every
// sample in place from the wire table (LinWireSrc: the group's wire_off column into the run's wire pool) and writes the slice's S M sums into
// lin.x; the engine's PBS stage reads them there as the flat call does (weight 1, bias 0, the table of job j = lut[j mod M], built once per group:
// a slice starts at a whole sample) and key-switches into stage.out; record [j][m][t] of the slice goes to wire head + m theta + t.
// pbs(src, jobs, d_tv, d_tva, theta, d_idx, ks_dst, timed): the engine's enqueue_pbs.  Profiling: the events of thfhe_linear_last_timings around the
// last slice's kernel (no upload: ev[0] = ev[1]), and the PBS stage of the group's last slice is a timed one (thfhe_last_timings).
template <typename T, typename Ctx, typename Pbs>
int dag_run_dense_group(Ctx *c, const DagFamilies &F, const DagExtGroup &g, size_t Ctx::*mv_slice, Pbs pbs) {
    const thfhe_dag_dense_spec l = F.dense->layers[g.tree];
    const int rec = c->rec_words();
    const size_t slice = dag_group_slice(c, F, g.cls, g.tree, (size_t)g.all, mv_slice);
    const int32_t *const words = c->lin.dag_words.template as<int32_t>(), *const pool = c->lin.dag_wires.template as<int32_t>();
    const int32_t *const bias = l.bias_off >= 0 ? words + l.bias_off : nullptr;
    int32_t *const d_x = c->lin.x.template as<int32_t>();
    int32_t *d_idx = nullptr;
    if (l.lut_off >= 0) {
        d_idx = c->d_lut_idx.template as<int32_t>();
        const long jobs = (long)slice * l.M;
        hipLaunchKernelGGL(dense_lut_idx_kernel, dim3((unsigned)std::min<long>((jobs + 255) / 256, 1024)), dim3(256), 0, c->stream, words + l.lut_off, d_idx, jobs, l.M);
        THFHE_HIP(hipGetLastError());
    }
    return dag_group_slices(g, slice, l.M * l.theta, c->stage.out_ptr(), rec, c->stream, [&](long first, long S) {
        const bool ev = c->profiling;
        if (ev) THFHE_TRY(c->lin.events());
        if (ev) THFHE_HIP(hipEventRecord(c->lin.ev[0], c->stream));
        if (ev) THFHE_HIP(hipEventRecord(c->lin.ev[1], c->stream));
        lwe_linear_launch(LinWireSrc{g.wires, pool, g.t0, first, g.cnt, g.n_wires}, words + l.w_off, bias, d_x, (size_t)S, l.M, l.K, rec, c->stream);
        if (ev) THFHE_HIP(hipEventRecord(c->lin.ev[2], c->stream));
        if (ev) c->lin.ev_valid = true, c->lin.ev_whole = false;
        THFHE_HIP(hipGetLastError());
        return pbs(LutFlatSrc<LutIdx::none>{d_x, d_x, d_x, thfhe_lut_spec{1, {1, 0, 0}, 0, l.theta}, 1, nullptr}, (size_t)S * l.M, c->d_tv.template as<T>(), (const T *)nullptr,
                   l.theta, (const int32_t *)d_idx, c->stage.out_ptr(), first + S >= g.all);
    });
}

// dag_execute's ensure: workspace and staging for slices of max_gates gates; theta_max > 0: a run with LUT groups of up to theta_max records per
// node.  grow(jobs, theta): the engine's workspace of `jobs` rotations (theta 0: a gate's) or PBS jobs of theta records.
template <typename Ctx, typename Grow>
int dag_ensure(Ctx *c, size_t max_gates, int theta_max, int32_t **in, int32_t **out, Grow grow) {
    const size_t words = c->rec_words();
    int r = grow(2 * max_gates, 0);
    if (!r && theta_max) r = grow(max_gates, theta_max);
    if (!r && theta_max) r = c->d_lut_idx.grow(max_gates * sizeof(int32_t));
    if (!r) r = c->stage.grow(max_gates * words);
    if (!r && theta_max) r = c->stage.out.grow(theta_max * max_gates * words * sizeof(int32_t));   // key switch of nodes x theta records
    in[0] = c->stage.in_ptr(0), in[1] = c->stage.in_ptr(1), in[2] = c->stage.in_ptr(2), *out = c->stage.out_ptr();
    return r;
}

}  // namespace

#endif  // THFHE_PBS_HOST_H
