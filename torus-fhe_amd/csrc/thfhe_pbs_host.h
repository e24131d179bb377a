// thfhe_pbs_host.h -- the programmable-bootstrap call bodies the single-key (thfhe_sk.hip) and 3-gen multi-key (thfhe_mk.hip) engines have in
// common: the flat LUT / encrypted-LUT call, the flat multi-value call, the host checks and the slice loop of a tree call, and dag_execute's
// ensure.  Function templates over the engine's context, like ctx_staged (thfhe_devctx.h); what differs per engine -- its workspace, its PBS
// stage, its tree chain -- comes in as a callable.  The table word (Torus32 / Torus64) follows the table pointer; the ring degree is c->p.N.
// Host code only: no kernels.
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
        lwe_linear_launch(d_in, d_w, d_bias, d_x, S, M, K, (int)rec, c->stream);
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
