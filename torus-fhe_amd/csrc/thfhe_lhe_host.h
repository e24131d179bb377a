// thfhe_lhe_host.h -- the leveled call bodies the single-key (thfhe_lhe.h) and 3-gen multi-key (thfhe_mk_lhe.h) engines have
// in common: creation and destruction of a TGSW set, the range and context checks of a call on a set, the flat CMux call, the launch chain of a
// leveled lookup (CMux tree, rotation, key switch, profiling events) and the lookup call with its host checks, slice rule and slice loop.
// Function templates over the engine's context, its set and its ring word (Torus32 / Torus64), like the ctx_* bodies of thfhe_pbs_host.h; what
// differs per engine -- ring degree, bounds, slice cap, spectra per sample, refusal texts -- is its LheRules, and its launches, key switch and set
// fill come in as callables.  The engine keeps its kernels, their argument structs and launchers.  Host code only: no kernels.
#ifndef THFHE_LHE_HOST_H
#define THFHE_LHE_HOST_H

#include <algorithm>
#include <memory>
#include <mutex>
#include <new>

#include "thfhe_devctx.h"
#include "thfhe_pbs_host.h"

namespace {
using namespace thfhe;

constexpr int kLheMaxBits = 16, kLheMaxTree = 6;   // address bits of a set, levels of a CMux tree

// what an engine's leveled calls admit and how they refuse
template <typename Ctx>
struct LheRules {
    int N;               // ring degree, the one source of it in these bodies: the checks that come before the context need it, so it is not c->p.N
    int d_rot_max;       // log2 N
    size_t cmux_slice;   // samples per launch of the flat CMux
    size_t (*sample_slots)(const Ctx *, int d);   // complex slots of the spectra of one sample of a set of d bits
    const char *set_d_text, *set_count_text, *range_text, *ctx_text, *bit_text;
    const char *d_tree_text, *d_rot_text, *theta_text, *box_text, *n_tables_text, *d_sum_text;
};

// One CMux launch, as the shared bodies describe it: out(s, p) = d0(s, p) + C_(s,bit) (.) (d1(s, p) - d0(s, p)).  Word offsets: inputs at
// index(s) * in_sample + p * in_pair, index(s) = in_idx[s] or s; output at s * out_sample + p * out_pair.  spec: the spectra at the launch's first
// sample.  pub: the masks are known to be zero (null d0_a / d1_a).  The engine turns it into its kernel's argument struct.
template <typename T>
struct LheCmuxIo {
    const cplx *spec;
    const T *d0_a, *d0_b, *d1_a, *d1_b;
    T *out_a, *out_b;
    const int32_t *in_idx;
    size_t in_sample, in_pair, out_sample, out_pair;
    int bit;
    bool pub;
};

// thfhe_tgsw_set_create / thfhe_mk_tgsw_set_create: the host checks and the allocation; fill(c, set, tgsw) is the engine's size check, upload
// and transform
template <typename Set, typename Ctx, typename T, typename Fill>
int ctx_tgsw_set_create(Ctx *c, const T *tgsw, size_t count, int d, Set **out, const LheRules<Ctx> &rules, Fill fill) {
    if (!tgsw || !out) return thfhe_fail(THFHE_E_INVALID, "null argument");
    *out = nullptr;
    if (d < 1 || d > kLheMaxBits) return thfhe_fail(THFHE_E_INVALID, rules.set_d_text);
    if (count < 1 || count > ((size_t)1 << 24)) return thfhe_fail(THFHE_E_INVALID, rules.set_count_text);
    if (!c) return thfhe_fail(THFHE_E_INVALID, "null ctx");
    std::unique_ptr<Set> set(new (std::nothrow) Set);
    if (!set) return thfhe_fail(THFHE_E_NOMEM, "out of host memory");
    set->ctx = c, set->count = count, set->d = d;
    const int rc = fill(c, set.get(), tgsw);
    if (rc) {   // nothing is left behind: the spectra are freed on the context's device
        (void)hipSetDevice(c->device);
        return rc;
    }
    *out = set.release();
    return THFHE_OK;
}

template <typename Set>
void ctx_tgsw_set_destroy(Set *set) {
    if (!set) return;
    {
        std::lock_guard<std::mutex> g(set->ctx->mu);   // a call still running on another thread finishes first
        (void)hipSetDevice(set->ctx->device);
        (void)hipStreamSynchronize(set->ctx->stream);
    }
    delete set;
}

// host checks of every leveled call once the set is known to be non-null: its samples, then the context
template <typename Set>
int ctx_lhe_validate_range(const Set *set, size_t first, size_t count, const char *text) {
    if (first > set->count || count > set->count - first) return thfhe_fail(THFHE_E_INVALID, text);
    return THFHE_OK;
}
template <typename Ctx, typename Set>
int ctx_lhe_validate_ctx(const Ctx *c, const Set *set, const char *text) {
    if (!c) return thfhe_fail(THFHE_E_INVALID, "null ctx");
    if (c != set->ctx) return thfhe_fail(THFHE_E_INVALID, text);
    return THFHE_OK;
}

// thfhe_lhe_cmux / thfhe_mk_lhe_cmux: out(s) = d0(s) + C_(s,bit) (.) (d1(s) - d0(s)) on host arrays of `count` TLWE samples, in slices of
// rules.cmux_slice.  launch(io, S): the engine's CMux launch of S samples, one pair each.
template <typename Ctx, typename Set, typename T, typename Launch>
int ctx_lhe_cmux(Ctx *c, const Set *set, int bit, const T *d1_a, const T *d1_b, const T *d0_a, const T *d0_b, T *out_a, T *out_b, size_t count,
                 const LheRules<Ctx> &rules, Launch launch) {
    if (!d1_a || !d1_b || !d0_a || !d0_b || !out_a || !out_b) return thfhe_fail(THFHE_E_INVALID, "null argument");
    if (bit < 0 || bit >= kLheMaxBits) return thfhe_fail(THFHE_E_INVALID, rules.bit_text);
    if (!set) return thfhe_fail(THFHE_E_INVALID, "null tgsw set");
    if (bit >= set->d) return thfhe_fail(THFHE_E_INVALID, rules.bit_text);
    THFHE_TRY(ctx_lhe_validate_range(set, 0, count, rules.range_text));
    THFHE_TRY(ctx_lhe_validate_ctx(c, set, rules.ctx_text));
    if (count == 0) return THFHE_OK;
    DevLock lk(*c);
    if (lk.rc) return lk.rc;
    const size_t N = rules.N, poly = N * sizeof(T);
    const size_t S_max = std::min(count, rules.cmux_slice), bytes = S_max * poly;
    for (DevBuf &b : c->d_lhe_in) THFHE_TRY(b.grow(bytes));
    THFHE_TRY(c->d_lhe_a.grow(bytes));
    THFHE_TRY(c->d_lhe_b.grow(bytes));
    const T *src[4] = {d0_a, d0_b, d1_a, d1_b};
    T *const in[4] = {c->d_lhe_in[0].template as<T>(), c->d_lhe_in[1].template as<T>(), c->d_lhe_in[2].template as<T>(), c->d_lhe_in[3].template as<T>()};
    T *const w_a = c->d_lhe_a.template as<T>(), *const w_b = c->d_lhe_b.template as<T>();
    for (size_t s0 = 0; s0 < count; s0 += S_max) {
        const size_t S = std::min(S_max, count - s0);
        for (int q = 0; q < 4; q++) THFHE_HIP(hipMemcpyAsync(in[q], src[q] + s0 * N, S * poly, hipMemcpyHostToDevice, c->stream));
        const LheCmuxIo<T> io{set->spec.template as<cplx>() + s0 * rules.sample_slots(c, set->d), in[0], in[1], in[2], in[3], w_a, w_b, nullptr, N, 0, N, 0, bit, false};
        THFHE_TRY(launch(io, S));
        THFHE_HIP(hipMemcpyAsync(out_a + s0 * N, w_a, S * poly, hipMemcpyDeviceToHost, c->stream));
        THFHE_HIP(hipMemcpyAsync(out_b + s0 * N, w_b, S * poly, hipMemcpyDeviceToHost, c->stream));
    }
    THFHE_HIP(hipStreamSynchronize(c->stream));
    return THFHE_OK;
}

// The launch chain of a leveled lookup over S samples, on device pointers only (the slices of ctx_lhe_lookup and the LOOKUP / GATHER groups of the
// gate DAG): the CMux tree, the rotations with the extraction of theta coefficients into d_u, and with ks_out the key switch of the
// S theta records into it (else they stay in d_u).  spec: the spectra at the first sample.  Sample s reads the 2^d_tree table polynomials at
// (t_a, t_b) + index(s) * tab_stride words, index(s) = idx[s] or s (t_a null: a public table).  The caller has sized d_lhe_a / d_lhe_b
// (S 2^(d_tree-1) polynomials each), d_u, what the engine's rotation needs besides, and ks_out.  prof: record the profiling events.
// cmux_level(io, pairs): the engine's CMux launch of S samples; rotate(src_a, src_b, src_idx, src_stride): its rotations of the S samples at
// (src_a, src_b) + index(s) * src_stride and the extraction into d_u; keyswitch(ks_out, records): its key switch of d_u.
template <typename Ctx, typename T, typename CmuxLevel, typename Rotate, typename Keyswitch>
int ctx_enqueue_lhe_lookup(Ctx *c, const cplx *spec, size_t S, int d_tree, int d_rot, int theta, const T *t_a, const T *t_b, const int32_t *idx, size_t tab_stride,
                           int32_t *ks_out, bool prof, const LheRules<Ctx> &rules, CmuxLevel cmux_level, Rotate rotate, Keyswitch keyswitch) {
    hipStream_t st = c->stream;
    const size_t N = rules.N, leaves = (size_t)1 << d_tree, ws = d_tree ? leaves / 2 : 0;   // ws: TLWE samples of tree workspace per sample
    T *const w_a = c->d_lhe_a.template as<T>(), *const w_b = c->d_lhe_b.template as<T>();
    if (prof) THFHE_HIP(hipEventRecord(c->ev[0], st));
    // the tree: level t pairs neighbours on bit d_rot + t; level 0 reads the table, the later levels run in place on the workspace -- the result
    // of pair p of level t lies at slot p 2^t of the sample, the slot of its own d0, which no other workgroup of the launch touches
    for (int t = 0; t < d_tree; t++) {
        LheCmuxIo<T> io{spec, nullptr, nullptr, nullptr, nullptr, w_a, w_b, nullptr, 0, 0, ws * N, 0, d_rot + t, t == 0 && !t_a};
        if (t == 0) {
            io.d0_a = t_a, io.d0_b = t_b, io.d1_a = t_a ? t_a + N : nullptr, io.d1_b = t_b + N;
            io.in_idx = idx, io.in_sample = tab_stride, io.in_pair = 2 * N, io.out_pair = N;
        } else {
            const size_t step = N << t;   // words between the d0 slots of neighbouring pairs
            io.d0_a = w_a, io.d0_b = w_b, io.d1_a = w_a + step / 2, io.d1_b = w_b + step / 2;
            io.in_sample = ws * N, io.in_pair = step, io.out_pair = step;
        }
        THFHE_TRY(cmux_level(io, leaves >> (t + 1)));
    }
    if (prof) THFHE_HIP(hipEventRecord(c->ev[1], st));
    THFHE_TRY(rotate(d_tree ? w_a : t_a, d_tree ? w_b : t_b, d_tree ? nullptr : idx, d_tree ? ws * N : tab_stride));
    if (prof) THFHE_HIP(hipEventRecord(c->ev[2], st));
    if (ks_out) THFHE_TRY(keyswitch(ks_out, S * theta));
    if (prof) {
        THFHE_HIP(hipEventRecord(c->ev[3], st));
        c->ev_valid = true;
    }
    return THFHE_OK;
}

// thfhe_lhe_lookup (keyswitch) / thfhe_lhe_lookup_wo_keyswitch and their thfhe_mk_ forms: out = count x theta records of rec_words() (resp. N + 1)
// words, in slices of at most tree_slice / 2^(d_tree-1) samples (the tree workspace: 2^(d_tree-1) TLWE samples per sample) and 65 535 samples.
// grow_extra(S_max): what the engine's rotation needs besides d_u; enqueue(spec, S, t_a, t_b, idx, tab_stride, ks_out, prof): its
// ctx_enqueue_lhe_lookup.
template <typename Ctx, typename Set, typename T, typename GrowExtra, typename Enqueue>
int ctx_lhe_lookup(Ctx *c, const Set *set, size_t first, size_t count, int d_tree, int d_rot, int theta, const T *tab_a, const T *tab_b, int n_tables,
                   const int32_t *table_index, int32_t *out, bool keyswitch, const LheRules<Ctx> &rules, GrowExtra grow_extra, Enqueue enqueue) {
    // host checks, before the context is looked at
    if (!tab_b || !out) return thfhe_fail(THFHE_E_INVALID, "null argument");
    if (d_tree < 0 || d_tree > kLheMaxTree) return thfhe_fail(THFHE_E_INVALID, rules.d_tree_text);
    if (d_rot < 0 || d_rot > rules.d_rot_max) return thfhe_fail(THFHE_E_INVALID, rules.d_rot_text);
    if (theta != 1 && theta != 2 && theta != 4) return thfhe_fail(THFHE_E_INVALID, rules.theta_text);
    if (theta > (rules.N >> d_rot)) return thfhe_fail(THFHE_E_INVALID, rules.box_text);
    if (n_tables < 1 || ((long)n_tables << d_tree) > kMaxEncLuts) return thfhe_fail(THFHE_E_INVALID, rules.n_tables_text);
    THFHE_TRY(tree_validate_index(table_index, n_tables, count));
    if (!set) return thfhe_fail(THFHE_E_INVALID, "null tgsw set");
    if (d_tree + d_rot != set->d) return thfhe_fail(THFHE_E_INVALID, rules.d_sum_text);
    THFHE_TRY(ctx_lhe_validate_range(set, first, count, rules.range_text));
    THFHE_TRY(ctx_lhe_validate_ctx(c, set, rules.ctx_text));
    if (count == 0) return THFHE_OK;
    DevLock lk(*c);
    if (lk.rc) return lk.rc;
    const size_t N = rules.N, poly = N * sizeof(T);
    const size_t leaves = (size_t)1 << d_tree, ws = d_tree ? leaves / 2 : 0;   // TLWE samples of tree workspace per sample
    const size_t S_max = std::min({count, (size_t)65535, std::max<size_t>(1, c->tree_slice / std::max<size_t>(ws, 1))});
    const size_t words = c->rec_words(), rec = keyswitch ? words : N + 1, tab_bytes = (size_t)n_tables * leaves * poly;
    int rc = c->d_tv.grow(tab_bytes);
    if (!rc && tab_a) rc = c->d_tva.grow(tab_bytes);
    if (!rc && ws) rc = c->d_lhe_a.grow(S_max * ws * poly);
    if (!rc && ws) rc = c->d_lhe_b.grow(S_max * ws * poly);
    if (!rc) rc = grow_extra(S_max);
    if (!rc) rc = c->d_u.grow(S_max * theta * (N + 1) * sizeof(int32_t));
    if (!rc && keyswitch) rc = c->stage.grow(S_max * theta * words);
    if (!rc && table_index) rc = c->d_lut_idx.grow(S_max * sizeof(int32_t));
    if (rc) return rc;
    hipStream_t st = c->stream;
    THFHE_HIP(hipMemcpyAsync(c->d_tv.template as<T>(), tab_b, tab_bytes, hipMemcpyHostToDevice, st));
    if (tab_a) THFHE_HIP(hipMemcpyAsync(c->d_tva.template as<T>(), tab_a, tab_bytes, hipMemcpyHostToDevice, st));
    const T *const t_a = tab_a ? c->d_tva.template as<T>() : nullptr, *const t_b = c->d_tv.template as<T>();
    int32_t *const d_idx = c->d_lut_idx.template as<int32_t>();
    const int32_t *const res = keyswitch ? c->stage.out_ptr() : c->d_u.template as<int32_t>();
    const size_t tab_stride = table_index ? leaves * N : 0;   // without an index every sample reads table 0
    for (size_t s0 = 0; s0 < count; s0 += S_max) {
        const size_t S = std::min(S_max, count - s0);
        const cplx *spec = set->spec.template as<cplx>() + (first + s0) * rules.sample_slots(c, set->d);
        if (table_index) THFHE_HIP(hipMemcpyAsync(d_idx, table_index + s0, S * sizeof(int32_t), hipMemcpyHostToDevice, st));
        THFHE_TRY(enqueue(spec, S, t_a, t_b, table_index ? d_idx : nullptr, tab_stride, keyswitch ? c->stage.out_ptr() : nullptr, c->profiling && s0 == 0));
        THFHE_HIP(hipMemcpyAsync(out + s0 * theta * rec, res, S * theta * rec * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    }
    THFHE_HIP(hipStreamSynchronize(st));
    return THFHE_OK;
}

}  // namespace

#endif  // THFHE_LHE_HOST_H
