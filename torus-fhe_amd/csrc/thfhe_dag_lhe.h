// thfhe_dag_lhe.h -- the leveled nodes of the gate-DAG executor (thfhe_dag_run_lhe_batch; single key): LHE_LOOKUP, LHE_GATHER and
// LHE_WFA groups on the client's TGSW sets and, in thfhe_dag_run_cb_batch, on the sets the run computed (looked up through sk_dag_sets).  Included by thfhe_sk.hip INSIDE its second anonymous namespace after thfhe_lhe.h, whose launch chains
// (enqueue_lhe_lookup, enqueue_lhe_wfa) the groups run on device pointers; sk_dag_run_luts calls the three functions below through forward declarations.
//
// The leveled kernels take the TGSW sample of a job from the job's number (spec + job d 2l 32 KiB), so a chain runs over consecutive instances of ONE
// node: a group of `cnt` nodes is cnt chains per slice of instances, each with count = the instances of the slice, its records scattered into the
// node's wires by dag_scatter_theta_kernel (one node per launch: cnt = 1, the index column advanced to the node).
#ifndef THFHE_DAG_LHE_H
#define THFHE_DAG_LHE_H

// d of set i of the run: a computed set's from its spec (thfhe_dag_run_cb_batch; an index past the client's sets), a client set's own
int sk_dag_set_d(const DagFamilies &T, int i) { return T.computed_d(i) >= 0 ? T.computed_d(i) : T.lhe->sets[i]->d; }
// the sets of the run from set i on: the client's array, or, in a run with computed sets, the context's list of both kinds (sk_dag_cb_reserve)
const thfhe_tgsw_set *const *sk_dag_sets(const thfhe_ctx *c, const DagFamilies &T, int i) { return (T.cb ? c->dag_sets.data() : T.lhe->sets) + i; }

// instances per chain of a group: the flat entries' thfhe_set_tree_slice rules, at most thfhe_set_dag_slice, one grid.y
size_t dag_lhe_slice(const thfhe_ctx *c, const thfhe_dag_lhe_families &F, const DagBatch &b, size_t instances) {
    const size_t cap = std::min({instances, c->dag_slice, (size_t)65535});
    if (b.cls == kDagLheWfa) {
        const thfhe_dag_wfa_spec &a = F.wfas[b.tree];
        const size_t recs = (size_t)a.n_out * a.theta;
        return std::min({cap, std::max<size_t>(1, c->tree_slice / (2 * (size_t)a.n_states)), std::max<size_t>(1, c->tree_slice / recs)});
    }
    const thfhe_dag_lhe_spec &k = F.lks[b.tree];
    if (b.cls == kDagLheGather) return std::min(cap, std::max<size_t>(1, c->tree_slice >> (k.d_tree + k.d_rot)));
    return std::min(cap, std::max<size_t>(1, c->tree_slice / std::max<size_t>(k.d_tree ? ((size_t)1 << k.d_tree) / 2 : 0, 1)));
}

// The checks of thfhe_dag_run_lhe_batch that look at the sets, after the plan's, in the order of the header: null sets, (the null context,) a set of
// another context, a set count below `instances`, d_tree + d_rot against the set's d, step_bit against the spec's sets.
int sk_dag_lhe_check_sets(const thfhe_ctx *c, const DagPlan &plan, const DagFamilies &T, size_t instances) {
    const thfhe_dag_lhe_families &F = *T.lhe;
    if (T.cb)   // a computed set's d is known on the host: the step bits that name one, before any set or context is looked at
        for (const DagBatch &b : plan.batches) {
            if (b.cls != kDagLheWfa) continue;
            const thfhe_dag_wfa_spec &a = F.wfas[b.tree];
            for (int j = 0; j < a.n_steps; j++) {
                const int32_t sb = F.wfa_words[a.step_off + j];
                if (sb >= 0 && (sb >> 4) < a.n_sets && T.computed_d(a.set0 + (sb >> 4)) >= 0 && (sb & 15) >= T.computed_d(a.set0 + (sb >> 4)))
                    return thfhe_fail(THFHE_E_INVALID, "LHE_WFA node: step_bit must name bit 0 .. d-1 of set 0 .. n_sets-1 of the spec (16 set + bit)");
            }
        }
    for (int i = 0; i < F.n_sets; i++)
        if (!F.sets[i]) return thfhe_fail(THFHE_E_INVALID, "null tgsw set");
    if (!c) return thfhe_fail(THFHE_E_INVALID, "null ctx");
    for (int i = 0; i < F.n_sets; i++)
        if (F.sets[i]->ctx != c) return thfhe_fail(THFHE_E_INVALID, "lhe: the set belongs to another context");
    for (int i = 0; i < F.n_sets; i++)
        if (F.sets[i]->count < instances) return thfhe_fail(THFHE_E_INVALID, "lhe: a set holds fewer samples than the run has instances");
    for (const DagBatch &b : plan.batches) {
        if (!dag_class_leveled(b.cls)) continue;
        if (b.cls == kDagLheWfa) {
            const thfhe_dag_wfa_spec &a = F.wfas[b.tree];
            const int32_t *const step_bit = F.wfa_words + a.step_off;
            for (int j = 0; j < a.n_steps; j++)
                if (step_bit[j] < 0 || (step_bit[j] >> 4) >= a.n_sets || (step_bit[j] & 15) >= sk_dag_set_d(T, a.set0 + (step_bit[j] >> 4)))
                    return thfhe_fail(THFHE_E_INVALID, "LHE_WFA node: step_bit must name bit 0 .. d-1 of set 0 .. n_sets-1 of the spec (16 set + bit)");
        } else {
            const thfhe_dag_lhe_spec &k = F.lks[b.tree];
            if (k.d_tree + k.d_rot != sk_dag_set_d(T, k.set)) return thfhe_fail(THFHE_E_INVALID, "leveled node: d_tree + d_rot must equal the set's d");
        }
    }
    return THFHE_OK;
}

// Every buffer the leveled groups of the plan use, the staging output included, before dag_execute takes pointers; w_cand: the most candidates one
// box packing of the run takes.  Then the run's table polynomials, final weights and word pool, once per call.
int sk_dag_lhe_reserve(thfhe_ctx *c, const DagPlan &plan, const DagFamilies &T, size_t instances, size_t &w_cand) {
    const thfhe_dag_lhe_families &F = *T.lhe;
    const size_t words = c->p.n + 1;
    bool any = false;
    for (const DagBatch &b : plan.batches) {
        if (!dag_class_leveled(b.cls)) continue;
        any = true;
        const size_t S = dag_lhe_slice(c, F, b, instances);
        size_t recs, ws;   // records and TLWE samples of workspace (per buffer) per instance
        if (b.cls == kDagLheWfa) {
            const thfhe_dag_wfa_spec &a = F.wfas[b.tree];
            recs = (size_t)a.n_out * a.theta, ws = (size_t)a.n_states * 2;   // a layer: n_states x (mask | body)
        } else {
            const thfhe_dag_lhe_spec &k = F.lks[b.tree];
            const size_t leaves = (size_t)1 << k.d_tree;
            recs = (size_t)k.theta, ws = k.d_tree ? leaves / 2 : 0;
            if (b.cls == kDagLheGather) {
                const size_t P = (size_t)1 << (k.d_tree + k.d_rot);
                THFHE_TRY(c->d_tree_lwe.grow(S * P * words * sizeof(int32_t)));
                THFHE_TRY(c->d_tree_a.grow(S * leaves * 4096));
                THFHE_TRY(c->d_tree_b.grow(S * leaves * 4096));
                w_cand = std::max(w_cand, S * P);
            }
        }
        if (ws) THFHE_TRY(c->d_lhe_a.grow(S * ws * 4096));
        if (ws) THFHE_TRY(c->d_lhe_b.grow(S * ws * 4096));
        THFHE_TRY(c->d_u.grow(S * recs * 1025 * sizeof(int32_t)));
        THFHE_TRY(c->stage.out.grow(S * recs * words * sizeof(int32_t)));
    }
    if (!any) return THFHE_OK;
    auto upload = [&](DevBuf &d, const void *h, size_t bytes) -> int {
        if (!h) return THFHE_OK;   // a family the run does not have (its count is 0: dag_families_check), or public tables / weights (no masks)
        THFHE_TRY(d.grow(bytes));
        THFHE_HIP(hipMemcpyAsync(d.as<void>(), h, bytes, hipMemcpyHostToDevice, c->stream));
        return THFHE_OK;
    };
    THFHE_TRY(upload(c->d_dag_lhe_tab_a, F.tab_a, (size_t)F.n_tab_rows * 4096));
    THFHE_TRY(upload(c->d_dag_lhe_tab_b, F.tab_b, (size_t)F.n_tab_rows * 4096));
    THFHE_TRY(upload(c->d_dag_lhe_fin_a, F.fin_a, (size_t)F.n_fin_rows * 4096));
    THFHE_TRY(upload(c->d_dag_lhe_fin_b, F.fin_b, (size_t)F.n_fin_rows * 4096));
    return upload(c->d_dag_lhe_words, F.wfa_words, F.n_wfa_words * sizeof(int32_t));
}

// One leveled group of a level: per slice of instances and per node of the group the flat entry's launch chain, then the scatter of its records.
//   LOOKUP  the chain of thfhe_lhe_lookup on the run's table polynomials from row0 (every instance reads the same rows: stride 0).
//   GATHER  dag_lhe_gather_kernel stages the slice's 2^d candidates per instance from the wire table, the packing context packs them into 2^d_tree
//           TLWE samples per instance (boxes of N / 2^d_rot coefficients), and the lookup chain reads instance j's own samples (stride 2^d_tree).
//   WFA     the chain of thfhe_lhe_wfa on the spec's slices of the word pool and the final weights from fin_row0.
int sk_dag_lhe_group(thfhe_ctx *c, thfhe_poly_ctx *pc, const DagPlan &plan, const DagFamilies &T, const DagExtGroup &g, size_t instances) {
    const thfhe_dag_lhe_families &F = *T.lhe;
    hipStream_t st = c->stream;
    const int words = c->p.n + 1;
    const unsigned wb = (unsigned)((words + 255) / 256);
    const size_t cnt = (size_t)g.cnt;
    const int32_t *const h_y = plan.tab.data() + g.off + 6 * cnt;   // row0 / first / fin_row0 of every node, on the host
    DagBatch b{};
    b.cls = g.cls, b.tree = g.tree;
    const size_t slice = dag_lhe_slice(c, F, b, instances);
    int cus = 0;
    if (g.cls == kDagLheWfa) THFHE_TRY(ctx_cus(c, &cus));
    int32_t *const ks_out = c->stage.out_ptr();
    for (size_t q0 = 0; q0 < instances; q0 += slice) {
        const size_t S = std::min(slice, instances - q0);
        for (size_t node = 0; node < cnt; node++) {
            int recs;
            if (g.cls == kDagLheWfa) {
                const thfhe_dag_wfa_spec &a = F.wfas[g.tree];
                const int32_t *const d_words = c->d_dag_lhe_words.as<int32_t>();
                const size_t fin = (size_t)h_y[node] * 1024;
                recs = a.n_out * a.theta;
                THFHE_TRY(enqueue_lhe_wfa(c, sk_dag_sets(c, T, a.set0), q0, S, a.n_steps, a.n_states, F.wfa_words + a.step_off, d_words + a.trans_off, d_words + a.start_off,
                                          F.fin_a ? c->d_dag_lhe_fin_a.as<int32_t>() + fin : nullptr, c->d_dag_lhe_fin_b.as<int32_t>() + fin, nullptr, 0, a.theta,
                                          a.n_out, cus, ks_out, false));
            } else {
                const thfhe_dag_lhe_spec &k = F.lks[g.tree];
                const thfhe_tgsw_set *const set = *sk_dag_sets(c, T, k.set);
                const cplx *const spec = set->spec.as<cplx>() + q0 * lhe_sample_slots(c, set->d);
                recs = k.theta;
                if (g.cls == kDagLheGather) {
                    const int P = 1 << (k.d_tree + k.d_rot);
                    const size_t leaves = (size_t)1 << k.d_tree;
                    const unsigned gx = (unsigned)std::min<size_t>(((size_t)P * words + 255) / 256, 64);
                    hipLaunchKernelGGL(dag_lhe_gather_kernel, dim3(gx, (unsigned)S), dim3(256), 0, st, (const int32_t *)g.wires, c->d_tree_lwe.as<int32_t>(), (long)q0,
                                       (long)S, g.n_wires, words, (int)h_y[node], P);
                    THFHE_HIP(hipGetLastError());
                    THFHE_TRY(pack_boxes_enqueue(pc, c->d_tree_lwe.as<int32_t>(), S * P, 1 << k.d_rot, c->d_tree_a.as<int32_t>(), c->d_tree_b.as<int32_t>(), st));
                    THFHE_TRY(enqueue_lhe_lookup(c, spec, set->d, S, k.d_tree, k.d_rot, 1, c->d_tree_a.as<int32_t>(), c->d_tree_b.as<int32_t>(), nullptr, leaves * 1024,
                                                 ks_out, false));
                } else {
                    const size_t row = (size_t)h_y[node] * 1024;
                    THFHE_TRY(enqueue_lhe_lookup(c, spec, set->d, S, k.d_tree, k.d_rot, k.theta, F.tab_a ? c->d_dag_lhe_tab_a.as<int32_t>() + row : nullptr,
                                                 c->d_dag_lhe_tab_b.as<int32_t>() + row, nullptr, 0, ks_out, false));
                }
            }
            // record j recs + t of the chain -> wire out[node] + t of instance q0 + j
            hipLaunchKernelGGL(dag_scatter_theta_kernel, dim3((unsigned)(S * recs), wb), dim3(256), 0, st, (const int32_t *)ks_out, g.t_out + node, g.wires, (long)q0,
                               (long)S, 1L, g.n_wires, words, recs);
            THFHE_HIP(hipGetLastError());
        }
    }
    return THFHE_OK;
}

#endif  // THFHE_DAG_LHE_H
