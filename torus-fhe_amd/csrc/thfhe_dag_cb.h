// thfhe_dag_cb.h -- the circuit-bootstrap nodes of the gate-DAG executor (thfhe_dag_run_cb_batch; single key): a level's CB nodes turn
// wires of the run into the TGSW bits of computed sets, which the leveled groups of later levels read like the client's sets (thfhe_dag_lhe.h:
// sk_dag_sets).  Included by thfhe_sk.hip INSIDE its second anonymous namespace after thfhe_cb_host.h, whose slice body (cb_slice_enqueue) the group
// runs; sk_dag_run_luts calls the two functions below through forward declarations, between cb_level2_begin and cb_level2_end.
//
// All CB nodes of a level are ONE batch: the level-2 rotation's efficiency depends on the batch size (the pair kernel takes over above 256 jobs,
// DESIGN 4.21), so a level with several small sets does not run one chain per set.  The stages are deterministic per record, so no word depends on
// the batching.
#ifndef THFHE_DAG_CB_H
#define THFHE_DAG_CB_H

// Operand gather of one CB group over a slice of S instances from q0 (grid: bit i, instance q, node): bit record base[node] S + q d + i is wire
// pool[off + i] of instance q0 + q, node-major so that each node's rows come out contiguous; the workgroup of bit 0 also stores the record into the
// node's own wire.  tab: int32[cnt][4] = (base, off, d, out wire), base = the d of the nodes before it.
__global__ __launch_bounds__(256) void dag_cb_gather_kernel(int32_t *__restrict__ wires, const int32_t *__restrict__ tab, const int32_t *__restrict__ pool,
                                                            int32_t *__restrict__ dst, long q0, long S, size_t n_wires, int words) {
    const int i = blockIdx.x;
    const long q = blockIdx.y;
    const int32_t *const t = tab + 4 * (size_t)blockIdx.z;
    const int base = t[0], d = t[2];
    if (i >= d || q >= S) return;
    const size_t row = (size_t)(q0 + q) * n_wires;
    const int32_t *const src = wires + (row + (size_t)pool[t[1] + i]) * words;
    int32_t *const out = dst + ((size_t)base * S + (size_t)q * d + i) * words;
    int32_t *const own = i == 0 ? wires + (row + (size_t)t[3]) * words : nullptr;
    for (int k = threadIdx.x; k < words; k += 256) {
        const int32_t v = src[k];
        out[k] = v;
        if (own) own[k] = v;
    }
}

// instances per slice of a CB group of `bits` bits per instance: the flat call's slice of kCbSliceBits bits, at most thfhe_set_dag_slice instances
size_t dag_cb_slice(const thfhe_ctx *c, size_t bits, size_t instances) {
    return std::min({instances, c->dag_slice, std::max<size_t>(1, kCbSliceBits / bits)});
}

// Before any device work of the run: the computed sets' spectra still to be allocated and the workspace of the widest slice against the free
// device memory (cb_reserve: THFHE_E_NOMEM with nothing run), then every buffer the CB groups use, the spectra included, before dag_execute takes
// pointers; and the sets of the run in the order its rows name them.
int sk_dag_cb_reserve(thfhe_ctx *c, const DagPlan &plan, const DagFamilies &T, const DagCbRun &cbr, size_t instances) {
    const thfhe_dag_cb_families &B = *T.cb;
    const size_t per_bit = (size_t)2 * c->p.l * 2 * 1024 * sizeof(cplx);
    if (c->cb_sets.size() < (size_t)B.n_sets) c->cb_sets.resize((size_t)B.n_sets);
    size_t to_alloc = 0;
    for (int s = 0; s < B.n_sets; s++) {
        const size_t bytes = instances * B.sets[s].d * per_bit;
        if (!c->cb_sets[s] || c->cb_sets[s]->spec.bytes() < bytes) to_alloc += bytes;
    }
    // the most bits a slice of any CB group of the run holds: S is a quotient, so a narrower group can hold more bits than the widest
    size_t R_max = 0;
    for (const DagBatch &b : plan.batches)
        if (b.cls == kDagCb) R_max = std::max(R_max, dag_cb_slice(c, b.bits, instances) * b.bits);
    THFHE_TRY(cb_reserve(c, B.mode, R_max, cbr.N2, to_alloc));
    c->dag_sets.clear();
    for (int s = 0; s < T.n_client_sets(); s++) c->dag_sets.push_back(T.lhe->sets[s]);
    for (int s = 0; s < B.n_sets; s++) {
        if (!c->cb_sets[s]) c->cb_sets[s].reset(new (std::nothrow) thfhe_tgsw_set);
        thfhe_tgsw_set *const set = c->cb_sets[s].get();
        if (!set) return thfhe_fail(THFHE_E_NOMEM, "out of host memory");
        THFHE_TRY(set->spec.grow(instances * B.sets[s].d * per_bit));
        set->ctx = c, set->count = instances, set->d = B.sets[s].d;
        c->dag_sets.push_back(set);
    }
    return THFHE_OK;
}

// One CB group: per slice of S instances dag_cb_gather_kernel stages the S sum-d bit records node-major in d_cb_lwe (and writes every node's own
// wire), then the slice body of the flat call with one part per node: the node's contiguous rows into its set's spectra at sample q0 and, where
// asked, into the caller's words.
int sk_dag_cb_group(thfhe_ctx *c, const DagCbRun &cbr, const DagPlan &plan, const DagFamilies &T, const DagExtGroup &g, size_t instances) {
    const thfhe_dag_cb_families &B = *T.cb;
    hipStream_t st = c->stream;
    const int words = c->p.n + 1;
    const size_t cnt = (size_t)g.cnt, polys_per_bit = (size_t)2 * c->p.l * 2;
    const int32_t *const h_set = plan.tab.data() + g.off + 5 * cnt;   // cbset of every node, on the host
    const int32_t *const h_tab = plan.tab.data() + g.ext, *const d_tab = g.tab + g.ext, *const d_pool = g.tab + plan.cb_pool;   // the node table, here and there
    size_t bits = 0;
    int d_max = 0;
    for (size_t k = 0; k < cnt; k++) bits += (size_t)h_tab[4 * k + 2], d_max = std::max(d_max, (int)h_tab[4 * k + 2]);
    const size_t slice = dag_cb_slice(c, bits, instances);
    if (slice * bits * words * sizeof(int32_t) > c->d_cb_lwe.bytes()) return thfhe_fail(THFHE_E_INVALID, "CB group: its slice exceeds the reserved workspace");
    std::vector<CbSliceOut> outs(cnt);
    for (size_t q0 = 0; q0 < instances; q0 += slice) {
        const size_t S = std::min(slice, instances - q0);
        hipLaunchKernelGGL(dag_cb_gather_kernel, dim3((unsigned)d_max, (unsigned)S, (unsigned)cnt), dim3(256), 0, st, g.wires, d_tab, d_pool,
                           c->d_cb_lwe.as<int32_t>(), (long)q0, (long)S, g.n_wires, words);
        THFHE_HIP(hipGetLastError());
        for (size_t k = 0; k < cnt; k++) {
            const size_t d = (size_t)h_tab[4 * k + 2], at = q0 * d * polys_per_bit * 1024;
            int32_t *const w = B.words ? B.words[h_set[k]] : nullptr;
            outs[k] = CbSliceOut{(size_t)h_tab[4 * k] * S, S * d, c->cb_sets[h_set[k]]->spec.as<cplx>() + at, w ? w + at : nullptr};
        }
        THFHE_TRY(cb_slice_enqueue(c, cbr.l2, B.mode, S * bits, outs.data(), cnt, false));
    }
    return THFHE_OK;
}

#endif  // THFHE_DAG_CB_H
