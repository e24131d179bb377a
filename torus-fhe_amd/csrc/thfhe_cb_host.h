// thfhe_cb_host.h -- circuit bootstrapping on the single-key context: the bodies of thfhe_cb_key_set,
// thfhe_cb_private_keyswitch, thfhe_cb_stage_a and thfhe_circuit_bootstrap(_mode).  Included by thfhe_sk.hip INSIDE its second anonymous
// namespace, after thfhe_lhe.h (it fills a thfhe_tgsw_set); the key, the kernels and their launcher are in thfhe_cb.h.

int cb_check_shape(int D, int t, int basebit) {
    if (D < 1 || D > kCbMaxD) return thfhe_fail(THFHE_E_INVALID, "circuit-bootstrap key: D must be 1 .. 2048");
    if (t < 1 || basebit < 1 || basebit > 8 || t * basebit > 32)
        return thfhe_fail(THFHE_E_INVALID, "circuit-bootstrap key: need t >= 1, 1 <= basebit <= 8 (a digit is a signed byte) and t basebit <= 32");
    return THFHE_OK;
}

int cb_key_set(thfhe_ctx *c, const int32_t *pks, int D, int t, int basebit) {
    if (!pks) return thfhe_fail(THFHE_E_INVALID, "null argument");
    THFHE_TRY(cb_check_shape(D, t, basebit));
    if (!c) return thfhe_fail(THFHE_E_INVALID, "null ctx");
    DevLock lk(*c);
    if (lk.rc) return lk.rc;
    return c->cb.upload(pks, D, t, basebit, c->stream);
}

// stage B alone on host buffers, in slices of at most 2048 inputs
int cb_private_keyswitch(thfhe_ctx *c, const int32_t *lwe2, size_t count, int32_t *tgsw) {
    if (!lwe2 || !tgsw) return thfhe_fail(THFHE_E_INVALID, "null argument");
    if (count > ((size_t)1 << 24)) return thfhe_fail(THFHE_E_INVALID, "private key switch: count must be at most 2^24");
    if (!c) return thfhe_fail(THFHE_E_INVALID, "null ctx");
    DevLock lk(*c);
    if (lk.rc) return lk.rc;
    if (!c->cb.D) return thfhe_fail(THFHE_E_INVALID, "no circuit-bootstrap key (thfhe_cb_key_set)");
    if (count == 0) return THFHE_OK;
    const int l = c->p.l, D = c->cb.D;
    const size_t S_max = std::min<size_t>(count, std::max(1, 2048 / l));
    const size_t in_words = (size_t)l * (D + 1), out_words = (size_t)2 * l * kCbRow;
    THFHE_TRY(c->d_cb_lwe2.grow(S_max * in_words * sizeof(int32_t)));
    THFHE_TRY(c->d_cb_rows.grow(S_max * out_words * sizeof(int32_t)));
    for (size_t s0 = 0; s0 < count; s0 += S_max) {
        const size_t S = std::min(S_max, count - s0);
        THFHE_HIP(hipMemcpyAsync(c->d_cb_lwe2.as<int32_t>(), lwe2 + s0 * in_words, S * in_words * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
        THFHE_TRY(cb_enqueue(c->cb, c->d_cb_lwe2.as<int32_t>(), (long)(S * l), l, c->d_cb_rows.as<int32_t>(), c->stream));
        THFHE_HIP(hipMemcpyAsync(tgsw + s0 * out_words, c->d_cb_rows.as<int32_t>(), S * out_words * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    }
    THFHE_HIP(hipStreamSynchronize(c->stream));
    return THFHE_OK;
}

constexpr size_t kCbSliceBits = 2048;   // bits per slice of thfhe_circuit_bootstrap: 64 MiB of level-2 accumulators, 2l x 16 MiB of rows

int cb_check_mode(int mode) {
    if (mode != THFHE_CB_PER_LEVEL && mode != THFHE_CB_ONE_ROTATION)
        return thfhe_fail(THFHE_E_INVALID, "circuit bootstrap: mode must be THFHE_CB_PER_LEVEL or THFHE_CB_ONE_ROTATION");
    return THFHE_OK;
}

// theta of the one-rotation mode: the smallest power of two >= l (l <= 4: the engines' theta stops there)
int cb_theta(int l) { return l <= 1 ? 1 : (l == 2 ? 2 : 4); }

// the checks of the two contexts that stage A makes, under c's lock: p2 / dev2 are thfhe_mk_ctx_info's answer about the level-2 context
int cb_check_pair(const thfhe_ctx *c, const thfhe_params &p2, int dev2, int mode) {
    if (!c->cb.D) return thfhe_fail(THFHE_E_INVALID, "no circuit-bootstrap key (thfhe_cb_key_set)");
    if (dev2 != c->device) return thfhe_fail(THFHE_E_INVALID, "circuit bootstrap: the two contexts are on different devices");
    if (p2.parties != 1 || p2.n != c->p.n || p2.N != c->cb.D)
        return thfhe_fail(THFHE_E_INVALID, "circuit bootstrap: the level-2 context needs parties = 1, the gate context's n and the key's D as its ring degree");
    if ((c->p.l) * c->p.Bgbit > 32) return thfhe_fail(THFHE_E_UNSUPPORTED, "circuit bootstrap: l Bgbit must be at most 32");
    if (mode == THFHE_CB_ONE_ROTATION && c->p.l > 4)
        return thfhe_fail(THFHE_E_UNSUPPORTED, "circuit bootstrap, one rotation per bit: l must be at most 4 (theta is 1, 2 or 4)");
    return THFHE_OK;
}

// The buffers of stage A for slices of R_max bits, and in one-rotation mode the call's test vector tv[q] = mu_(q mod theta) for q mod theta < l, else 0
// (built here, once per call, into the context's grow-only d_cb_tv).  One-rotation mode needs neither the mod-switched words (the level-2 context
// keeps them in its own workspace) nor the one-level hop d_cb_x.
int cb_stage_a_prepare(thfhe_ctx *c, int mode, size_t R_max, int N2) {
    const int l = c->p.l, n = c->p.n, D = c->cb.D;
    THFHE_TRY(c->d_cb_lwe.grow(R_max * (n + 1) * 4));
    THFHE_TRY(c->d_cb_acc.grow(R_max * 2 * N2 * sizeof(int64_t)));
    THFHE_TRY(c->d_cb_lwe2.grow(R_max * l * (D + 1) * 4));
    if (mode == THFHE_CB_PER_LEVEL) {
        THFHE_TRY(c->d_cb_bara.grow(R_max * n * 4));
        THFHE_TRY(c->d_cb_barb.grow(R_max * 4));
        THFHE_TRY(c->d_cb_x.grow(R_max * (D + 1) * 4));
        return THFHE_OK;
    }
    THFHE_TRY(c->d_cb_tv.grow((size_t)N2 * sizeof(int64_t)));
    std::vector<int64_t> tv((size_t)N2, 0);
    const int theta = cb_theta(l);
    for (int q = 0; q < N2; q++)
        if (q % theta < l) tv[q] = (int64_t)1 << (63 - (q % theta + 1) * c->p.Bgbit);
    THFHE_HIP(hipMemcpyAsync(c->d_cb_tv.as<int64_t>(), tv.data(), tv.size() * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
    THFHE_HIP(hipStreamSynchronize(c->stream));   // tv goes out of scope
    return THFHE_OK;
}

// Stage A of R bits on c's stream, which the level-2 context has been lent: d_cb_lwe [R][n + 1] -> d_cb_lwe2 [R][l][D + 1].
//   per level:     one prologue, l rotations with mu_j = 2^(63 - (j+1) Bgbit), extraction of coefficient 0, + 2^(31 - (j+1) Bgbit) on the body
//   one rotation:  the theta-rounded prologue, the start from d_cb_tv and ONE rotation (thfhe_mk_lut_rotate_dev), then cb_extract_levels_kernel:
//                  coefficients 0 .. l-1 with the same body offsets
int cb_stage_a_enqueue(thfhe_ctx *c, thfhe_mk_ctx *l2, int mode, size_t R) {
    const int l = c->p.l, n = c->p.n, D = c->cb.D;
    hipStream_t st = c->stream;
    if (mode == THFHE_CB_ONE_ROTATION) {
        if (D < 512 || (D & (D - 1))) return thfhe_fail(THFHE_E_UNSUPPORTED, "circuit bootstrap, one rotation per bit: D must be a power of two >= 512");
        THFHE_TRY(thfhe_mk_lut_rotate_dev(l2, c->d_cb_lwe.as<int32_t>(), cb_theta(l), c->d_cb_tv.as<int64_t>(), c->d_cb_acc.as<int64_t>(), R));
        hipLaunchKernelGGL(cb_extract_levels_kernel, dim3((unsigned)R), dim3(256), 0, st, c->d_cb_acc.as<int64_t>(), D, l, c->p.Bgbit, c->d_cb_lwe2.as<int32_t>());
        THFHE_HIP(hipGetLastError());
        return THFHE_OK;
    }
    THFHE_TRY(thfhe_mk_prologue_dev(l2, -1, 0, c->d_cb_lwe.as<int32_t>(), nullptr, nullptr, n + 1, 0, c->d_cb_bara.as<int32_t>(), c->d_cb_barb.as<int32_t>(), R));
    for (int j = 0; j < l; j++) {
        const int64_t mu = (int64_t)1 << (63 - (j + 1) * c->p.Bgbit);
        THFHE_TRY(thfhe_mk_rotate_partial_dev(l2, c->d_cb_bara.as<int32_t>(), c->d_cb_barb.as<int32_t>(), mu, nullptr, c->d_cb_acc.as<int64_t>(), R));
        THFHE_TRY(thfhe_mk_extract_dev(l2, c->d_cb_acc.as<int64_t>(), c->d_cb_x.as<int32_t>(), R));
        hipLaunchKernelGGL(cb_place_kernel, dim3((unsigned)((D + 1 + 255) / 256), (unsigned)R), dim3(256), 0, st, c->d_cb_x.as<int32_t>(), D, l, j,
                           1u << (31 - (j + 1) * c->p.Bgbit), c->d_cb_lwe2.as<int32_t>());
        THFHE_HIP(hipGetLastError());
    }
    return THFHE_OK;
}

// thfhe_cb_stage_a after its host checks: slices of kCbSliceBits records up, stage A, the l records per bit down
int cb_stage_a_fill(thfhe_ctx *c, thfhe_mk_ctx *l2, int N2, int mode, const int32_t *lwe, size_t count, int32_t *lwe2) {
    const int l = c->p.l, n = c->p.n, D = c->cb.D;
    const size_t R_max = std::min(count, kCbSliceBits), out_words = (size_t)l * (D + 1);
    THFHE_TRY(cb_stage_a_prepare(c, mode, R_max, N2));
    hipStream_t st = c->stream;
    for (size_t b0 = 0; b0 < count; b0 += R_max) {
        const size_t R = std::min(R_max, count - b0);
        THFHE_HIP(hipMemcpyAsync(c->d_cb_lwe.as<int32_t>(), lwe + b0 * (n + 1), R * (n + 1) * 4, hipMemcpyHostToDevice, st));
        THFHE_TRY(cb_stage_a_enqueue(c, l2, mode, R));
        THFHE_HIP(hipMemcpyAsync(lwe2 + b0 * out_words, c->d_cb_lwe2.as<int32_t>(), R * out_words * 4, hipMemcpyDeviceToHost, st));
    }
    THFHE_HIP(hipStreamSynchronize(st));
    return THFHE_OK;
}

// Before any device work of a call: the spectra it has to allocate (spec_bytes) and the workspace of slices of R_max bits against the free device
// memory, THFHE_E_NOMEM with nothing run; then the buffers of the three stages.
int cb_reserve(thfhe_ctx *c, int mode, size_t R_max, int N2, size_t spec_bytes) {
    const int l = c->p.l, n = c->p.n, D = c->cb.D;
    const size_t polys_per_bit = (size_t)2 * l * 2;
    // one-rotation mode has no one-level hop: b_x drops out (its mod-switched words, b_bara and b_barb, are in the level-2 context's workspace)
    const size_t b_lwe = R_max * (n + 1) * 4, b_bara = R_max * n * 4, b_barb = R_max * 4, b_acc = R_max * 2 * N2 * sizeof(int64_t),
                 b_x = mode == THFHE_CB_PER_LEVEL ? R_max * (D + 1) * 4 : 0, b_lwe2 = R_max * (D + 1) * 4 * l, b_rows = R_max * polys_per_bit * 4096,
                 b_dig = std::min<size_t>(R_max * l, kCbMaxLaunchInputs) * c->cb.nstages * kCbStage;
    size_t free_b = 0, total_b = 0;
    THFHE_HIP(hipMemGetInfo(&free_b, &total_b));
    if (spec_bytes + b_lwe + b_bara + b_barb + b_acc + b_x + b_lwe2 + b_rows + b_dig > free_b)
        return thfhe_fail(THFHE_E_NOMEM, "circuit bootstrap: count d 2l 32 KiB of spectra and the slice workspace exceed the free device memory");
    THFHE_TRY(cb_stage_a_prepare(c, mode, R_max, N2));
    return c->d_cb_rows.grow(b_rows);
}

// One part of a slice's TGSW rows on its way out: the rows of bits [bit0, bit0 + bits) of the slice go to `words` on the host, if wanted, and as
// spectra to `spec`.
struct CbSliceOut {
    size_t bit0, bits;
    cplx *spec;
    int32_t *words;
};
// The device part of one slice of R bits whose gate records are in d_cb_lwe: stage A (cb_stage_a_enqueue), stage B (the private key switch) and
// stage C (the key transform of every part of `outs` into its spectra), all on c's stream.  prof: the stages' events around them.  cb_fill has one
// part per slice; a CB group of the gate DAG (thfhe_dag_cb.h) one per node.
int cb_slice_enqueue(thfhe_ctx *c, thfhe_mk_ctx *l2, int mode, size_t R, const CbSliceOut *outs, size_t n_outs, bool prof) {
    const int l = c->p.l;
    const size_t polys_per_bit = (size_t)2 * l * 2;
    hipStream_t st = c->stream;
    if (prof) THFHE_HIP(hipEventRecord(c->ev[0], st));
    THFHE_TRY(cb_stage_a_enqueue(c, l2, mode, R));
    if (prof) THFHE_HIP(hipEventRecord(c->ev[1], st));
    THFHE_TRY(cb_enqueue(c->cb, c->d_cb_lwe2.as<int32_t>(), (long)(R * l), l, c->d_cb_rows.as<int32_t>(), st));
    if (prof) THFHE_HIP(hipEventRecord(c->ev[2], st));
    for (size_t k = 0; k < n_outs; k++) {
        const CbSliceOut &o = outs[k];
        const int32_t *const rows = c->d_cb_rows.as<int32_t>() + o.bit0 * polys_per_bit * 1024;
        if (o.words) THFHE_HIP(hipMemcpyAsync(o.words, rows, o.bits * polys_per_bit * 4096, hipMemcpyDeviceToHost, st));
        THFHE_TRY((launch_torus_transform<1024, 32>(st, rows, (long)(o.bits * polys_per_bit), c->d_tw.as<cplx>(), o.spec)));
    }
    if (prof) {
        THFHE_HIP(hipEventRecord(c->ev[3], st));
        c->ev_valid = true;
    }
    return THFHE_OK;
}

// thfhe_circuit_bootstrap_mode after its host checks, the level-2 context enqueueing on c's stream: per slice of bits stage A (cb_stage_a_enqueue),
// stage B (the private key switch) and stage C (the key transform into the set's spectra).  Nothing leaves the device between the stages;
// `words`, if wanted, gets the rows of stage B.
int cb_fill(thfhe_ctx *c, thfhe_mk_ctx *l2, int N2, thfhe_tgsw_set *set, const int32_t *lwe, int32_t *words, int mode) {
    const int l = c->p.l, n = c->p.n;
    const size_t polys_per_bit = (size_t)2 * l * 2, bits = set->count * set->d, R_max = std::min(bits, kCbSliceBits);
    const size_t spec_bytes = bits * polys_per_bit * 1024 * sizeof(cplx);
    THFHE_TRY(cb_reserve(c, mode, R_max, N2, spec_bytes));
    THFHE_TRY(set->spec.grow(spec_bytes));
    hipStream_t st = c->stream;
    const bool prof = c->profiling;
    for (size_t b0 = 0; b0 < bits; b0 += R_max) {
        const size_t R = std::min(R_max, bits - b0);
        const bool last = b0 + R == bits;
        THFHE_HIP(hipMemcpyAsync(c->d_cb_lwe.as<int32_t>(), lwe + b0 * (n + 1), R * (n + 1) * 4, hipMemcpyHostToDevice, st));
        const CbSliceOut out{0, R, set->spec.as<cplx>() + b0 * polys_per_bit * 1024, words ? words + b0 * polys_per_bit * 1024 : nullptr};
        THFHE_TRY(cb_slice_enqueue(c, l2, mode, R, &out, 1, prof && last));
    }
    THFHE_HIP(hipStreamSynchronize(st));
    return THFHE_OK;
}

// Under c's lock: the checks of the two contexts, then c's stream lent to the level-2 context (one stream for all stages); *N2: its ring degree.
// cb_level2_end hands the stream back, and is due whatever ran in between.
int cb_level2_begin(thfhe_ctx *c, thfhe_mk_ctx *l2, int mode, int *N2) {
    thfhe_params p2;
    int dev2 = -1;
    THFHE_TRY(thfhe_mk_ctx_info(l2, &p2, &dev2));
    THFHE_TRY(cb_check_pair(c, p2, dev2, mode));
    *N2 = p2.N;
    return thfhe_mk_set_stream(l2, c->stream);
}
int cb_level2_end(thfhe_mk_ctx *l2) { return thfhe_mk_set_stream(l2, nullptr); }   // drains the stream first

// `run` under c's lock between the two, the stream handed back whatever `run` returns
template <typename Run>
int cb_with_level2(thfhe_ctx *c, thfhe_mk_ctx *l2, int mode, Run &&run) {
    DevLock lk(*c);
    if (lk.rc) return lk.rc;
    int N2 = 0;
    THFHE_TRY(cb_level2_begin(c, l2, mode, &N2));
    int rc = run(N2);
    const int rc2 = cb_level2_end(l2);
    return rc ? rc : rc2;
}

// stage A alone on host buffers: the counterpart of cb_private_keyswitch
int cb_stage_a(thfhe_ctx *c, thfhe_mk_ctx *l2, const int32_t *lwe, size_t count, int mode, int32_t *lwe2) {
    if (!lwe || !lwe2) return thfhe_fail(THFHE_E_INVALID, "null argument");
    THFHE_TRY(cb_check_mode(mode));
    if (count > ((size_t)1 << 24)) return thfhe_fail(THFHE_E_INVALID, "circuit bootstrap, stage A: count must be at most 2^24");
    if (!c || !l2) return thfhe_fail(THFHE_E_INVALID, "null ctx");
    return cb_with_level2(c, l2, mode, [&](int N2) { return count ? cb_stage_a_fill(c, l2, N2, mode, lwe, count, lwe2) : THFHE_OK; });
}

int circuit_bootstrap(thfhe_ctx *c, thfhe_mk_ctx *l2, const int32_t *lwe, size_t count, int d, int mode, int32_t *words, thfhe_tgsw_set **out) {
    if (!lwe || !out) return thfhe_fail(THFHE_E_INVALID, "null argument");
    *out = nullptr;
    THFHE_TRY(cb_check_mode(mode));
    if (d < 1 || d > kLheMaxBits) return thfhe_fail(THFHE_E_INVALID, "circuit bootstrap: d must be 1 .. 16");
    if (count < 1 || count > ((size_t)1 << 24)) return thfhe_fail(THFHE_E_INVALID, "circuit bootstrap: count must be 1 .. 2^24");
    if (!c || !l2) return thfhe_fail(THFHE_E_INVALID, "null ctx");
    std::unique_ptr<thfhe_tgsw_set> set(new (std::nothrow) thfhe_tgsw_set);
    if (!set) return thfhe_fail(THFHE_E_NOMEM, "out of host memory");
    set->ctx = c, set->count = count, set->d = d;
    const int rc = cb_with_level2(c, l2, mode, [&](int N2) { return cb_fill(c, l2, N2, set.get(), lwe, words, mode); });
    if (rc) {   // nothing is left behind: the spectra are freed on the context's device
        (void)hipSetDevice(c->device);
        return rc;
    }
    *out = set.release();
    return THFHE_OK;
}
