// thfhe_polymac.hip -- exact multiply-accumulate of small-coefficient polynomials with torus polynomials on gfx950:
//     out[j] = addend[j] + sum over the terms (j, s, t, sign) of  sign * small[s] (*) torus[t]      mod X^N + 1, mod 2^32 / 2^64
// This is the arithmetic of multi-key KEY GENERATION -- tgsw_encrypt_3gen (J/tgsw_3gen.jl:41-95: r1 (*) B, r2 (*) B, r2 (*) A, r1 (*) A),
// PublicKey / CommonPubKey_3gen (J/mk_internals.jl:266-345: z (*) a), the CCS mk_tgsw_encrypt (J/mk_internals.jl:390-446:
// r (*) a_i, s (*) f1_i) -- with the randomness handed in as arrays, so that the GPU result equals the host (numpy) key generation
// bit for bit (thfhe/keygen.py, tests/test_gpu_keygen.py).
// Method: the engine's split-limb FP64 transform (thfhe_lane.h).  Every torus polynomial is split into balanced 16-bit limbs and
// transformed once (torus_transform_kernel); one wave per output transforms each small operand once, multiplies it into the
// limb spectra of its partner and inverse-transforms every limb product separately: |product| <= N 2^(sb-1) 2^15 with |small| < 2^(sb-1),
// sb <= 13 -- at most 2^38 for N = 2048, inside the exactness bound.  Ring degrees 1024 and 2048 (radix-2 split
// + two twisted 512-point transforms), Torus32 (N = 1024) and Torus64.
#include <hip/hip_runtime.h>

#include <memory>
#include <mutex>
#include <new>
#include <type_traits>
#include <vector>

#include "../../include/thfhe_hip.h"
#include "thfhe_common.h"
#include "thfhe_devctx.h"
#include "thfhe_lane.h"

using namespace thfhe;

namespace {

#include "thfhe_transform.h"
#include "thfhe_pm_kernels.h"

}  // namespace

struct THFHE_INTERNAL thfhe_pm_ctx : DevCtx {
    int N = 1024, torus_bits = 32;
    DevBuf d_flag;
    DevBuf d_buf[7];  // small, torus, spec, terms, first, addend, out
};

namespace {
template <int NN, int TB>
int pm_run(thfhe_pm_ctx *c, size_t n_torus, const PMArgs &a) {
    THFHE_TRY((launch_torus_transform<NN, TB>(c->stream, c->d_buf[1].as<void>(), (long)n_torus, c->d_tw.as<cplx>(), c->d_buf[2].as<cplx>())));
    hipLaunchKernelGGL((pm_mac_kernel<NN, TB>), dim3((unsigned)((a.n_out + 3) / 4)), dim3(256), 0, c->stream, a);
    THFHE_HIP(hipGetLastError());
    return THFHE_OK;
}
}  // namespace

extern "C" {

int thfhe_pm_ctx_create(int device, int N, int torus_bits, thfhe_pm_ctx **out) {
    if (!out) return thfhe_fail(THFHE_E_INVALID, "null argument");
    *out = nullptr;
    if (!((N == 1024 && (torus_bits == 32 || torus_bits == 64)) || (N == 2048 && torus_bits == 64)))
        return thfhe_fail(THFHE_E_UNSUPPORTED, "polynomial products: N = 1024 with Torus32 / Torus64, N = 2048 with Torus64");
    std::unique_ptr<thfhe_pm_ctx> c(new (std::nothrow) thfhe_pm_ctx);
    if (!c) return thfhe_fail(THFHE_E_NOMEM, "out of host memory");
    THFHE_TRY(c->open(device, false));
    c->N = N, c->torus_bits = torus_bits;
    THFHE_TRY(c->upload_twiddles(N));
    THFHE_TRY(c->d_flag.grow(sizeof(int)));
    *out = c.release();
    return THFHE_OK;
}

void thfhe_pm_ctx_destroy(thfhe_pm_ctx *c) { ctx_destroy(c); }

int thfhe_pm_mac(thfhe_pm_ctx *c, const int32_t *small, size_t n_small, const void *torus, size_t n_torus, const int32_t *terms, size_t n_terms,
                 const void *addend, void *out, size_t n_out) {
    if (!c || !small || !torus || !out || (!terms && n_terms)) return thfhe_fail(THFHE_E_INVALID, "null argument");
    if (n_out == 0) return THFHE_OK;
    // validate the term list on the host: grouped by output, indices in range
    std::vector<int32_t> first(n_out + 1, 0);
    long prev = -1;
    for (size_t t = 0; t < n_terms; t++) {
        const int32_t j = terms[4 * t], s = terms[4 * t + 1], q = terms[4 * t + 2], sg = terms[4 * t + 3];
        if (j < 0 || (size_t)j >= n_out || s < 0 || (size_t)s >= n_small || q < 0 || (size_t)q >= n_torus || (sg != 1 && sg != -1) || j < prev)
            return thfhe_fail(THFHE_E_INVALID, "term list: need (out, small, torus, +-1) with indices in range and outputs in ascending order");
        prev = j;
        first[j + 1]++;
    }
    for (size_t j = 0; j < n_out; j++) first[j + 1] += first[j];
    DevLock lk(*c);
    if (lk.rc) return lk.rc;
    const size_t N = c->N, wb = c->torus_bits / 8, limbs = c->torus_bits / 16;
    const size_t bytes[7] = {n_small * N * 4, n_torus * N * wb, n_torus * limbs * (N / 2) * sizeof(cplx), (n_terms ? n_terms : 1) * 16, (n_out + 1) * 4,
                             n_out * N * wb, n_out * N * wb};
    for (int q = 0; q < 7; q++) {
        int rc = c->d_buf[q].grow(bytes[q]);
        if (rc) return rc;
    }
    THFHE_HIP(hipMemsetAsync(c->d_flag.as<int>(), 0, sizeof(int), c->stream));
    THFHE_HIP(hipMemcpyAsync(c->d_buf[0].as<void>(), small, bytes[0], hipMemcpyHostToDevice, c->stream));
    THFHE_HIP(hipMemcpyAsync(c->d_buf[1].as<void>(), torus, bytes[1], hipMemcpyHostToDevice, c->stream));
    if (n_terms) THFHE_HIP(hipMemcpyAsync(c->d_buf[3].as<void>(), terms, n_terms * 16, hipMemcpyHostToDevice, c->stream));
    THFHE_HIP(hipMemcpyAsync(c->d_buf[4].as<void>(), first.data(), bytes[4], hipMemcpyHostToDevice, c->stream));
    if (addend) THFHE_HIP(hipMemcpyAsync(c->d_buf[5].as<void>(), addend, bytes[5], hipMemcpyHostToDevice, c->stream));
    PMArgs a{c->d_buf[0].as<int32_t>(), c->d_buf[2].as<cplx>(), c->d_buf[3].as<int32_t>(), c->d_buf[4].as<int32_t>(),
             addend ? c->d_buf[5].as<void>() : nullptr, c->d_buf[6].as<void>(), c->d_tw.as<cplx>(), (long)n_out, c->d_flag.as<int>()};
    int rc = c->N == 2048 ? pm_run<2048, 64>(c, n_torus, a) : (c->torus_bits == 64 ? pm_run<1024, 64>(c, n_torus, a) : pm_run<1024, 32>(c, n_torus, a));
    if (rc) return rc;
    int flag = 0;
    THFHE_HIP(hipMemcpyAsync(out, c->d_buf[6].as<void>(), bytes[6], hipMemcpyDeviceToHost, c->stream));
    THFHE_HIP(hipMemcpyAsync(&flag, c->d_flag.as<int>(), sizeof(int), hipMemcpyDeviceToHost, c->stream));
    THFHE_HIP(hipStreamSynchronize(c->stream));
    if (flag) return thfhe_fail(THFHE_E_UNSUPPORTED, "a small-operand coefficient exceeds 2^12 (outside the FP64 exactness bound of the product)");
    return THFHE_OK;
}

}  // extern "C"
