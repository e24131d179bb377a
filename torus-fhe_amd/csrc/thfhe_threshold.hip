// thfhe_threshold.hip -- the step AFTER the gate path in the reference's C++ applications, on gfx950:
//   TLweFromLwe           src/libthfhe.cpp:340-348 (= src/KNN_medical_data.cpp:492-500): LWE(N) -> ring sample (a', b')
//   PartialDecrypt        src/libthfhe.cpp:270-293, partialDecrypt src/threshold_decryption_functions.cpp:441-480:
//                         partial = key_share (*) a' + smudging noise, (*) = exact negacyclic product mod 2^32
//                         (libtfhe's torusPolynomialAddMulR; the reference's own nonFFTmul, :357-375, is the exact twin)
//   finalDecrypt          src/libthfhe.cpp:296-315: result = b' - partial_0 + sum_{i>=1} partial_i, bit = result[0] > 0
// The product is the blind-rotate engine's split-limb FP64 transform with the roles swapped: the small integer polynomial
// (the key share, |s| <= 2^9) is transformed once per call, every ciphertext mask is split into two balanced 16-bit limbs
// (two forward, two inverse transforms per ciphertext, one wave each).  |sum| <= N 2^9 2^15 = 2^34: inside the exactness bound.
//   PackLwe               the LWE -> TLWE packing key switch (the reference's TODO at src/Convert.cpp:103):
//                         m <= N LWE samples of any dimension n -> ONE ring sample whose coefficient i holds sample i's phase.
//                         Phase 1 is the shared key switch (thfhe_keyswitch.h) with the packing key's 2N-word TLWE rows into
//                         per-sample T_i; phase 2 (pack_rotate_sum_kernel) sums X^i T_i mod X^N + 1 in integers.
//   PackBoxes             the same key switch into the box layout of a test vector: p samples -> ONE ring sample
//                         whose box i (the N/p coefficients centred on i N/p) holds sample i's phase on every coefficient -- an
//                         encrypted test vector for thfhe_lut_bootstrap_enc.  Phase 2 is pack_boxes_kernel.
#include <hip/hip_runtime.h>

#include <memory>
#include <mutex>
#include <new>
#include <vector>

#include "../../include/thfhe_hip.h"
#include "thfhe_common.h"
#include "thfhe_devctx.h"
#include "thfhe_keyswitch.h"
#include "thfhe_lane.h"
#include "thfhe_pack.h"

using namespace thfhe;

namespace {

__global__ __launch_bounds__(64) void share_transform_kernel(const int32_t *__restrict__ share, const cplx *__restrict__ tw, cplx *__restrict__ spec,
                                                             int *__restrict__ too_big) {
    __shared__ cplx sT1[512];
    __shared__ cplx sX[512];
    const int lane = threadIdx.x;
    for (int t = lane; t < 512; t += 64) sT1[t] = tw[t];
    __syncthreads();
    const W64 w64{tw[TwRing1k::T2 + 1 * 8 + (lane & 7)]};
    cplx z[8];
    int big = 0;
#pragma unroll
    for (int m = 0; m < 8; m++) {
        const int32_t a = share[lane + 64 * m], b = share[lane + 64 * m + 512];
        big |= (a > 512 || a < -512 || b > 512 || b < -512);
        z[m] = cplx{(double)a, (double)b};
    }
    if (big) atomicOr(too_big, 1);
    wave_fft_fwd_s(lane, z, sX, sT1, w64);
#pragma unroll
    for (int m = 0; m < 8; m++) spec[m * 64 + lane] = cplx{z[m].re * (1.0 / 512), z[m].im * (1.0 / 512)};
}

// one wave per ciphertext: partial[c] = share (*) a[c] (+ noise[c])
__global__ __launch_bounds__(256) void partial_decrypt_kernel(const int32_t *__restrict__ a, const int32_t *__restrict__ noise,
                                                              const cplx *__restrict__ spec, const cplx *__restrict__ tw,
                                                              int32_t *__restrict__ out, long count) {
    __shared__ cplx sT1[512];
    __shared__ cplx sX[4][512];
    for (int t = threadIdx.x; t < 512; t += 256) sT1[t] = tw[t];
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const W64 w64{tw[TwRing1k::T2 + 1 * 8 + (lane & 7)]};
    const long c = (long)blockIdx.x * 4 + wave;
    if (c >= count) return;
    cplx zlo[8], zhi[8], S[8];
    key_limbs_to_z(lane, a + c * 1024, zlo, zhi);
    load8(lane, S, spec);
    wave_fft_fwd_s(lane, zlo, sX[wave], sT1, w64);
    wave_fft_fwd_s(lane, zhi, sX[wave], sT1, w64);
#pragma unroll
    for (int m = 0; m < 8; m++) {
        zlo[m] = cmul(zlo[m], S[m]);
        zhi[m] = cmul(zhi[m], S[m]);
    }
    wave_fft_inv_s(lane, zlo, sX[wave], sT1, w64);
    wave_fft_inv_s(lane, zhi, sX[wave], sT1, w64);
    int32_t *o = out + c * 1024;
    const int32_t *e = noise ? noise + c * 1024 : nullptr;
#pragma unroll
    for (int m = 0; m < 8; m++) {
        const int q = lane + 64 * m;
        uint32_t vr = round_lo32(zlo[m].re) + (round_lo32(zhi[m].re) << 16);
        uint32_t vi = round_lo32(zlo[m].im) + (round_lo32(zhi[m].im) << 16);
        if (e) {
            vr += (uint32_t)e[q];
            vi += (uint32_t)e[q + 512];
        }
        o[q] = (int32_t)vr;
        o[q + 512] = (int32_t)vi;
    }
}

__global__ __launch_bounds__(256) void tlwe_from_lwe_kernel(const int32_t *__restrict__ lwe, int32_t *__restrict__ ta, int32_t *__restrict__ tb, long count) {
    const long c = blockIdx.x;
    if (c >= count) return;
    const int32_t *x = lwe + c * 1025;
    for (int q = threadIdx.x; q < 1024; q += 256) {
        ta[c * 1024 + q] = q == 0 ? x[0] : (int32_t)(0u - (uint32_t)x[1024 - q]);
        tb[c * 1024 + q] = q == 0 ? x[1024] : 0;
    }
}

__global__ __launch_bounds__(256) void final_decrypt_kernel(const int32_t *__restrict__ tb, const int32_t *__restrict__ partials, int t, long count,
                                                            int32_t *__restrict__ result, int32_t *__restrict__ bits) {
    const long c = blockIdx.x;
    if (c >= count) return;
    for (int q = threadIdx.x; q < 1024; q += 256) {
        uint32_t v = (uint32_t)tb[c * 1024 + q];
        for (int i = 0; i < t; i++) {
            const uint32_t pv = (uint32_t)partials[((size_t)i * count + c) * 1024 + q];
            v = i == 0 ? v - pv : v + pv;
        }
        if (result) result[c * 1024 + q] = (int32_t)v;
        if (q == 0) bits[c] = (int32_t)v > 0 ? 1 : 0;
    }
}

// LWE records [count][n + 1] -> [count][n_pad + 1]: the mask padded with zeros (zero digits: no key row), b last
__global__ __launch_bounds__(256) void pack_pad_lwe_kernel(const int32_t *__restrict__ lwe, int n, int n_pad, long count, int32_t *__restrict__ out) {
    const long c = blockIdx.x;
    if (c >= count) return;
    for (int q = threadIdx.x; q <= n_pad; q += 256)
        out[c * (n_pad + 1) + q] = q < n ? lwe[c * (n + 1) + q] : q == n_pad ? lwe[c * (n + 1) + n] : 0;
}

// P_g = sum_{i < m_g} X^i T_{g m + i} mod X^N + 1 for both polynomials of the 2N-word records T (alpha: words [0, N), beta: [N, 2N)).
// grid = (outputs, 2N / 64): block (g, w) owns words [64 w, 64 w + 64) of output g; its 16 waves take the rows i = wave (mod 16), lane
// = coefficient, and meet in LDS.  Coefficient c of X^i f is f[c - i] for c >= i and -f[c - i + N] below: integer sums, no atomics.
__global__ __launch_bounds__(1024) void pack_rotate_sum_kernel(const int32_t *__restrict__ T, long count, int m, int N, int32_t *__restrict__ out_a,
                                                               int32_t *__restrict__ out_b) {
    __shared__ uint32_t sRed[16][64];
    const long g = blockIdx.x;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int word = (int)blockIdx.y * 64 + lane;
    const int poly = word >= N, c = word - poly * N;
    const long row0 = g * m;
    const int mg = (int)(count - row0 < m ? count - row0 : m);
    const uint32_t *src = reinterpret_cast<const uint32_t *>(T) + (size_t)row0 * 2 * N + (size_t)poly * N;
    uint32_t acc = 0;
#pragma unroll 8
    for (int i = wave; i < mg; i += 16) {
        const uint32_t *row = src + (size_t)i * 2 * N;
        acc += c >= i ? row[c - i] : 0u - row[c - i + N];
    }
    sRed[wave][lane] = acc;
    __syncthreads();
    if (wave == 0) {
        uint32_t v = 0;
#pragma unroll
        for (int w = 0; w < 16; w++) v += sRed[w][lane];
        (poly ? out_b : out_a)[g * N + c] = (int32_t)v;
    }
}

// Box packing: output g = U(X) * sum_{i < p} X^{i B} T_{g p + i} mod X^N + 1, B = N / p, U = X^{-B/2} (1 + X + ... + X^{B-1}), N = 1024.
// grid = (outputs, 2): block (g, poly) owns one polynomial (alpha: words [0, N) of the 2N-word records T, beta: [N, 2N)), thread = coefficient c.
//   strided rotate-sum   S[c] = sum_i (X^{i B} T_i)[c]: T_i[c - i B], negated where c < i B -- every word of the p records is read once
//   window sum           (U S)[c] = sum over the negacyclic extension E of S (E[j + N] = -E[j]) of E[j], c - B/2 < j <= c + B/2.  With the
//                        inclusive prefix sums Pre of S (Hillis-Steele scan in LDS) and Tot = Pre[N - 1], the prefix of E up to j is
//                        Pre[j] inside [0, N) and Tot - Pre[j mod N] one period below or above; the window is a difference of two.
// Integer sums mod 2^32, no atomics; 64-bit offsets into T.
__global__ __launch_bounds__(1024) void pack_boxes_kernel(const int32_t *__restrict__ T, int p, int32_t *__restrict__ out_a, int32_t *__restrict__ out_b) {
    __shared__ uint32_t sP[2][1024];
    const size_t g = blockIdx.x;
    const int poly = blockIdx.y, c = threadIdx.x;
    const int B = 1024 / p;
    const uint32_t *src = reinterpret_cast<const uint32_t *>(T) + g * p * 2048 + (size_t)poly * 1024;
    uint32_t acc = 0;
#pragma unroll 8
    for (int i = 0; i < p; i++) {
        const int e = c - i * B;   // in (-N, N)
        const uint32_t v = src[(size_t)i * 2048 + (e & 1023)];
        acc += e < 0 ? 0u - v : v;
    }
    int cur = 0;
    sP[0][c] = acc;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
        uint32_t v = sP[cur][c];
        if (c >= d) v += sP[cur][c - d];
        sP[cur ^ 1][c] = v;
        __syncthreads();
        cur ^= 1;
    }
    const uint32_t tot = sP[cur][1023];
    const int hi = c + B / 2, lo = c - B / 2;   // hi < 2N, lo >= -N
    const uint32_t ph = hi < 1024 ? sP[cur][hi] : tot - sP[cur][hi & 1023];
    const uint32_t pl = lo >= 0 ? sP[cur][lo] : tot - sP[cur][lo & 1023];
    (poly ? out_b : out_a)[g * 1024 + c] = (int32_t)(ph - pl);
}

// below this many samples the packing key switch runs the plain kernel (rows of 2N words, coordinates in ranges of 64); from here on the
// matrix cores, whose cost up to 256 samples is about one pass over the planes (measured, SK-128, whole calls: 4 samples 0.096 ms plain /
// 0.095 matrix cores, 8 0.107 / 0.103, 16 0.120 / 0.103, 31 0.176 / 0.108)
constexpr long kPackMfmaMinSamples = 8;

}  // namespace

struct THFHE_INTERNAL thfhe_poly_ctx : DevCtx {
    DevBuf d_spec, d_flag;
    DevBuf d_buf[4];
    KsKey pk;        // the packing key (thfhe_pack_key_set)
    int pk_n = 0;    // its LWE dimension; 0: no key
    DevBuf d_pin, d_pt;   // padded LWE input, per-sample T_i
};

namespace {

// phase 1 of thfhe_pack_lwe / thfhe_pack_boxes on device records: pad the masks, key-switch with the packing key into c->d_pt [count][2N]
int pack_per_sample(thfhe_poly_ctx *c, const int32_t *d_lwe, size_t count, hipStream_t stream) {
    const int n = c->pk_n, n_pad = c->pk.N, N = 1024;
    int rc = c->d_pin.grow(count * (n_pad + 1) * 4);
    if (!rc) rc = c->d_pt.grow(count * 2 * N * 4);
    if (rc) return rc;
    hipLaunchKernelGGL(pack_pad_lwe_kernel, dim3((unsigned)count), dim3(256), 0, stream, d_lwe, n, n_pad, (long)count, c->d_pin.as<int32_t>());
    THFHE_HIP(hipGetLastError());
    KsArgs k = c->pk.args(c->d_pin.as<int32_t>(), c->d_pt.as<int32_t>(), (long)count);
    k.out_rec = 2 * N, k.b_col = N;   // (u_rec = n_pad + 1: args' default)
    return ks_enqueue(c->pk, k, n_pad / 64, stream, kPackMfmaMinSamples);
}

}  // namespace

namespace thfhe {

int pack_ctx_device(thfhe_poly_ctx *c) { return c->device; }
hipStream_t pack_ctx_stream(thfhe_poly_ctx *c) { return c->stream; }
std::mutex &pack_ctx_mutex(thfhe_poly_ctx *c) { return c->mu; }
int pack_key_n(thfhe_poly_ctx *c) { return c->pk_n; }

int pack_boxes_reserve(thfhe_poly_ctx *c, size_t count) {
    THFHE_TRY(c->d_pin.grow(count * (c->pk.N + 1) * 4));
    return c->d_pt.grow(count * 2 * 1024 * 4);
}

int pack_boxes_enqueue(thfhe_poly_ctx *c, const int32_t *d_lwe, size_t count, int p, int32_t *d_a, int32_t *d_b, hipStream_t stream) {
    THFHE_TRY(pack_per_sample(c, d_lwe, count, stream));
    hipLaunchKernelGGL(pack_boxes_kernel, dim3((unsigned)(count / p), 2), dim3(1024), 0, stream, c->d_pt.as<int32_t>(), p, d_a, d_b);
    THFHE_HIP(hipGetLastError());
    return THFHE_OK;
}

}  // namespace thfhe

extern "C" {

int thfhe_poly_ctx_create(int device, int N, thfhe_poly_ctx **out) {
    if (!out) return thfhe_fail(THFHE_E_INVALID, "null argument");
    *out = nullptr;
    if (N != 1024) return thfhe_fail(THFHE_E_UNSUPPORTED, "only N = 1024 (k = 1) is implemented");
    std::unique_ptr<thfhe_poly_ctx> c(new (std::nothrow) thfhe_poly_ctx);
    if (!c) return thfhe_fail(THFHE_E_NOMEM, "out of host memory");
    THFHE_TRY(c->open(device, false));
    THFHE_TRY(c->upload_twiddles(1024));
    THFHE_TRY(c->d_spec.grow(512 * sizeof(cplx)));
    THFHE_TRY(c->d_flag.grow(sizeof(int)));
    *out = c.release();
    return THFHE_OK;
}

void thfhe_poly_ctx_destroy(thfhe_poly_ctx *c) { ctx_destroy(c); }

int thfhe_tlwe_from_lwe(thfhe_poly_ctx *c, const int32_t *lwe, int32_t *tlwe_a, int32_t *tlwe_b, size_t count) {
    if (!c || !lwe || !tlwe_a || !tlwe_b) return thfhe_fail(THFHE_E_INVALID, "null argument");
    if (count == 0) return THFHE_OK;
    DevLock lk(*c);
    if (lk.rc) return lk.rc;
    int rc = c->d_buf[0].grow(count * 1025 * 4);
    if (!rc) rc = c->d_buf[1].grow(count * 1024 * 4);
    if (!rc) rc = c->d_buf[2].grow(count * 1024 * 4);
    if (rc) return rc;
    THFHE_HIP(hipMemcpyAsync(c->d_buf[0].as<void>(), lwe, count * 1025 * 4, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(tlwe_from_lwe_kernel, dim3((unsigned)count), dim3(256), 0, c->stream, c->d_buf[0].as<int32_t>(), c->d_buf[1].as<int32_t>(),
                       c->d_buf[2].as<int32_t>(), (long)count);
    THFHE_HIP(hipGetLastError());
    THFHE_HIP(hipMemcpyAsync(tlwe_a, c->d_buf[1].as<void>(), count * 1024 * 4, hipMemcpyDeviceToHost, c->stream));
    THFHE_HIP(hipMemcpyAsync(tlwe_b, c->d_buf[2].as<void>(), count * 1024 * 4, hipMemcpyDeviceToHost, c->stream));
    THFHE_HIP(hipStreamSynchronize(c->stream));
    return THFHE_OK;
}

int thfhe_partial_decrypt(thfhe_poly_ctx *c, const int32_t *key_share, const int32_t *tlwe_a, const int32_t *noise, int32_t *partial, size_t count) {
    if (!c || !key_share || !tlwe_a || !partial) return thfhe_fail(THFHE_E_INVALID, "null argument");
    if (count == 0) return THFHE_OK;
    DevLock lk(*c);
    if (lk.rc) return lk.rc;
    const size_t bytes = count * 1024 * 4;
    int rc = c->d_buf[0].grow(bytes);
    if (!rc) rc = c->d_buf[1].grow(bytes);
    if (!rc) rc = c->d_buf[2].grow(bytes);
    if (!rc) rc = c->d_buf[3].grow(1024 * 4);
    if (rc) return rc;
    THFHE_HIP(hipMemcpyAsync(c->d_buf[3].as<void>(), key_share, 1024 * 4, hipMemcpyHostToDevice, c->stream));
    THFHE_HIP(hipMemcpyAsync(c->d_buf[0].as<void>(), tlwe_a, bytes, hipMemcpyHostToDevice, c->stream));
    if (noise) THFHE_HIP(hipMemcpyAsync(c->d_buf[1].as<void>(), noise, bytes, hipMemcpyHostToDevice, c->stream));
    THFHE_HIP(hipMemsetAsync(c->d_flag.as<int>(), 0, sizeof(int), c->stream));
    hipLaunchKernelGGL(share_transform_kernel, dim3(1), dim3(64), 0, c->stream, c->d_buf[3].as<int32_t>(), c->d_tw.as<cplx>(), c->d_spec.as<cplx>(), c->d_flag.as<int>());
    hipLaunchKernelGGL(partial_decrypt_kernel, dim3((unsigned)((count + 3) / 4)), dim3(256), 0, c->stream, c->d_buf[0].as<int32_t>(),
                       noise ? c->d_buf[1].as<int32_t>() : nullptr, c->d_spec.as<cplx>(), c->d_tw.as<cplx>(), c->d_buf[2].as<int32_t>(), (long)count);
    THFHE_HIP(hipGetLastError());
    int flag = 0;
    THFHE_HIP(hipMemcpyAsync(&flag, c->d_flag.as<int>(), sizeof(int), hipMemcpyDeviceToHost, c->stream));
    THFHE_HIP(hipMemcpyAsync(partial, c->d_buf[2].as<void>(), bytes, hipMemcpyDeviceToHost, c->stream));
    THFHE_HIP(hipStreamSynchronize(c->stream));
    if (flag) return thfhe_fail(THFHE_E_UNSUPPORTED, "key-share coefficients must satisfy |s| <= 512 (FP64 exactness bound)");
    return THFHE_OK;
}

int thfhe_final_decrypt(thfhe_poly_ctx *c, const int32_t *tlwe_b, const int32_t *partials, int t, int32_t *result, int32_t *bits, size_t count) {
    if (!c || !tlwe_b || !partials || !bits || t < 1) return thfhe_fail(THFHE_E_INVALID, "bad argument");
    if (count == 0) return THFHE_OK;
    DevLock lk(*c);
    if (lk.rc) return lk.rc;
    const size_t bytes = count * 1024 * 4;
    int rc = c->d_buf[0].grow(bytes);
    if (!rc) rc = c->d_buf[1].grow(bytes * t);
    if (!rc) rc = c->d_buf[2].grow(bytes);
    if (!rc) rc = c->d_buf[3].grow(count * 4 > 4096 ? count * 4 : 4096);
    if (rc) return rc;
    THFHE_HIP(hipMemcpyAsync(c->d_buf[0].as<void>(), tlwe_b, bytes, hipMemcpyHostToDevice, c->stream));
    THFHE_HIP(hipMemcpyAsync(c->d_buf[1].as<void>(), partials, bytes * t, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(final_decrypt_kernel, dim3((unsigned)count), dim3(256), 0, c->stream, c->d_buf[0].as<int32_t>(), c->d_buf[1].as<int32_t>(), t,
                       (long)count, result ? c->d_buf[2].as<int32_t>() : nullptr, c->d_buf[3].as<int32_t>());
    THFHE_HIP(hipGetLastError());
    if (result) THFHE_HIP(hipMemcpyAsync(result, c->d_buf[2].as<void>(), bytes, hipMemcpyDeviceToHost, c->stream));
    THFHE_HIP(hipMemcpyAsync(bits, c->d_buf[3].as<void>(), count * 4, hipMemcpyDeviceToHost, c->stream));
    THFHE_HIP(hipStreamSynchronize(c->stream));
    return THFHE_OK;
}

int thfhe_pack_key_set(thfhe_poly_ctx *c, const int32_t *pk, int n, int t, int basebit) {
    if (!c || !pk) return thfhe_fail(THFHE_E_INVALID, "null argument");
    if (n < 1 || t < 1 || basebit < 1 || (long)t * basebit > 32) return thfhe_fail(THFHE_E_INVALID, "packing key: need n >= 1, t >= 1, basebit >= 1, t basebit <= 32");
    if (basebit > 4) return thfhe_fail(THFHE_E_UNSUPPORTED, "packing key: basebit <= 4");
    if (n > 2048) return thfhe_fail(THFHE_E_UNSUPPORTED, "packing key: LWE dimension n <= 2048");
    DevLock lk(*c);
    if (lk.rc) return lk.rc;
    c->pk_n = 0;
    THFHE_TRY(c->pk.upload_pack(pk, n, t, basebit, 1024, c->stream));
    c->pk_n = n;
    return THFHE_OK;
}

int thfhe_pack_lwe(thfhe_poly_ctx *c, const int32_t *lwe, size_t count, int slots, int32_t *tlwe_a, int32_t *tlwe_b) {
    if (!c || !lwe || !tlwe_a || !tlwe_b) return thfhe_fail(THFHE_E_INVALID, "null argument");
    if (slots < 1 || slots > 1024) return thfhe_fail(THFHE_E_INVALID, "slots must be in 1 .. N");
    DevLock lk(*c);
    if (lk.rc) return lk.rc;
    if (!c->pk_n) return thfhe_fail(THFHE_E_INVALID, "no packing key set (thfhe_pack_key_set)");
    if (count == 0) return THFHE_OK;
    const int n = c->pk_n, N = 1024;
    const size_t outs = (count + slots - 1) / slots;
    int rc = c->d_buf[0].grow(count * (n + 1) * 4);
    if (!rc) rc = c->d_buf[1].grow(outs * N * 4);
    if (!rc) rc = c->d_buf[2].grow(outs * N * 4);
    if (rc) return rc;
    THFHE_HIP(hipMemcpyAsync(c->d_buf[0].as<void>(), lwe, count * (n + 1) * 4, hipMemcpyHostToDevice, c->stream));
    THFHE_TRY(pack_per_sample(c, c->d_buf[0].as<int32_t>(), count, c->stream));
    hipLaunchKernelGGL(pack_rotate_sum_kernel, dim3((unsigned)outs, (unsigned)(2 * N / 64)), dim3(1024), 0, c->stream, c->d_pt.as<int32_t>(), (long)count,
                       slots, N, c->d_buf[1].as<int32_t>(), c->d_buf[2].as<int32_t>());
    THFHE_HIP(hipGetLastError());
    THFHE_HIP(hipMemcpyAsync(tlwe_a, c->d_buf[1].as<void>(), outs * N * 4, hipMemcpyDeviceToHost, c->stream));
    THFHE_HIP(hipMemcpyAsync(tlwe_b, c->d_buf[2].as<void>(), outs * N * 4, hipMemcpyDeviceToHost, c->stream));
    THFHE_HIP(hipStreamSynchronize(c->stream));
    return THFHE_OK;
}

int thfhe_pack_boxes(thfhe_poly_ctx *c, const int32_t *lwe, size_t count, int p, int32_t *tlwe_a, int32_t *tlwe_b) {
    if (!c || !lwe || !tlwe_a || !tlwe_b) return thfhe_fail(THFHE_E_INVALID, "null argument");
    if (p < 2 || p > 512 || (p & (p - 1))) return thfhe_fail(THFHE_E_INVALID, "p must be a power of two in 2 .. N/2");
    if (count % p) return thfhe_fail(THFHE_E_INVALID, "count must be a multiple of p");
    DevLock lk(*c);
    if (lk.rc) return lk.rc;
    if (!c->pk_n) return thfhe_fail(THFHE_E_INVALID, "no packing key set (thfhe_pack_key_set)");
    if (count == 0) return THFHE_OK;
    const int n = c->pk_n, N = 1024;
    const size_t outs = count / p;
    int rc = c->d_buf[0].grow(count * (n + 1) * 4);
    if (!rc) rc = c->d_buf[1].grow(outs * N * 4);
    if (!rc) rc = c->d_buf[2].grow(outs * N * 4);
    if (rc) return rc;
    THFHE_HIP(hipMemcpyAsync(c->d_buf[0].as<void>(), lwe, count * (n + 1) * 4, hipMemcpyHostToDevice, c->stream));
    THFHE_TRY(pack_boxes_enqueue(c, c->d_buf[0].as<int32_t>(), count, p, c->d_buf[1].as<int32_t>(), c->d_buf[2].as<int32_t>(), c->stream));
    THFHE_HIP(hipMemcpyAsync(tlwe_a, c->d_buf[1].as<void>(), outs * N * 4, hipMemcpyDeviceToHost, c->stream));
    THFHE_HIP(hipMemcpyAsync(tlwe_b, c->d_buf[2].as<void>(), outs * N * 4, hipMemcpyDeviceToHost, c->stream));
    THFHE_HIP(hipStreamSynchronize(c->stream));
    return THFHE_OK;
}

}  // extern "C"
