// thfhe_transform.h -- the forward transform of torus polynomials (bootstrapping keys, public keys, CRS, TLev samples) into limb spectra,
// shared by every engine, and the host staging of party-major key tables.  Included INSIDE the anonymous namespace of each translation
// unit that launches it (after thfhe_common.h and thfhe_devctx.h), so that every unit has its own internal-linkage copy of the kernel.
#ifndef THFHE_TRANSFORM_H
#define THFHE_TRANSFORM_H

// item -> (source polynomial, destination limb spectrum) of torus_transform_kernel for contiguous tables
struct MapIdentity {
    __device__ long src(long p) const { return p; }
    __device__ size_t dst(long p, int h, int limbs) const { return (size_t)p * limbs + h; }
};

// The phased copy of a Torus32, N = 1024 key (variant "p" in thfhe_lane.h; the single-key ring kernels stream it): the layout of MapIdentity; at the
// points whose natural position nu has bit 5 set the value is the spectrum of X^kKeyPhase b_h, the limb polynomial rotated AFTER the split
// (limb_pair_rot32), everywhere else the plain value.  Both come out of the same transform, so the copy costs a second transform per limb.
struct MapPhased : MapIdentity {
    static constexpr bool kPhased = true;
};
template <class Map, class = void>
struct map_is_phased : std::false_type {};
template <class Map>
struct map_is_phased<Map, std::void_t<decltype(Map::kPhased)>> : std::true_type {};

// torus polynomials [NN] of TB-bit words -> balanced 16-bit limb spectra, scaled by 1/(NN/2), one wave per (polynomial, limb): limb h of
// polynomial map.src(p) goes to spec + map.dst(p, h, limbs) * NN/2, i.e. [poly][limb][halves or quarters][512] with MapIdentity.
//   NN = 1024: the "s" form; NN = 2048: radix-2 split + two twisted halves (T1 tables in LDS); NN = 4096: radix-4 split + four twisted
//   quarters in the table-free "tq" form.  Spectra in the register order of the blind-rotate kernels.
template <int NN, int TB, class Map>
__global__ __launch_bounds__(256) void torus_transform_kernel(const void *__restrict__ torus, long npolys, const cplx *__restrict__ tw,
                                                              cplx *__restrict__ spec, Map map) {
    constexpr int LIMBS = TB / 16;
    __shared__ cplx sT1[NN == 2048 ? 2 : 1][512];   // not used (nor allocated) for NN = 4096
    __shared__ cplx sX[4][512];
    if constexpr (NN == 1024) {
        for (int t = threadIdx.x; t < 512; t += 256) sT1[0][t] = tw[TwRing1k::T1 + t];
        __syncthreads();
    } else if constexpr (NN == 2048) {
        for (int t = threadIdx.x; t < 512; t += 256) {
            sT1[0][t] = tw[TwRing2k::T1_TWIST1 + t];
            sT1[1][t] = tw[TwRing2k::T1_TWIST5 + t];
        }
        __syncthreads();
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const W64 w64{tw[tw_t2<NN>() + 1 * 8 + (lane & 7)]};
    const long item = (long)blockIdx.x * 4 + wave;
    if (item >= npolys * LIMBS) return;
    const long p = item / LIMBS;
    const int h = (int)(item % LIMBS);
    const char *poly = static_cast<const char *>(torus) + (size_t)map.src(p) * NN * (TB / 8);
    cplx *dst = spec + map.dst(p, h, LIMBS) * (NN / 2);
    if constexpr (NN == 1024) {
        cplx z[8];
#pragma unroll
        for (int m = 0; m < 8; m++) z[m] = limb_pair<TB>(poly, lane + 64 * m, lane + 64 * m + 512, h);
        wave_fft_fwd_s(lane, z, sX[wave], sT1[0], w64);
        if constexpr (map_is_phased<Map>::value) {
            static_assert(TB == 32, "the phased copy is the single-key ring kernels'");
            cplx y[8];
#pragma unroll
            for (int m = 0; m < 8; m++) y[m] = limb_pair_rot32(reinterpret_cast<const int32_t *>(poly), lane + 64 * m, lane + 64 * m + 512, h, kKeyPhase);
            wave_fft_fwd_s(lane, y, sX[wave], sT1[0], w64);
            if (key_point_phased(lane)) {   // spectra come out at their natural positions: lane = nu
#pragma unroll
                for (int m = 0; m < 8; m++) z[m] = y[m];
            }
        }
#pragma unroll
        for (int m = 0; m < 8; m++) dst[m * 64 + lane] = cplx{z[m].re * (1.0 / 512), z[m].im * (1.0 / 512)};
    } else if constexpr (NN == 2048) {
        cplx z[16], y0[8], y1[8];
#pragma unroll
        for (int m = 0; m < 16; m++) z[m] = limb_pair<TB>(poly, lane + 64 * m, lane + 64 * m + 1024, h);
        split2048(z, y0, y1);
        wave_fft_fwd_t<1>(lane, y0, sX[wave], sT1[0], w64);
        wave_fft_fwd_t<5>(lane, y1, sX[wave], sT1[1], w64);
#pragma unroll
        for (int m = 0; m < 8; m++) {
            dst[m * 64 + lane] = cplx{y0[m].re * (1.0 / 1024), y0[m].im * (1.0 / 1024)};
            dst[512 + m * 64 + lane] = cplx{y1[m].re * (1.0 / 1024), y1[m].im * (1.0 / 1024)};
        }
    } else {
        static_assert(NN == 4096, "ring degrees 1024, 2048 and 4096");
        const cplx ratio = tw[TwRing2k::RATIO + lane];
#pragma unroll
        for (int qt = 0; qt < 4; qt++) {
            cplx y[8];
#pragma unroll
            for (int m = 0; m < 8; m++) {
                cplx u[4];
#pragma unroll
                for (int s = 0; s < 4; s++) u[s] = limb_pair<TB>(poly, lane + 64 * m + 512 * s, lane + 64 * m + 512 * s + 2048, h);
                pre4096(u);
                y[m] = qt == 0 ? comb4096<0>(u) : qt == 1 ? comb4096<1>(u) : qt == 2 ? comb4096<2>(u) : comb4096<3>(u);
            }
            const LaneRoots roots{tw[TwRing2k::ROOTS4K + qt * 64 + lane], ratio};
            if (qt == 0) wave_fft_fwd_tq<1, 64>(lane, y, sX[wave], roots, w64);
            if (qt == 1) wave_fft_fwd_tq<5, 64>(lane, y, sX[wave], roots, w64);
            if (qt == 2) wave_fft_fwd_tq<9, 64>(lane, y, sX[wave], roots, w64);
            if (qt == 3) wave_fft_fwd_tq<13, 64>(lane, y, sX[wave], roots, w64);
            wave_sync();
#pragma unroll
            for (int m = 0; m < 8; m++) dst[qt * 512 + m * 64 + lane] = cplx{y[m].re * (1.0 / 2048), y[m].im * (1.0 / 2048)};
        }
    }
}

template <int NN, int TB, class Map = MapIdentity>
int launch_torus_transform(hipStream_t stream, const void *torus, long npolys, const cplx *tw, cplx *spec, Map map = Map()) {
    hipLaunchKernelGGL((torus_transform_kernel<NN, TB, Map>), dim3((unsigned)((npolys * (TB / 16) + 3) / 4)), dim3(256), 0, stream, torus, npolys, tw,
                       spec, map);
    THFHE_HIP(hipGetLastError());
    return THFHE_OK;
}

// Torus64 key table staged party by party (the 256-party set: 194 MB of coefficients per party): row part (r, part) of output o of key
// bit i is the polynomial src(party, i, r, o) shifted left by part * pw bits (wrapping), so that d (*) K = sum over the digit parts d_w of
// d_w (*) (K << pw w).  d_bk: [party][i][row part r * parts + part][output o][limb][NN/2].
template <int NN, class Src>
int stage_party_keys(DevCtx &c, DevBuf &d_bk, int parties, int n, int rows, int parts, int pw, Src src) {
    const size_t polys_per_party = (size_t)n * rows * parts * 2, party_spec = polys_per_party * 4 * (NN / 2);
    THFHE_TRY(d_bk.grow((size_t)parties * party_spec * sizeof(cplx)));
    DevBuf coeff;  // upload staging
    THFHE_TRY(coeff.grow(polys_per_party * NN * sizeof(int64_t)));
    std::vector<int64_t> host(polys_per_party * NN);
    for (int q = 0; q < parties; q++) {
        int64_t *dst = host.data();
        for (int i = 0; i < n; i++)
            for (int r = 0; r < rows; r++)
                for (int part = 0; part < parts; part++)
                    for (int o = 0; o < 2; o++, dst += NN) {
                        const int64_t *s = src(q, i, r, o);
                        const int sh = part * pw;
                        for (int t = 0; t < NN; t++) dst[t] = (int64_t)((uint64_t)s[t] << sh);
                    }
        THFHE_HIP(hipMemcpyAsync(coeff.as<int64_t>(), host.data(), host.size() * sizeof(int64_t), hipMemcpyHostToDevice, c.stream));
        THFHE_TRY((launch_torus_transform<NN, 64>(c.stream, coeff.as<int64_t>(), (long)polys_per_party, c.d_tw.as<cplx>(), d_bk.as<cplx>() + q * party_spec)));
        THFHE_HIP(hipStreamSynchronize(c.stream));   // `host` is reused for the next party
    }
    return THFHE_OK;
}

#endif
