// fold_emu.cpp -- TEST INFRASTRUCTURE ONLY (never linked into libthfhe_hip.so).  Replays variant "f" of torus-fhe_amd/csrc/thfhe_lane.h (the ring
// kernel's transforms with every inter-pass twiddle folded into the butterflies) lane by lane on the host, the register exchange of
// wave_transpose_hi3 modelled as a permutation, next to the table form (fwd_seg1..3) it must agree with and the "s" form that transforms the key.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../torus-fhe_amd/csrc/thfhe_lane.h"

using namespace thfhe;

namespace {
// host model of wave_transpose_hi3: register index (bits 2,1,0) <-> lane bits (5,4,3)
void lanes_transpose_hi3(cplx (*z)[8]) {
    static cplx t[64][8];
    for (int l = 0; l < 64; l++)
        for (int r = 0; r < 8; r++) t[(l & 7) | (r << 3)][l >> 3] = z[l][r];
    memcpy(z, t, sizeof(t));
}
struct WaveTable {  // the reference form: padded buffer, T1 and T2 from tables
    cplx T1[512], T2[64], xbuf[kXbufSlots];
    WaveTable() { make_twiddles_1024(T1, T2); }
    void fwd(cplx (*z)[8]) {
        for (int l = 0; l < 64; l++) fwd_seg1(l, z[l], xbuf, T1);
        for (int l = 0; l < 64; l++) fwd_seg2_ld(l, z[l], xbuf);
        for (int l = 0; l < 64; l++) fwd_seg2_st(l, z[l], xbuf, T2);
        for (int l = 0; l < 64; l++) fwd_seg3(l, z[l], xbuf);
    }
};
struct WaveKey {  // the form of torus_transform_kernel ("s"): the bootstrapping key's spectra come from it
    cplx T1[512], T2[64], xbuf[512];
    WaveKey() { make_twiddles_1024(T1, T2); }
    void fwd(cplx (*z)[8]) {
        for (int l = 0; l < 64; l++) fwds_seg1(l, z[l], xbuf, T1);
        for (int l = 0; l < 64; l++) fwds_seg2_ld(l, z[l], xbuf);
        for (int l = 0; l < 64; l++) fwds_seg2_st(l, z[l], xbuf, W64{T2[1 * 8 + (l & 7)]});
        for (int l = 0; l < 64; l++) fwds_seg3(l, z[l], xbuf);
    }
};
struct WaveF {  // variant "f", constants loaded and built as sk_blind_rotate_ring_kernel does
    cplx xbuf[kXbufSlots];
    LaneRootsF rf[64];
    W64 w64[64];
    LaneRoots ri[64];
    cplx bc[64][4];
    WaveF() {
        const std::vector<cplx> tw = make_twiddle_table(1024);
        for (int l = 0; l < 64; l++) {
            rf[l] = LaneRootsF{tw[TwRing1k::ROOTSF + 2 * l], tw[TwRing1k::ROOTSF + 2 * l + 1]};
            w64[l] = W64{tw[TwRing1k::T2 + 1 * 8 + (l & 7)]};
            ri[l] = LaneRoots{tw[TwRing1k::ROOTS + 2 * l], tw[TwRing1k::ROOTS + 2 * l + 1]};
            make_untwist_f(ri[l].b, bc[l]);
        }
    }
    void fwd(cplx (*z)[8]) {
        for (int l = 0; l < 64; l++) fwdf_seg1(z[l]);
        lanes_transpose_hi3(z);
        for (int l = 0; l < 64; l++) fwdf_seg2_st(l, z[l], xbuf, rf[l]);
        for (int l = 0; l < 64; l++) fwdf_seg3(l, z[l], xbuf, rf[l]);
    }
    void inv(cplx (*z)[8]) {
        for (int l = 0; l < 64; l++) invf_seg1(l, z[l], xbuf);
        for (int l = 0; l < 64; l++) {
            inv_seg2_ld(l, z[l], xbuf);
            invf_seg2(z[l], w64[l]);
        }
        lanes_transpose_hi3(z);
        for (int l = 0; l < 64; l++) invf_seg3(z[l], ri[l], bc[l]);
    }
};
void load_natural(const double *zin, cplx (*z)[8]) {
    for (int l = 0; l < 64; l++)
        for (int m = 0; m < 8; m++) z[l][m] = cplx{zin[2 * (l + 64 * m)], zin[2 * (l + 64 * m) + 1]};
}
double off_integer(const cplx (*a)[8], const cplx (*b)[8], double worst) {
    for (int l = 0; l < 64; l++)
        for (int m = 0; m < 8; m++)
            for (double v : {a[l][m].re, a[l][m].im, b[l][m].re, b[l][m].im}) worst = std::fmax(worst, std::fabs(v - std::rint(v)));
    return worst;
}
}  // namespace

extern "C" {
// zin: 512 complex in natural order j.  out[lane][m]: the "f" spectra in register order; back: its "f" inverse (512 z) in natural order.
// Returns through norms[0] the 2-norm of (f spectra - table-form spectra), through norms[1] the 2-norm of the table-form spectra.
void fold_fwd_raw(const double *zin, double *out, double *back, double *norms) {
    static cplx zf[64][8], zt[64][8];
    WaveF wf;
    WaveTable wt;
    load_natural(zin, zf);
    load_natural(zin, zt);
    wf.fwd(zf);
    wt.fwd(zt);
    double d2 = 0, n2 = 0;
    for (int l = 0; l < 64; l++)
        for (int m = 0; m < 8; m++) {
            d2 += (zf[l][m].re - zt[l][m].re) * (zf[l][m].re - zt[l][m].re) + (zf[l][m].im - zt[l][m].im) * (zf[l][m].im - zt[l][m].im);
            n2 += zt[l][m].re * zt[l][m].re + zt[l][m].im * zt[l][m].im;
        }
    norms[0] = std::sqrt(d2);
    norms[1] = std::sqrt(n2);
    memcpy(out, zf, sizeof(zf));
    wf.inv(zf);
    for (int l = 0; l < 64; l++)
        for (int m = 0; m < 8; m++) {
            back[2 * (l + 64 * m)] = zf[l][m].re;
            back[2 * (l + 64 * m) + 1] = zf[l][m].im;
        }
}

// coefficient-domain key polynomials -> spectral layout [poly][limb][m][lane], scaled by 1/512 (torus_transform_kernel)
void fold_transform_key_polys(const int32_t *polys, int64_t npolys, double *spec /* npolys*2*512*2 doubles */) {
    WaveKey w;
    static cplx zlo[64][8], zhi[64][8];
    for (int64_t q = 0; q < npolys; q++) {
        for (int l = 0; l < 64; l++) key_limbs_to_z(l, polys + q * 1024, zlo[l], zhi[l]);
        w.fwd(zlo);
        w.fwd(zhi);
        cplx *out = reinterpret_cast<cplx *>(spec) + q * 2 * 512;
        for (int l = 0; l < 64; l++)
            for (int m = 0; m < 8; m++) {
                out[m * 64 + l] = cplx{zlo[l][m].re * (1.0 / 512), zlo[l][m].im * (1.0 / 512)};
                out[512 + m * 64 + l] = cplx{zhi[l][m].re * (1.0 / 512), zhi[l][m].im * (1.0 / 512)};
            }
    }
}

// digits (small) x Torus32 polynomial b through forward "f", the multiply-accumulate, inverse "f" and acc_update16; returns the worst distance of
// an inverse output from an integer
double fold_polymul(const int32_t *small, const int32_t *b, int32_t *out) {
    WaveF w;
    std::vector<double> spec(2 * 512 * 2);
    fold_transform_key_polys(b, 1, spec.data());
    const cplx *B = reinterpret_cast<const cplx *>(spec.data());
    static cplx z[64][8], slo[64][8], shi[64][8];
    for (int l = 0; l < 64; l++)
        for (int m = 0; m < 8; m++) z[l][m] = cplx{(double)small[l + 64 * m], (double)small[l + 64 * m + 512]};
    w.fwd(z);
    memset(slo, 0, sizeof(slo));
    memset(shi, 0, sizeof(shi));
    for (int l = 0; l < 64; l++) {
        mac8(l, slo[l], z[l], B);
        mac8(l, shi[l], z[l], B + 512);
    }
    w.inv(slo);
    w.inv(shi);
    std::vector<int32_t> acc(1024, 0);
    for (int l = 0; l < 64; l++) acc_update16(l, acc.data(), slo[l], shi[l]);
    memcpy(out, acc.data(), sizeof(int32_t) * 1024);
    return off_integer(slo, shi, 0);
}

// one CMux on acc[2][1024] with the spectral key of index i (fold_transform_key_polys over the coefficient table [n][2l][2][1024]), in the ring
// kernel's order: fields of the rotated difference once per polynomial, a digit level per row, forward "f", four accumulating spectra, inverse "f".
// Returns the worst distance of an inverse output from an integer.
double fold_mux_rotate(const double *bk_spec, int l_levels, int Bgbit, int i, int barai, int32_t *acc) {
    WaveF w;
    const cplx *BK = reinterpret_cast<const cplx *>(bk_spec);
    const int rows = 2 * l_levels, a2n = barai & 2047;
    static cplx S[2][2][64][8], z[64][8];
    static uint32_t fld[64][16];
    memset(S, 0, sizeof(S));
    for (int r = 0; r < rows; r++) {
        const int32_t *poly = acc + (r / l_levels) * 1024;
        for (int l = 0; l < 64; l++) {
            if (r % l_levels == 0) rotated_fields_keep<16>(l, poly, a2n, l_levels, Bgbit, fld[l]);
            mixed_digits_z<16>(l, poly, a2n, (r % l_levels) + 1, l_levels, Bgbit, fld[l], z[l]);
        }
        w.fwd(z);
        for (int c = 0; c < 2; c++)
            for (int h = 0; h < 2; h++)
                for (int l = 0; l < 64; l++) mac8(l, S[c][h][l], z[l], BK + bk_spec_index(i, r, c, h, rows));
    }
    double worst = 0;
    for (int c = 0; c < 2; c++) {
        w.inv(S[c][0]);
        w.inv(S[c][1]);
        worst = off_integer(S[c][0], S[c][1], worst);
        for (int l = 0; l < 64; l++) acc_update16(l, acc + c * 1024, S[c][0][l], S[c][1][l]);
    }
    return worst;
}
}
