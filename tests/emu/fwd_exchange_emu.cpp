// fwd_exchange_emu.cpp -- TEST INFRASTRUCTURE ONLY (never linked into libthfhe_hip.so).  Replays variant "p" of torus-fhe_amd/csrc/thfhe_lane.h: the
// ring kernel's forward transform with the UNMASKED lane-bit-3 exchange stage (16 row_ror:8 moves, modelled move by move as in exchange_emu.cpp) over
// the phased key copy, whose spectra at the points with bit 5 of nu set are those of X^32 b.  Everything of variant "x" -- the exchange model, the
// table form, the key transform, the inverse, the current forward and the current CMux -- comes from exchange_emu.cpp, which this file includes, so
// the two forms are compared inside one replay.  Builds as a stand-alone program (-DFWD_EXCHANGE_EMU_MAIN) for sanitizer runs.
#include "exchange_emu.cpp"

namespace {
struct WaveP : WaveX {  // forward of "p"; the inverse is that of "x" with the ring kernel's last segment (outputs m + 4 left without the scale R)
    // in: lane l holds the coefficients lane_nu(l) + 64 m.  out: lane l holds the spectrum of position lane_nu(l), times rho^(-32) where nu has bit 5 set
    void fwd(cplx (*z)[8]) {
        for (int l = 0; l < 64; l++) fwdp_seg1(z[l], flip[l]);
        lanes_transpose_x3<true>(z);
        moves_fwd = g_moves;
        for (int l = 0; l < 64; l++) fwdp_seg2_st(l, z[l], xbuf, rf[l], flip[l]);
        for (int l = 0; l < 64; l++) fwdf_seg3(l, z[l], xbuf, rf[l]);
    }
    void inv_ring(cplx (*z)[8]) {
        for (int l = 0; l < 64; l++) invf_seg1(l, z[l], xbuf);
        for (int l = 0; l < 64; l++) {
            inv_seg2_ld(l, z[l], xbuf);
            invf_seg2(z[l], w64[l]);
        }
        lanes_transpose_x3<true>(z);
        for (int l = 0; l < 64; l++) invx_seg3_ring(z[l], ri[l], flip[l], bc[l]);
    }
};
// worst distance from an integer of the values acc_update16_ring rounds: outputs m < 4 as they are, outputs m + 4 times R (exactly: long double)
double off_integer_ring(const cplx (*a)[8], const cplx (*b)[8], double worst) {
    const long double R = 0.70710678118654752440;   // the double the kernel multiplies with
    for (int l = 0; l < 64; l++)
        for (int m = 0; m < 8; m++)
            for (double v : {a[l][m].re, a[l][m].im, b[l][m].re, b[l][m].im}) {
                const long double x = m < 4 ? (long double)v : R * (long double)v;
                worst = std::fmax(worst, (double)fabsl(x - rintl(x)));
            }
    return worst;
}
void load_nu(const double *zin, cplx (*z)[8]) {
    for (int l = 0; l < 64; l++)
        for (int m = 0; m < 8; m++) z[l][m] = cplx{zin[2 * (lane_nu(l) + 64 * m)], zin[2 * (lane_nu(l) + 64 * m) + 1]};
}
// folded input of X^rot p, p the real polynomial folded in z (p_j = Re z_j, p_(j + 512) = Im z_j), -1024 < rot < 1024
void rotate_folded(const double *zin, int rot, double *zout) {
    double p[1024], q[1024];
    for (int j = 0; j < 512; j++) p[j] = zin[2 * j], p[j + 512] = zin[2 * j + 1];
    for (int j = 0; j < 1024; j++) {
        const int e = (j - rot) & 2047;
        q[j] = (e & 1024) ? -p[e & 1023] : p[e & 1023];
    }
    for (int j = 0; j < 512; j++) zout[2 * j] = q[j], zout[2 * j + 1] = q[j + 512];
}
// the key transform on limb inputs read through the rotation (rot = 0: the plain key): [limb][m][lane], scaled by 1/512
void key_spectra_rot(const int32_t *poly, int rot, cplx *out) {
    WaveKey w;
    static cplx z[2][64][8];
    for (int h = 0; h < 2; h++) {
        for (int l = 0; l < 64; l++)
            for (int m = 0; m < 8; m++) z[h][l][m] = limb_pair_rot32(poly, l + 64 * m, l + 64 * m + 512, h, rot);
        w.fwd(z[h]);
        for (int l = 0; l < 64; l++)
            for (int m = 0; m < 8; m++) out[h * 512 + m * 64 + l] = cplx{z[h][l][m].re * (1.0 / 512), z[h][l][m].im * (1.0 / 512)};
    }
}
void merge_phased(const cplx *plain, const cplx *rotated, cplx *out) {   // per (limb, m): the rotated spectrum at the phased points
    for (int t = 0; t < 1024; t++) out[t] = key_point_phased(t & 63) ? rotated[t] : plain[t];
}
}  // namespace

extern "C" {
// zin: 512 complex in natural order.  out[nu][m]: the "p" spectra at the natural positions.  norms: [0] 2-norm of ("p" - table form of p) over the
// points with bit 5 of nu clear, [1] 2-norm of the table form there, [2] 2-norm of ("p" - table form of X^(-32) p) over the other points, [3] 2-norm
// of that table form there, [4] vector instructions of the exchange, [5] 2-norm of ("p" - table form of p) over the phased points (the control: it
// must NOT be small)
void fxe_fwd_raw(const double *zin, double *out, double *norms) {
    static cplx zp[64][8], zt[64][8], zr[64][8];
    static double zrot[1024];
    WaveP wp;
    WaveTable wt;
    load_nu(zin, zp);
    load_natural(zin, zt);
    rotate_folded(zin, -kKeyPhase, zrot);
    load_natural(zrot, zr);
    wp.fwd(zp);
    wt.fwd(zt);
    wt.fwd(zr);
    double acc[6] = {0, 0, 0, 0, 0, 0};
    cplx *o = reinterpret_cast<cplx *>(out);
    auto d2 = [](cplx a, cplx b) { return (a.re - b.re) * (a.re - b.re) + (a.im - b.im) * (a.im - b.im); };
    for (int l = 0; l < 64; l++) {
        const int nu = lane_nu(l);
        for (int m = 0; m < 8; m++) {
            const cplx a = zp[l][m];
            o[nu * 8 + m] = a;
            if (!key_point_phased(nu)) {
                acc[0] += d2(a, zt[nu][m]);
                acc[1] += d2(zt[nu][m], cplx{0, 0});
            } else {
                acc[2] += d2(a, zr[nu][m]);
                acc[3] += d2(zr[nu][m], cplx{0, 0});
                acc[5] += d2(a, zt[nu][m]);
            }
        }
    }
    for (int k : {0, 1, 2, 3, 5}) norms[k] = std::sqrt(acc[k]);
    norms[4] = wp.moves_fwd;
}

// npolys Torus32 polynomials -> the plain key spectra (as exch_transform_key_polys) and the phased copy the ring kernel streams, both
// [poly][limb][m][lane].  split_after_rotate != 0: the WRONG phased copy, from the limbs of the rotated words (the negative control).
void fxe_transform_key_polys(const int32_t *polys, int64_t npolys, double *plain, double *ring, int split_after_rotate) {
    static cplx pl[1024], ro[1024];
    for (int64_t q = 0; q < npolys; q++) {
        const int32_t *poly = polys + q * 1024;
        key_spectra_rot(poly, 0, pl);
        if (split_after_rotate) {
            int32_t rot[1024];
            for (int j = 0; j < 1024; j++) {
                const int e = (j - kKeyPhase) & 2047;
                rot[j] = (e & 1024) ? (int32_t)(0u - (uint32_t)poly[e & 1023]) : poly[e & 1023];
            }
            key_spectra_rot(rot, 0, ro);
        } else {
            key_spectra_rot(poly, kKeyPhase, ro);
        }
        memcpy(reinterpret_cast<cplx *>(plain) + q * 1024, pl, sizeof(pl));
        merge_phased(pl, ro, reinterpret_cast<cplx *>(ring) + q * 1024);
    }
}

// the phased copy of one polynomial against rho^32 * (plain spectrum), rho = zeta^(4 k + 1) from long double sines: norms[0] = 2-norm of the
// difference over the phased points of both limbs, norms[1] = 2-norm of the plain spectra of both limbs over ALL points (= ||b_lo, b_hi||_2 /
// sqrt(512): the 1/512 is folded in), norms[2] = largest |difference| over the unphased points (a copy: 0)
void fxe_key_phase_check(const int32_t *poly, double *norms) {
    static cplx pl[1024], ro[1024], rg[1024];
    key_spectra_rot(poly, 0, pl);
    key_spectra_rot(poly, kKeyPhase, ro);
    merge_phased(pl, ro, rg);
    long double d2 = 0, n2 = 0;
    double copy = 0;
    const long double pi = 3.14159265358979323846264338327950288L;
    for (int h = 0; h < 2; h++)
        for (int m = 0; m < 8; m++)
            for (int nu = 0; nu < 64; nu++) {
                const cplx a = rg[h * 512 + m * 64 + nu], b = pl[h * 512 + m * 64 + nu];
                n2 += (long double)b.re * b.re + (long double)b.im * b.im;
                if (!key_point_phased(nu)) {
                    copy = std::fmax(copy, std::fmax(std::fabs(a.re - b.re), std::fabs(a.im - b.im)));
                    continue;
                }
                const int k = (nu >> 3) + 8 * (nu & 7) + 64 * m;   // nu = k1 + 8 k0
                const long double ang = pi * (long double)((kKeyPhase * (4 * k + 1)) % 2048) / 1024.0L, c = cosl(ang), s = sinl(ang);
                const long double er = c * b.re - s * b.im - a.re, ei = c * b.im + s * b.re - a.im;
                d2 += er * er + ei * ei;
            }
    norms[0] = (double)sqrtl(d2);
    norms[1] = (double)sqrtl(n2);
    norms[2] = copy;
}

// exch_polymul with the forward of "p" and the phased copy of b's spectra
double fxe_polymul(const int32_t *small, const int32_t *b, int32_t *out, int split_after_rotate) {
    WaveP w;
    std::vector<double> plain(2 * 512 * 2), ring(2 * 512 * 2);
    fxe_transform_key_polys(b, 1, plain.data(), ring.data(), split_after_rotate);
    const cplx *B = reinterpret_cast<const cplx *>(ring.data());
    static cplx z[64][8], slo[64][8], shi[64][8];
    for (int l = 0; l < 64; l++)
        for (int m = 0; m < 8; m++) z[l][m] = cplx{(double)small[lane_nu(l) + 64 * m], (double)small[lane_nu(l) + 64 * m + 512]};
    w.fwd(z);
    memset(slo, 0, sizeof(slo));
    memset(shi, 0, sizeof(shi));
    for (int l = 0; l < 64; l++) {
        mac8_nu(l, slo[l], z[l], B);
        mac8_nu(l, shi[l], z[l], B + 512);
    }
    w.inv_ring(slo);
    w.inv_ring(shi);
    const double off = off_integer_ring(slo, shi, 0);
    std::vector<int32_t> acc(1024, 0);
    for (int l = 0; l < 64; l++) acc_update16_ring(lane_nu(l), acc.data(), slo[l], shi[l]);
    memcpy(out, acc.data(), sizeof(int32_t) * 1024);
    return off;
}

// exch_mux_rotate in the ring kernel's present order: the digits read at nu, forward "p", the phased key copy, the ring kernel's inverse and update
double fxe_mux_rotate(const double *bk_ring, int l_levels, int Bgbit, int i, int barai, int32_t *acc) {
    WaveP w;
    const cplx *BK = reinterpret_cast<const cplx *>(bk_ring);
    const int rows = 2 * l_levels, a2n = barai & 2047;
    static cplx S[2][2][64][8], z[64][8];
    static uint32_t fld[64][16];
    memset(S, 0, sizeof(S));
    for (int r = 0; r < rows; r++) {
        const int32_t *poly = acc + (r / l_levels) * 1024;
        for (int l = 0; l < 64; l++) {
            const int nu = lane_nu(l);
            if (r % l_levels == 0) rotated_fields_keep<16>(nu, poly, a2n, l_levels, Bgbit, fld[l]);
            mixed_digits_z<16>(nu, poly, a2n, (r % l_levels) + 1, l_levels, Bgbit, fld[l], z[l]);
        }
        w.fwd(z);
        for (int c = 0; c < 2; c++)
            for (int h = 0; h < 2; h++)
                for (int l = 0; l < 64; l++) mac8_nu(l, S[c][h][l], z[l], BK + bk_spec_index(i, r, c, h, rows));
    }
    double worst = 0;
    for (int c = 0; c < 2; c++) {
        w.inv_ring(S[c][0]);
        w.inv_ring(S[c][1]);
        worst = off_integer_ring(S[c][0], S[c][1], worst);
        for (int l = 0; l < 64; l++) acc_update16_ring(lane_nu(l), acc + c * 1024, S[c][0][l], S[c][1][l]);
    }
    return worst;
}

// the fused rounding of acc_update16_ring on x[0 .. count): fused[i] = round_scaled_lo32(x[i]), two_step[i] = round_lo32(R x[i]) (the form it replaces)
void fxe_round_scaled(const double *x, int64_t count, uint32_t *fused, uint32_t *two_step) {
    for (int64_t i = 0; i < count; i++) {
        fused[i] = round_scaled_lo32(x[i]);
        two_step[i] = round_lo32(0.70710678118654752440 * x[i]);
    }
}
}

#ifdef FWD_EXCHANGE_EMU_MAIN
// stand-alone run (built with -fsanitize=address,undefined by tests/test_fwd_exchange_emu.py): forward against the table forms, the phased key
// against rho^32 B, a product against the schoolbook negacyclic product and against the current form.  Exit status 0 = all held.
int main() {
    static double zin[1024], out[1024], norms[6];
    uint64_t s = 88172645463325252ull;
    auto rnd = [&]() {
        s ^= s << 13, s ^= s >> 7, s ^= s << 17;
        return s;
    };
    for (double &v : zin) v = (double)(int)(rnd() % 1024) - 512.0;
    fxe_fwd_raw(zin, out, norms);
    int bad = 0;
    if (!(norms[0] <= 1e-12 * norms[1]) || !(norms[2] <= 1e-12 * norms[3])) bad |= 1;
    if (!(norms[5] > 0.1 * norms[3])) bad |= 2;
    if (norms[4] != 48) bad |= 4;
    static int32_t a[1024], b[1024], got[1024], cur[1024];
    for (int j = 0; j < 1024; j++) a[j] = (int32_t)(rnd() % 1024) - 512, b[j] = (int32_t)rnd();
    double kn[3];
    fxe_key_phase_check(b, kn);
    if (!(kn[0] <= 1e-12 * kn[1]) || kn[2] != 0) bad |= 8;
    fxe_polymul(a, b, got, 0);
    exch_polymul(a, b, cur);
    for (int q = 0; q < 1024; q++) {
        uint32_t ref = 0;
        for (int j = 0; j < 1024; j++) {
            const int k = q - j;
            const uint32_t t = (uint32_t)a[j] * (uint32_t)b[k & 1023];
            ref += k < 0 ? 0u - t : t;
        }
        if (ref != (uint32_t)got[q] || got[q] != cur[q]) bad |= 16;
    }
    printf("fwd_exchange_emu: moves fwd %g, status %d\n", norms[4], bad);
    return bad;
}
#endif
