// exchange_emu.cpp -- TEST INFRASTRUCTURE ONLY (never linked into libthfhe_hip.so).  Replays variant "x" of torus-fhe_amd/csrc/thfhe_lane.h (the ring
// kernel's transforms: the folded passes of "f" around the exchange of register bits (2, 1, 0) with lane bits (3, 5, 4)) lane by lane on the host.
// The exchange is modelled MOVE BY MOVE on the 64 x 8 x 4 dwords of a wave: v_mov_b32_dpp row_ror:8 with its bank mask, v_permlane32_swap,
// v_permlane16_swap, in the order and on the registers wave_transpose_x3 (thfhe_common.h) uses.  Next to it the table form (fwd_seg1..3) it must
// agree with and the "s" form that transforms the key.  The same file builds as a stand-alone program (-DEXCHANGE_EMU_MAIN) for sanitizer runs.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../torus-fhe_amd/csrc/thfhe_lane.h"

using namespace thfhe;

namespace {
// ---- the three lane instructions on one dword register of a wave ----
using Reg = uint32_t[64];
// v_mov_b32_dpp dst, src row_ror:8 row_mask:0xf bank_mask:BM -- lane l of a 16-lane row reads lane l ^ 8; a lane whose bank (l >> 2) & 3 is not in
// BM keeps dst (the builtin's `old` operand)
void dpp_ror8(Reg &dst, const Reg &old, const Reg &src, unsigned bank_mask) {
    Reg out;
    for (int l = 0; l < 64; l++) out[l] = (bank_mask >> ((l >> 2) & 3)) & 1 ? src[l ^ 8] : old[l];
    memcpy(dst, out, sizeof(out));
}
// v_permlane32_swap a, b: a of the upper half-wave <-> b of the lower half-wave
void permlane32_swap(Reg &a, Reg &b) {
    for (int l = 0; l < 32; l++) {
        const uint32_t t = a[l + 32];
        a[l + 32] = b[l];
        b[l] = t;
    }
}
// v_permlane16_swap a, b: a of the odd 16-lane rows <-> b of the even rows
void permlane16_swap(Reg &a, Reg &b) {
    for (int l = 0; l < 64; l++) {
        if (l & 16) continue;
        const uint32_t t = a[l + 16];
        a[l + 16] = b[l];
        b[l] = t;
    }
}
int g_moves;   // vector instructions of the last exchange (a kept 64-bit copy counts one)
template <bool FLIPPED>
void lanes_transpose_x3(cplx (*z)[8]) {
    static Reg w[8][4];
    g_moves = 0;
    for (int l = 0; l < 64; l++)
        for (int r = 0; r < 8; r++) {
            uint32_t d[4];
            memcpy(d, &z[l][r], 16);
            for (int k = 0; k < 4; k++) w[r][k][l] = d[k];
        }
    if (FLIPPED) {
        for (int r = 4; r < 8; r++)
            for (int d = 0; d < 4; d++) dpp_ror8(w[r][d], w[r][d], w[r][d], 0xF), g_moves++;
    } else {
        for (int r = 0; r < 4; r++)
            for (int d = 0; d < 4; d++) {
                Reg kept;
                memcpy(kept, w[r + 4][d], sizeof(kept));
                g_moves += (d & 1);   // one v_mov_b64 per double
                dpp_ror8(w[r + 4][d], w[r + 4][d], w[r][d], 0x3), g_moves++;
                dpp_ror8(w[r][d], w[r][d], kept, 0xC), g_moves++;
            }
    }
    for (int d = 0; d < 4; d++) {
        for (int r = 0; r < 8; r++)
            if (!(r & 2)) permlane32_swap(w[r][d], w[r + 2][d]), g_moves++;
        for (int r = 0; r < 8; r += 2) permlane16_swap(w[r][d], w[r + 1][d]), g_moves++;
    }
    for (int l = 0; l < 64; l++)
        for (int r = 0; r < 8; r++) {
            uint32_t d[4];
            for (int k = 0; k < 4; k++) d[k] = w[r][k][l];
            memcpy(&z[l][r], d, 16);
        }
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
struct WaveX {  // variant "x", constants loaded and built as sk_blind_rotate_ring_kernel does
    cplx xbuf[kXbufSlots];
    LaneRootsF rf[64];
    W64 w64[64];
    LaneRoots ri[64];
    uint32_t flip[64];
    cplx bc[64][4];
    int moves_fwd = 0, moves_inv = 0;
    WaveX() {
        const std::vector<cplx> tw = make_twiddle_table(1024);
        for (int l = 0; l < 64; l++) {
            const int nu = lane_nu(l);
            flip[l] = lane_flip_x(l);
            rf[l] = LaneRootsF{tw[TwRing1k::ROOTSF + 2 * nu], tw[TwRing1k::ROOTSF + 2 * nu + 1]};
            w64[l] = lane_w64_x(tw[TwRing1k::T2 + 1 * 8 + (l & 7)], flip[l]);
            ri[l] = lane_roots_x(tw.data(), TwRing1k::T1, TwRing1k::ROOTS, l);
            make_untwist_x(ri[l].b, flip[l], bc[l]);
        }
    }
    // in: lane l holds the coefficients l + 64 m (natural lanes).  out: lane l holds the spectrum of position lane_nu(l)
    void fwd(cplx (*z)[8]) {
        for (int l = 0; l < 64; l++) fwdf_seg1(z[l]);
        lanes_transpose_x3<false>(z);
        moves_fwd = g_moves;
        for (int l = 0; l < 64; l++) fwdx_seg2_st(l, z[l], xbuf, rf[l]);
        for (int l = 0; l < 64; l++) fwdf_seg3(l, z[l], xbuf, rf[l]);
    }
    // in: as fwd leaves it.  out: lane l holds the coefficients lane_nu(l) + 64 m
    void inv(cplx (*z)[8]) {
        for (int l = 0; l < 64; l++) invf_seg1(l, z[l], xbuf);
        for (int l = 0; l < 64; l++) {
            inv_seg2_ld(l, z[l], xbuf);
            invf_seg2(z[l], w64[l]);
        }
        lanes_transpose_x3<true>(z);
        moves_inv = g_moves;
        for (int l = 0; l < 64; l++) invx_seg3(z[l], ri[l], flip[l], bc[l]);
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
// S[m] += z[m] * B[m * 64 + nu], the ring kernel's key read
void mac8_nu(int lane, cplx (&S)[8], const cplx (&z)[8], const cplx *B) { mac8(lane_nu(lane), S, z, B); }
}  // namespace

extern "C" {
// zin: 512 complex in natural order j.  out[nu][m]: the "x" spectra brought back to the natural position nu; back: the "x" inverse (512 z) in natural
// order.  norms[0]: 2-norm of ("x" spectra - table-form spectra), norms[1]: 2-norm of the table-form spectra, norms[2], norms[3]: vector instructions
// of the forward and of the inverse exchange.
void exch_fwd_raw(const double *zin, double *out, double *back, double *norms) {
    static cplx zx[64][8], zt[64][8];
    WaveX wx;
    WaveTable wt;
    load_natural(zin, zx);
    load_natural(zin, zt);
    wx.fwd(zx);
    wt.fwd(zt);
    double d2 = 0, n2 = 0;
    cplx *o = reinterpret_cast<cplx *>(out);
    for (int l = 0; l < 64; l++) {
        const int nu = lane_nu(l);
        for (int m = 0; m < 8; m++) {
            const cplx a = zx[l][m], b = zt[nu][m];
            d2 += (a.re - b.re) * (a.re - b.re) + (a.im - b.im) * (a.im - b.im);
            n2 += b.re * b.re + b.im * b.im;
            o[nu * 8 + m] = a;
        }
    }
    norms[0] = std::sqrt(d2);
    norms[1] = std::sqrt(n2);
    wx.inv(zx);
    norms[2] = wx.moves_fwd;
    norms[3] = wx.moves_inv;
    for (int l = 0; l < 64; l++)
        for (int m = 0; m < 8; m++) {
            back[2 * (lane_nu(l) + 64 * m)] = zx[l][m].re;
            back[2 * (lane_nu(l) + 64 * m) + 1] = zx[l][m].im;
        }
}

// the inverse alone against the table form's inverse on the same spectra (given at natural positions [nu][m]): norms[0] = 2-norm of the difference
// of the 512 outputs, norms[1] = 2-norm of the table form's outputs
void exch_inv_raw(const double *spec, double *norms) {
    static cplx zx[64][8], zt[64][8];
    WaveX wx;
    WaveTable wt;
    const cplx *s = reinterpret_cast<const cplx *>(spec);
    for (int l = 0; l < 64; l++)
        for (int m = 0; m < 8; m++) {
            zx[l][m] = s[lane_nu(l) * 8 + m];
            zt[l][m] = s[l * 8 + m];
        }
    wx.inv(zx);
    for (int l = 0; l < 64; l++) inv_seg1(l, zt[l], wt.xbuf, wt.T2);
    for (int l = 0; l < 64; l++) inv_seg2_ld(l, zt[l], wt.xbuf);
    for (int l = 0; l < 64; l++) inv_seg2_st(l, zt[l], wt.xbuf);
    for (int l = 0; l < 64; l++) inv_seg3(l, zt[l], wt.xbuf, wt.T1);
    double d2 = 0, n2 = 0;
    static cplx nat[512];
    for (int l = 0; l < 64; l++)
        for (int m = 0; m < 8; m++) nat[lane_nu(l) + 64 * m] = zx[l][m];
    for (int l = 0; l < 64; l++)
        for (int m = 0; m < 8; m++) {
            const cplx a = nat[l + 64 * m], b = zt[l][m];
            d2 += (a.re - b.re) * (a.re - b.re) + (a.im - b.im) * (a.im - b.im);
            n2 += b.re * b.re + b.im * b.im;
        }
    norms[0] = std::sqrt(d2);
    norms[1] = std::sqrt(n2);
}

// coefficient-domain key polynomials -> spectral layout [poly][limb][m][lane], scaled by 1/512 (torus_transform_kernel)
void exch_transform_key_polys(const int32_t *polys, int64_t npolys, double *spec /* npolys*2*512*2 doubles */) {
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

// digits (small) x Torus32 polynomial b through forward "x", the multiply-accumulate, inverse "x" and acc_update16; returns the worst distance of
// an inverse output from an integer
double exch_polymul(const int32_t *small, const int32_t *b, int32_t *out) {
    WaveX w;
    std::vector<double> spec(2 * 512 * 2);
    exch_transform_key_polys(b, 1, spec.data());
    const cplx *B = reinterpret_cast<const cplx *>(spec.data());
    static cplx z[64][8], slo[64][8], shi[64][8];
    for (int l = 0; l < 64; l++)
        for (int m = 0; m < 8; m++) z[l][m] = cplx{(double)small[l + 64 * m], (double)small[l + 64 * m + 512]};
    w.fwd(z);
    memset(slo, 0, sizeof(slo));
    memset(shi, 0, sizeof(shi));
    for (int l = 0; l < 64; l++) {
        mac8_nu(l, slo[l], z[l], B);
        mac8_nu(l, shi[l], z[l], B + 512);
    }
    w.inv(slo);
    w.inv(shi);
    std::vector<int32_t> acc(1024, 0);
    for (int l = 0; l < 64; l++) acc_update16(lane_nu(l), acc.data(), slo[l], shi[l]);
    memcpy(out, acc.data(), sizeof(int32_t) * 1024);
    return off_integer(slo, shi, 0);
}

// one CMux on acc[2][1024] with the spectral key of index i (exch_transform_key_polys over the coefficient table [n][2l][2][1024]), in the ring
// kernel's order: fields of the rotated difference once per polynomial, a digit level per row, forward "x", four accumulating spectra, inverse "x".
// Returns the worst distance of an inverse output from an integer.
double exch_mux_rotate(const double *bk_spec, int l_levels, int Bgbit, int i, int barai, int32_t *acc) {
    WaveX w;
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
                for (int l = 0; l < 64; l++) mac8_nu(l, S[c][h][l], z[l], BK + bk_spec_index(i, r, c, h, rows));
    }
    double worst = 0;
    for (int c = 0; c < 2; c++) {
        w.inv(S[c][0]);
        w.inv(S[c][1]);
        worst = off_integer(S[c][0], S[c][1], worst);
        for (int l = 0; l < 64; l++) acc_update16(lane_nu(l), acc + c * 1024, S[c][0][l], S[c][1][l]);
    }
    return worst;
}
}

#ifdef EXCHANGE_EMU_MAIN
// stand-alone run (built with -fsanitize=address,undefined by tests/test_exchange_emu.py): forward against the table form, round trip, a product
// against the schoolbook negacyclic product, every array of the replay touched.  Exit status 0 = all held.
int main() {
    static double zin[1024], out[1024], back[1024], norms[4];
    uint64_t s = 88172645463325252ull;
    auto rnd = [&]() {
        s ^= s << 13, s ^= s >> 7, s ^= s << 17;
        return s;
    };
    for (double &v : zin) v = (double)(int)(rnd() % 1024) - 512.0;
    exch_fwd_raw(zin, out, back, norms);
    int bad = 0;
    if (!(norms[0] <= 1e-12 * norms[1])) bad |= 1;
    for (int j = 0; j < 1024; j++)
        if (std::fabs(back[j] / 512.0 - zin[j]) > 1e-9) bad |= 2;
    if (norms[2] != 72 || norms[3] != 48) bad |= 4;
    exch_inv_raw(out, norms);
    if (!(norms[0] <= 1e-12 * norms[1])) bad |= 8;
    static int32_t a[1024], b[1024], got[1024];
    for (int j = 0; j < 1024; j++) a[j] = (int32_t)(rnd() % 1024) - 512, b[j] = (int32_t)rnd();
    exch_polymul(a, b, got);
    for (int q = 0; q < 1024; q++) {
        uint32_t ref = 0;
        for (int j = 0; j < 1024; j++) {
            const int k = q - j;
            const uint32_t t = (uint32_t)a[j] * (uint32_t)b[k & 1023];
            ref += k < 0 ? 0u - t : t;
        }
        if (ref != (uint32_t)got[q]) bad |= 16;
    }
    printf("exchange_emu: moves fwd %g inv %g, status %d\n", norms[2], norms[3], bad);
    return bad;
}
#endif
