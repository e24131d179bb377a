// thfhe_launch_plan.h -- which blind-rotation kernel a batch runs on, for every engine: the one copy of the rule.
//
// Plain C++17, no HIP: the launchers (launch_br in thfhe_sk.hip, mk_launch_rotation in thfhe_mk.hip, rot2k_launch in thfhe_rot2k.h,
// thfhe_ccs_ctx_create) act on these answers, thfhe_*_rotation_kernel_name reports them, and tests/cpp/launch_plan_test.cpp checks them
// on the host.  The kernel names are what profiles, bench.py and the GPU tests' coverage assertions read.
#pragma once

#include <cstddef>
#include <cstdio>

namespace thfhe {
namespace launch_plan {

// ---- single key (thfhe_sk.hip) -----------------------------------------------------------------------------------------------------------
// Measured on one MI355X (256 CUs, SK-128; profiles/r04_time_batch.txt): a round of the eight-wave ring kernel takes 14.9 ms whether its
// workgroups hold 1 025 or 2 048 jobs between them, a round of the four-wave shape 9.8 ms for up to 1 024 jobs, the cooperative kernel
// 3.0 ms per 256 jobs.  So a batch is cut into whole rounds of 2 048 jobs on the eight-wave kernel plus a remainder r on the cheapest
// shape: cooperative up to coop_max (default 768: 8.6 ms), four-wave ring up to ring4_max (1 024), four-wave ring + one cooperative round
// up to ring4_max + 256 (12.9 ms), else one more eight-wave round.  (3 072 rotations: 30.1 ms as one launch of 384 eight-wave workgroups,
// 24.8 ms as 2 048 + 1 024.)  Both thresholds 0: everything on the eight-wave kernel.
enum SkShape : int { kRing8, kRing4, kCoop };
struct SkPiece {
    SkShape shape;
    long first, count;   // jobs [first, first + count) of the batch
};
constexpr long kRound = 2048;   // 256 CUs x 8 jobs
constexpr int kMaxPieces = 3;

inline int sk_rotation_plan(long jobs, int coop_max, int ring4_max, SkPiece pieces[kMaxPieces]) {
    int n = 0;
    const long full = (coop_max > 0 || ring4_max > 0) ? jobs / kRound * kRound : jobs;
    if (full > 0) pieces[n++] = {kRing8, 0, full};
    const long r = jobs - full;
    if (r == 0) return n;
    if (r <= coop_max) pieces[n++] = {kCoop, full, r};
    else if (r <= ring4_max) pieces[n++] = {kRing4, full, r};
    else if (ring4_max > 0 && coop_max > 0 && r <= ring4_max + (coop_max < 256 ? coop_max : 256)) {
        pieces[n++] = {kRing4, full, (long)ring4_max};
        pieces[n++] = {kCoop, full + ring4_max, r - ring4_max};
    } else pieces[n++] = {kRing8, full, r};
    return n;
}

// ---- 3-gen multi key (thfhe_mk.hip) ------------------------------------------------------------------------------------------------------
// Digits beyond 10 bit are cut into balanced parts of <= 9 bit (N = 2048 only: the sets that use a wide base live on that ring,
// J/mk_api.jl:214-298); |sum| <= 2 l parts N 2^(pw-1) 2^15 <= 2^36.6 stays inside the N = 2048 exactness bound.
// l x parts <= 3: the one-pass N = 2048 kernel; more row parts (the 256-party set: l = 2, Bgbit = 18 -> 2 x 2 parts) go through the batched
// rotation of thfhe_rot2k.h, which knows one- and two-part digits.  Exactness: 2 l parts N 2^(part bits - 1) 2^15 <= 2^37 (section 4.3).
struct MkDigitParts {
    int parts, pw;   // parts per digit; bits per part (0: digits are not cut)
    bool batched;
};
inline MkDigitParts mk_digit_parts(int N, int l, int Bgbit) {
    const int parts = Bgbit > 10 ? (Bgbit + 8) / 9 : 1;
    const int pw = parts > 1 ? (Bgbit + parts - 1) / parts : 0;
    return {parts, pw, N == 2048 && l * parts > 3};
}

// one job per workgroup up to `pair_threshold` jobs (one per CU), two above (thfhe_rot2k.h, and the pair kernels of thfhe_mk.hip)
inline bool rot2k_pair(long jobs, long pair_threshold) { return jobs > pair_threshold; }

enum MkFamily : int { kR4k, kRot2kSingle, kRot2kPair, kCoop2k, kPair2k, kMkCoop, kMkPair };
struct MkChoice {
    MkFamily family;
    int LE;   // the kernel's template argument: l x parts at N = 2048, l at N = 1024; 0 where the kernel has none
};
inline MkChoice mk_rotation_choice(int N, int l, int parts, bool batched, long jobs, long pair_threshold) {
    const bool pair = rot2k_pair(jobs, pair_threshold);
    if (N == 4096) return {kR4k, 0};
    if (batched) return {pair ? kRot2kPair : kRot2kSingle, 0};
    if (N == 2048) return {pair ? kPair2k : kCoop2k, l * parts};   // more gates than CUs: two gates per workgroup share every key chunk
    return {l <= 3 && pair ? kMkPair : kMkCoop, l};               // the pair kernel exists for l <= 3
}

// ---- CCS (thfhe_ccs.hip) -----------------------------------------------------------------------------------------------------------------
constexpr int kCcsMaxParties = 8;   // accumulators the one-pass kernel holds in the LDS, less one
inline bool ccs_wide(int parties, int l) { return parties > kCcsMaxParties || l > 8; }

// ---- names -------------------------------------------------------------------------------------------------------------------------------
// Each writes the kernel's name into buf and returns its length, as snprintf does (>= len: it did not fit).

// the kernel of the plan's first piece: whole rounds come first, so this is the shape that does most of a batch; an empty batch names the
// eight-wave kernel
inline int sk_kernel_name(int l, long jobs, int coop_max, int ring4_max, char *buf, size_t len) {
    SkPiece pc[kMaxPieces];
    const SkShape s = sk_rotation_plan(jobs, coop_max, ring4_max, pc) ? pc[0].shape : kRing8;
    return std::snprintf(buf, len, s == kCoop ? "sk_blind_rotate_coop_kernel<%d>" : s == kRing4 ? "sk_blind_rotate_ring_kernel<%d, 4 waves>" : "sk_blind_rotate_ring_kernel<%d>", l);
}
inline int kms_kernel_name(long jobs, long pair_threshold, char *buf, size_t len) {
    return std::snprintf(buf, len, "%s", rot2k_pair(jobs, pair_threshold) ? "kms_tlev_rotate_pair_kernel" : "kms_tlev_rotate_kernel");
}
inline int mk_kernel_name(int N, int l, int parts, bool batched, long jobs, long pair_threshold, char *buf, size_t len) {
    const MkChoice ch = mk_rotation_choice(N, l, parts, batched, jobs, pair_threshold);
    switch (ch.family) {
    case kR4k: return std::snprintf(buf, len, "r4k_rotate_kernel");
    case kRot2kSingle:
    case kRot2kPair: return kms_kernel_name(jobs, pair_threshold, buf, len);
    case kCoop2k: return std::snprintf(buf, len, "mk_blind_rotate_coop2k_kernel<%d>", ch.LE);
    case kPair2k: return std::snprintf(buf, len, "mk_blind_rotate_pair2k_kernel<%d>", ch.LE);
    case kMkPair: return std::snprintf(buf, len, "mk_blind_rotate_pair_kernel<%d>", ch.LE);
    default: return std::snprintf(buf, len, "mk_blind_rotate_coop_kernel<%d>", ch.LE);
    }
}
// the packing-rows kernel of `records` records (mk_pack_enqueue, thfhe_mk.hip): the wide one from wide_threshold records on, 0 = never
inline bool mk_pack_wide(size_t records, size_t wide_threshold) { return wide_threshold != 0 && records >= wide_threshold; }
inline int mk_pack_kernel_name(size_t records, size_t wide_threshold, char *buf, size_t len) {
    return std::snprintf(buf, len, "%s", mk_pack_wide(records, wide_threshold) ? "mk_pack_rows_wide_kernel" : "mk_pack_rows_kernel");
}
inline int ccs_kernel_name(bool wide, char *buf, size_t len) {   // wide: ccs_wide of the context's parameters
    return std::snprintf(buf, len, "%s", wide ? "ccs_blind_rotate_wide_kernel" : "ccs_blind_rotate_kernel");
}

}  // namespace launch_plan
}  // namespace thfhe
