// thfhe_ring_schedule.h -- the slot schedule of the single-key ring kernel's key hand-off (sk_blind_rotate_ring_kernel, thfhe_sk.hip).
//
// Plain constexpr C++, no HIP: the kernel takes its constants from here, and tests/cpp/ring_schedule_test.cpp replays the same tables on the
// host (every chunk issued once and in order, no slot written before the barrier that frees it, no chunk read before the barrier that
// certifies it, the borrowed slot used only between A and B of one row, every vmcnt argument = the younger DMAs in flight).
//
// A digit row consumes four key chunks c0 .. c3 = (column, limb) (0,0), (0,1), (1,0), (1,1), 8 KiB each.  Three slots are resident (the key
// ring); the fourth is BORROWED: the first 8 KiB of transpose buffer 0, which no wave touches between the first and the last barrier of a row
// (transposes happen only inside transforms, and every wave is out of its transform at barrier A and stays out until barrier B).
//
//   barrier A   after the forward transform     certifies c0 c1 c2 (issued one row earlier, or by the prologue) and that sX is idle
//               then: DMA c3 -> borrowed slot;  consume c0, c1, c2 back to back, no barrier between them
//   barrier X                                   certifies c3 and that every wave's reads of c0 .. c2 have returned
//               then: DMA the NEXT row's c0 c1 c2 -> resident slots 0 1 2;  consume c3 from the borrowed slot
//   barrier B   before anything touches sX      certifies that every wave's reads of the borrowed slot have returned
//
// 3 barriers and 4 issues per wave and row (8 at four waves per workgroup: two slices per chunk).  A wave issues the key stream in linear
// order: c3 of row r, then c0 c1 c2 of row r + 1.  Issues past the end of the stream repeat its last chunk (clamped) and are never read.
#pragma once

namespace thfhe {
namespace ring_schedule {

constexpr int kChunksPerRow = 4;
constexpr int kResidentSlots = 3;
constexpr int kBorrowedSlot = 3;          // slot index 3 = the first kSlotBytes of transpose buffer 0
constexpr int kSlots = 4;
constexpr int kSlotBytes = 8192;
constexpr int kSliceBytes = 1024;         // one LDS-DMA of one wave

enum Barrier : int { kBarA = 0, kBarX = 1, kBarB = 2, kBarriersPerRow = 3 };

// the life of chunk c of a row; barriers of "row - 1" are those of the previous row (the prologue stands in for them before row 0)
struct ChunkPlan {
    int slot;            // where it lands
    int issue_barrier;   // issued right after this barrier ...
    int issue_row;       // ... of this row (0) or of the previous one (-1)
    int certify_barrier; // this row's barrier after which it may be read
    int free_barrier;    // this row's barrier after which its slot may be written again
};
constexpr ChunkPlan kPlan[kChunksPerRow] = {
    {0, kBarX, -1, kBarA, kBarX},
    {1, kBarX, -1, kBarA, kBarX},
    {2, kBarX, -1, kBarA, kBarX},
    {kBorrowedSlot, kBarA, 0, kBarX, kBarB},
};
constexpr int kPrologueIssues = 3;        // c0 c1 c2 of the first row, in the slots kPlan gives them

// the chunks consumed between barrier b and the next one: [first_consumed(b), first_consumed(b + 1))
constexpr int first_consumed(int b) {
    int c = 0;
    while (c < kChunksPerRow && kPlan[c].certify_barrier < b) c++;
    return c;
}
// the chunks issued right after barrier b, in issue order: those of this row, then those of the next row
constexpr int issues_at(int b) {
    int k = 0;
    for (int c = 0; c < kChunksPerRow; c++) k += kPlan[c].issue_barrier == b;
    return k;
}
constexpr int issue_chunk(int b, int k) {   // k-th chunk issued after barrier b (row-relative index; see issue_row for whose row)
    for (int row = 0; row >= -1; row--)
        for (int c = 0; c < kChunksPerRow; c++)
            if (kPlan[c].issue_barrier == b && kPlan[c].issue_row == row && k-- == 0) return c;
    return -1;
}
constexpr int issue_slot(int b, int k) { return kPlan[issue_chunk(b, k)].slot; }
// chunks (not DMAs: multiply by the DMAs per wave and chunk) a wave has issued AFTER the youngest chunk barrier b certifies, at the time it
// reaches b: the s_waitcnt vmcnt argument.  A barrier that certifies nothing waits for the chunk certified before it.
constexpr int vmcnt_at(int b) {
    // walk the issue order backwards from barrier b over one period (a row) until the youngest chunk certified at or before b
    int younger = 0;
    for (int back = 0; back < kBarriersPerRow; back++) {
        const int bb = (b - 1 - back + 2 * kBarriersPerRow) % kBarriersPerRow;     // issue groups before b, youngest first
        const bool prev_row = b - 1 - back < 0;
        for (int k = issues_at(bb) - 1; k >= 0; k--) {
            const int c = issue_chunk(bb, k);
            // the chunk issued there belongs to this row or the next (issue_row -1), seen from the row the group sits in
            const int rows_ahead = (kPlan[c].issue_row == -1 ? 1 : 0) - (prev_row ? 1 : 0);   // 0: a chunk of b's row, 1: of the row after
            if (rows_ahead == 0 && kPlan[c].certify_barrier <= b) return younger;
            younger++;
        }
    }
    return younger;
}

static_assert(first_consumed(kBarA) == 0 && first_consumed(kBarX) == 3 && first_consumed(kBarB) == 4 && first_consumed(kBarriersPerRow) == 4, "");
static_assert(issues_at(kBarA) == 1 && issues_at(kBarX) == 3 && issues_at(kBarB) == 0, "");
static_assert(issue_chunk(kBarA, 0) == 3 && issue_chunk(kBarX, 0) == 0 && issue_chunk(kBarX, 1) == 1 && issue_chunk(kBarX, 2) == 2, "");
static_assert(vmcnt_at(kBarA) == 0 && vmcnt_at(kBarX) == 0 && vmcnt_at(kBarB) == 3, "");
static_assert(issues_at(kBarA) + issues_at(kBarX) + issues_at(kBarB) == kChunksPerRow, "");

}  // namespace ring_schedule
}  // namespace thfhe
