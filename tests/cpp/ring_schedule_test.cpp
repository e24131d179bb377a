// Host replay of the ring kernel's key hand-off (torus-fhe_amd/csrc/thfhe_ring_schedule.h): one wave's sequence of barriers, LDS-DMA issues and
// chunk reads, walked from the header's tables by the rules the kernel uses, for l = 1 .. 4, W = 4 and 8, n = 1, 2, 3 and 630.  The eight (four)
// waves of a workgroup run the same sequence, so what holds for one wave between two barriers holds for all of them.  Checked:
//   1  every chunk of the key stream is issued exactly once and in linear order (issues past the end repeat the last chunk and are never read);
//   2  no slot is written before a barrier has passed since its last read;
//   3  no chunk is read before a barrier whose vmcnt wait retired all of its DMAs;
//   4  the borrowed slot is written and read only between barriers A and B of one row, and nothing is in flight into it at B;
//   5  the vmcnt argument of every barrier = the DMAs in flight that are younger than the youngest chunk needed so far.
// The checker is also run on broken schedules, each of which it must reject.  CPU only; built with -fsanitize=address,undefined.
#include <cstdio>
#include <deque>
#include <string>
#include <vector>

#include "../../torus-fhe_amd/csrc/thfhe_ring_schedule.h"

namespace RS = thfhe::ring_schedule;

struct Sched {
    RS::ChunkPlan plan[RS::kChunksPerRow];
    int vm[RS::kBarriersPerRow];   // in chunks
    int prologue;
};

static Sched shipped() {
    Sched s{};
    for (int c = 0; c < RS::kChunksPerRow; c++) s.plan[c] = RS::kPlan[c];
    for (int b = 0; b < RS::kBarriersPerRow; b++) s.vm[b] = RS::vmcnt_at(b);
    s.prologue = RS::kPrologueIssues;
    return s;
}

// chunks issued after barrier b: this row's first, then the next row's, each in chunk order (the rule of RS::issue_chunk)
static std::vector<int> issue_group(const Sched &s, int b) {
    std::vector<int> g;
    for (int row = 0; row >= -1; row--)
        for (int c = 0; c < RS::kChunksPerRow; c++)
            if (s.plan[c].issue_barrier == b && s.plan[c].issue_row == row) g.push_back(c);
    return g;
}
static int first_consumed(const Sched &s, int b) {
    int c = 0;
    while (c < RS::kChunksPerRow && s.plan[c].certify_barrier < b) c++;
    return c;
}

struct Dma {
    long chunk;   // stream index
    bool pad;     // an issue past the end of the stream
    int slot;
};
struct Slot {
    long chunk = -1;
    bool pad = false, certified = false;
    int last_read_epoch = -1;   // barriers passed when it was last read
};

struct Replay {
    const Sched &s;
    int dpc;
    long total;
    std::deque<Dma> fifo;      // this wave's DMAs in flight, oldest first (vmcnt retires in order)
    Slot slot[RS::kSlots];
    long next_issue = 0, next_read = 0, issues = 0;
    long youngest_needed = -1;  // stream index of the youngest chunk a barrier has had to certify so far
    int epoch = 0;              // barriers passed
    int phase = -1;             // last barrier of the current row (-1: outside A .. B)
    std::string err;

    void fail(const std::string &m) {
        if (err.empty()) err = m;
    }
    void issue(int sl) {
        Slot &t = slot[sl];
        if (t.last_read_epoch >= epoch) fail("slot " + std::to_string(sl) + " written before the barrier that frees it");
        if (t.chunk >= 0 && !t.certified && !t.pad) fail("slot " + std::to_string(sl) + " rewritten while a chunk is still landing in it");
        if (sl == RS::kBorrowedSlot && !(phase == RS::kBarA || phase == RS::kBarX)) fail("borrowed slot written outside A .. B");
        const bool pad = next_issue >= total;
        const long q = pad ? total - 1 : next_issue++;
        for (int d = 0; d < dpc; d++) fifo.push_back(Dma{q, pad, sl});
        t.chunk = q, t.pad = pad, t.certified = false;
        issues++;
    }
    void barrier(int b, int vm_dmas) {
        // 5: what the wait has to retire = every DMA up to the youngest chunk read before the next barrier
        long need = youngest_needed;
        for (int c = first_consumed(s, b); c < first_consumed(s, b + 1); c++) need = next_read + (c - first_consumed(s, b));
        youngest_needed = need;
        int younger = 0;
        for (auto it = fifo.rbegin(); it != fifo.rend() && (it->pad || it->chunk > need); ++it) younger++;
        if (vm_dmas != younger)
            fail("barrier " + std::to_string(b) + ": vmcnt(" + std::to_string(vm_dmas) + ") but " + std::to_string(younger) + " younger DMAs in flight");
        while ((int)fifo.size() > vm_dmas) fifo.pop_front();
        for (int sl = 0; sl < RS::kSlots; sl++) {
            bool landing = false;
            for (const Dma &d : fifo) landing |= d.slot == sl;
            if (!landing && slot[sl].chunk >= 0) slot[sl].certified = true;
            if (sl == RS::kBorrowedSlot && b == RS::kBarB && landing) fail("a DMA is in flight into the borrowed slot at barrier B");
        }
        epoch++;
        phase = b == RS::kBarB ? -1 : b;
    }
    void read(int sl) {
        Slot &t = slot[sl];
        if (t.pad || t.chunk != next_read) fail("read " + std::to_string(next_read) + " finds chunk " + std::to_string(t.chunk) + " in slot " + std::to_string(sl));
        if (!t.certified) fail("chunk " + std::to_string(next_read) + " read before the barrier that certifies it");
        if (sl == RS::kBorrowedSlot && !(phase == RS::kBarA || phase == RS::kBarX)) fail("borrowed slot read outside A .. B");
        t.last_read_epoch = epoch;
        next_read++;
    }
    void run(long rows) {
        epoch = 1;   // the __syncthreads in front of the prologue
        for (int k = 0; k < s.prologue; k++) issue(s.plan[k].slot);
        for (long r = 0; r < rows; r++)
            for (int b = 0; b < RS::kBarriersPerRow; b++) {
                barrier(b, s.vm[b] * dpc);
                for (int c : issue_group(s, b)) issue(s.plan[c].slot);
                for (int c = first_consumed(s, b); c < first_consumed(s, b + 1); c++) read(s.plan[c].slot);
            }
        fifo.clear();   // the final vmcnt(0)
        if (next_issue != total) fail("issued " + std::to_string(next_issue) + " of " + std::to_string(total) + " chunks");
        if (next_read != total) fail("read " + std::to_string(next_read) + " of " + std::to_string(total) + " chunks");
    }
};

static std::string check(const Sched &s, int L, int W, long n) {
    Replay r{s, 8 / W, n * 2 * L * RS::kChunksPerRow};
    r.run(n * 2 * L);
    return r.err;
}

int main() {
    int errors = 0, cases = 0;
    const Sched good = shipped();
    // the walk rules used here are the header's
    for (int b = 0; b <= RS::kBarriersPerRow; b++) errors += first_consumed(good, b) != RS::first_consumed(b);
    for (int b = 0; b < RS::kBarriersPerRow; b++) {
        const std::vector<int> g = issue_group(good, b);
        errors += (int)g.size() != RS::issues_at(b);
        for (int k = 0; k < (int)g.size() && k < RS::issues_at(b); k++) errors += g[k] != RS::issue_chunk(b, k) || good.plan[g[k]].slot != RS::issue_slot(b, k);
    }
    // the slices of the W waves tile a slot exactly once, and the borrowed slot fits the 576-slot transpose buffer
    for (int W : {4, 8}) {
        std::vector<int> hit(RS::kSlotBytes / RS::kSliceBytes, 0);
        for (int w = 0; w < W; w++)
            for (int d = 0; d < 8 / W; d++) hit[(w * (8 / W) * RS::kSliceBytes + d * RS::kSliceBytes) / RS::kSliceBytes]++;
        for (int h : hit) errors += h != 1;
    }
    errors += RS::kSlotBytes > 8 * 72 * 16;
    int barriers = 0, issues = 0;
    for (int b = 0; b < RS::kBarriersPerRow; b++) barriers++, issues += RS::issues_at(b);
    errors += barriers != 3 || issues != 4;

    for (int L = 1; L <= 4; L++)
        for (int W : {4, 8})
            for (long n : {1L, 2L, 3L, 630L}) {
                const std::string e = check(good, L, W, n);
                cases++;
                if (!e.empty()) errors++, std::fprintf(stderr, "l=%d W=%d n=%ld: %s\n", L, W, n, e.c_str());
            }

    // broken schedules the checker must reject
    int rejected = 0, broken = 0;
    auto must_fail = [&](const char *what, Sched s) {
        broken++;
        bool all = true;
        for (int W : {4, 8}) all &= !check(s, 3, W, 3).empty();
        if (all) rejected++;
        else std::fprintf(stderr, "accepted a broken schedule: %s\n", what);
    };
    { Sched s = good; s.vm[RS::kBarA] = 1; must_fail("A certifies one chunk too few", s); }
    { Sched s = good; s.vm[RS::kBarX] = 1; must_fail("X does not wait for the borrowed chunk", s); }
    { Sched s = good; s.vm[RS::kBarB] = 0; must_fail("B drains the refills", s); }
    { Sched s = good; s.plan[3].issue_barrier = RS::kBarX; must_fail("borrowed chunk issued at X and read after X", s); }
    { Sched s = good; s.plan[3].certify_barrier = RS::kBarA; must_fail("borrowed chunk read in the phase it is issued in", s); }
    { Sched s = good; s.plan[0].issue_barrier = RS::kBarA; must_fail("slot 0 refilled while it is read", s); }
    { Sched s = good; s.plan[3].slot = 2; must_fail("fourth chunk into a resident slot that is being read", s); }
    { Sched s = good; s.plan[2].slot = RS::kBorrowedSlot; s.plan[3].slot = 2; must_fail("borrowed slot written outside A .. B", s); }
    { Sched s = good; s.prologue = 2; must_fail("prologue one chunk short", s); }
    errors += rejected != broken;

    std::printf("{\"cases\": %d, \"errors\": %d, \"broken\": %d, \"rejected\": %d, \"barriers_per_row\": %d, \"issues_per_row\": %d}\n", cases, errors, broken, rejected, barriers, issues);
    return errors ? 1 : 0;
}
