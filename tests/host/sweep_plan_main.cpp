// The six-interval tile programs' plan (csrc/geometry.h: sweep_*) walked by a model of one wave: the four LDS slots of the query
// block, the three register slots of the corpus ring and the in-order vector-memory queue.  Plain C++17, no HIP.
//
//   sweep_plan_main <sweep 0|1> <tiles of the workgroup> <early mask> <dps> [<bug> <where>]
//
// bug 0: the plan as it is.  1: the slot rule off by one (slot + 1 mod 4) for K-step <where>.  2: the corpus wait of interval <where>
// one operation too lax.  3: ... one too strict.  4: the barrier wait of interval <where> one too lax.
// Prints "ok <slices staged in the prologue> <slices staged per tile> <tiles>" and exits 0, or "FAIL <what>" and exits 1.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "geometry.h"

using namespace codd;

namespace {

struct Op {
    int kind;      // 0 block metadata, 1 slice DMA, 2 corpus load
    int slot;      // LDS slot (1) or ring slot (2)
    int tile, step;
    bool retired = false;
};

struct Model {
    bool sweep;
    int tiles, early, dps, bug, where;
    std::vector<Op> q;
    size_t head = 0;   // first operation not retired
    // LDS slots: the slice a slot holds once handed over by a barrier (-1: nothing yet), the slice on its way
    int held[4] = {-1, -1, -1, -1}, landing[4] = {-1, -1, -1, -1};
    bool read_in_span[4] = {false, false, false, false}, written_in_span[4] = {false, false, false, false};
    // ring slots: what was requested into them, whether it was consumed
    int ring_tile[3] = {-1, -1, -1}, ring_step[3] = {-1, -1, -1};
    size_t ring_op[3] = {0, 0, 0};
    bool ring_used[3] = {true, true, true};
    int staged_prologue = 0, staged_tile = 0;

    [[noreturn]] void fail(const char* what, int o, int i) {
        printf("FAIL %s (tile %d interval %d)\n", what, o, i);
        exit(1);
    }
    bool back(int o) const { return sweep && (o & 1); }
    int step_of(int o, int i) const { return sweep ? sweep_step(back(o), i) : i; }
    int slot_of(int o, int i, int step) const {
        int s = sweep ? sweep_slot(step) : (kSweepSteps * o + i) & 3;
        if (bug == 1 && step == where) s = (s + 1) & 3;
        return s;
    }
    void issue(Op op) { q.push_back(op); }
    size_t outstanding() const { return q.size() - head; }
    void wait(int n) {
        while (outstanding() > (size_t)n) q[head++].retired = true;
    }
    void dma_slice(int slot, int slice, int o, int i) {
        if (read_in_span[slot]) fail("a slot is overwritten before the barrier that follows its last read", o, i);
        written_in_span[slot] = true;
        held[slot] = -1;
        landing[slot] = slice;
        for (int j = 0; j < dps; ++j) issue({1, slot, o, slice});
    }
    void corpus(int ring, int tile, int step, int o, int i) {
        if (!ring_used[ring]) fail("a ring slot is requested again before its fragments were consumed", o, i);
        ring_tile[ring] = tile;
        ring_step[ring] = step;
        ring_used[ring] = false;
        for (int j = 0; j < kSweepCorpusOps; ++j) issue({2, ring, tile, step});
        ring_op[ring] = q.size() - 1;
    }
    void barrier(int o, int i) {
        // what this wave's wait has retired is handed over; the waves are symmetric, so every wave's share has landed
        for (int s = 0; s < 4; ++s) {
            if (landing[s] >= 0) {
                bool all = true;
                for (const Op& op : q)
                    if (op.kind == 1 && op.slot == s && !op.retired) all = false;
                if (all) { held[s] = landing[s]; landing[s] = -1; }
            }
            if (read_in_span[s] && written_in_span[s]) fail("a slot is read and written between two barriers", o, i);
            read_in_span[s] = written_in_span[s] = false;
        }
    }
    // operations younger than the last one of `kind_mask` kinds
    int younger_than_last_dma() const {
        int n = 0;
        for (size_t j = q.size(); j-- > 0;) {
            if (q[j].kind != 2) return n;
            ++n;
        }
        return n;
    }

    void run() {
        // prologue: metadata, the first slices, two corpus steps, everything waited for, barrier
        issue({0, 0, 0, 0});
        const int first = sweep ? 4 : 2;
        for (int s = 0; s < first; ++s) {
            const int slice = sweep ? sweep_prologue_slice(s) : s;
            dma_slice(slot_of(0, s, slice), slice, 0, -1);
            ++staged_prologue;
        }
        corpus(0, 0, step_of(0, 0), 0, -1);
        corpus(1, 0, step_of(0, 1), 0, -1);
        wait(0);
        barrier(0, -1);
        for (int o = 0; o < tiles; ++o) {
            bool seen[kSweepSteps] = {};
            int staged = 0;
            for (int i = 0; i < kSweepSteps; ++i) {
                const int step = step_of(o, i), slot = slot_of(o, i, step);
                // head
                if (i == 0) issue({0, 0, o, 0});
                const int st = sweep_stage(sweep, back(o), i);
                if (st >= 0) {
                    const int dst = sweep ? slot_of(o, i + 2, st) : (kSweepSteps * o + i + 2) & 3;
                    if (sweep && dst != ((sweep_stage_slot(sweep, back(o), i) + (bug == 1 && st == where ? 1 : 0)) & 3)) fail("the staging slot is not the slice's slot", o, i);
                    dma_slice(dst, st, o, i);
                    ++staged;
                }
                auto load = [&](int iv) {
                    const bool next = sweep_load_next_tile(iv);
                    const int lt = next ? o + 1 : o, lstep = sweep_load_step(sweep, back(o), iv);
                    corpus((iv + 2) % 3, lt, lstep, o, iv);
                };
                if (!sweep_early(early, i)) load(i);
                if ((int)outstanding() != 0 && sweep_head_ops(sweep, i, dps, early) != (i == 0 ? 1 : 0) + (st >= 0 ? dps : 0) + (sweep_early(early, i) ? 0 : kSweepCorpusOps))
                    fail("sweep_head_ops disagrees with the issue order", o, i);
                // the wait for this interval's fragments
                int w = sweep_vm_corpus_wait(sweep, i, dps, early);
                if (bug == 2 && i == where) w += 1;
                if (bug == 3 && i == where) w -= 1;
                const int ring = i % 3;
                const int younger = (int)(q.size() - 1 - ring_op[ring]);
                // (the first tile's intervals 0 and 1 consume what the prologue waited for with vmcnt(0): nothing to compare)
                if (!(o == 0 && i < 2) && w != younger) fail("a corpus wait differs from the model's count of younger operations", o, i);
                wait(w < 0 ? 0 : w);
                if (!q[ring_op[ring]].retired) fail("fragments are consumed before they have landed", o, i);
                if (ring_tile[ring] != o || ring_step[ring] != step) fail("the ring slot holds another step's fragments", o, i);
                ring_used[ring] = true;
                // the MFMAs read the slice
                if (held[slot] != step) fail("a computed step reads a slot that does not hold its slice, landed by the preceding barrier", o, i);
                read_in_span[slot] = true;
                if (seen[step]) fail("a K-step is computed twice", o, i);
                seen[step] = true;
                // tail
                if (sweep_tail_ops(i, early)) load(i + 1);
                if (i & 1) {
                    int wb = sweep_vm_barrier_wait(sweep, i, dps, early);
                    if (bug == 4 && i == where) wb += 1;
                    if (wb != younger_than_last_dma() + (bug == 4 && i == where ? 1 : 0)) fail("a barrier wait differs from the model's count of operations younger than the last DMA", o, i);
                    wait(wb);
                    barrier(o, i);
                }
            }
            for (int s = 0; s < kSweepSteps; ++s)
                if (!seen[s]) fail("a K-step is missing", o, kSweepSteps);
            if (o == 0) staged_tile = staged;
            else if (staged != staged_tile) fail("tiles stage different numbers of slices", o, kSweepSteps);
        }
        wait(0);
        printf("ok %d %d %d\n", staged_prologue, staged_tile, tiles);
    }
};

}  // namespace

int main(int argc, char** argv) {
    if (argc < 5) return 2;
    Model m;
    m.sweep = atoi(argv[1]) != 0;
    m.tiles = atoi(argv[2]);
    m.early = atoi(argv[3]);
    m.dps = atoi(argv[4]);
    m.bug = argc > 5 ? atoi(argv[5]) : 0;
    m.where = argc > 6 ? atoi(argv[6]) : 0;
    m.run();
    return 0;
}
