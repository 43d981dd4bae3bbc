// geometry.h — the sizes and build switches that the kernels and the host's route rules (search_plan.h) both read: tiles, waves,
// storage dtypes, queries per work item.  No HIP in here: plain C++17, so that search_plan.h compiles with a host compiler alone.
// Each name is documented where its kernels live (the header named behind it).
#pragma once
#include <stdint.h>

namespace codd {

// wave_topk.h
constexpr int kWave = 64;

// row_traits.h
constexpr int DT_F32 = 0;   // == CODD_KNN_DTYPE_F32
constexpr int DT_BF16 = 1;  // == CODD_KNN_DTYPE_BF16
constexpr int DT_F16 = 2;   // == CODD_KNN_DTYPE_F16

// exact_score.h: NITER = kWideRows selects the wide form of an exact-score body
constexpr int kWideRows = 0;

// filter_gemm.h
#ifndef CODD_SHADOW_F16
#define CODD_SHADOW_F16 1    // the 2-byte shadow's element type: 1 = fp16 (11-bit significand: eps 0.0011 at 768-d), 0 = bf16 (8 bits: eps 0.0079).
                             // Same MFMA rate, same bytes; fp16 since round 3: this filter is what an index falls back to when the int8 one (eps ~0.02)
                             // cannot separate a query's neighbourhood from the rest of a dense cluster, and there a 7x tighter slack is worth more than
                             // anything else (profiles/r3/clustered_corpora.txt).  Unit-norm operands cannot overflow fp16; its subnormal grid is in the bound.
#endif
#ifndef CODD_MFMA16
#define CODD_MFMA16 1        // 1: v_mfma_f32_16x16x32_bf16 (16-row x 16-query blocks, K 32) instead of 32x32x16
#endif
constexpr int kTileRows = 256;
constexpr int kTileQ = 256;

// filter_i8.h: does the resident program apply? (nbq: 32-query blocks of the batch: 8 -> NQB = 16, 4 -> NQB = 8)
constexpr bool i8_tile_resident(int nsteps, int nbq) { return nsteps <= (nbq == 8 ? 4 : 8); }

// filter_i8.h (the tile programs' cursors) and search_plan.h (cascade_plan): the run-tiles that are NO multiple of d + 1, shared out
// between `grid` workgroups when d divides the grid.  The m-th such tile is m + 1 + m / d, so workgroup b's tiles b + j grid are
// skip_first(b, d) + j skip_step(grid, d).  One definition for the kernel and for the plan the CPU tests walk.
template <typename T>
constexpr T skip_first(T b, T d) { return b + 1 + b / d; }
template <typename T>
constexpr T skip_step(T grid, T d) { return grid + grid / d; }

// filter_i8.h: the six-interval tile programs' plan — which K-step an interval computes, from which LDS slot, which
// query slice its head stages, which corpus step its loads request, and the wave's vector-memory issue order, from which every
// counted s_waitcnt vmcnt of those programs is derived (tests/host/sweep_plan_main.cpp walks it with a model of the slots and of
// the in-order queue).  sweep = false is the static program: every tile walks K-steps 0..5 and stages all six slices, two
// intervals ahead of their use.  sweep = true: a tile stages two.  Tiles of even ordinal walk K-steps 0 2 4 5 1 3, tiles of odd
// ordinal (`back`) 1 3 4 5 0 2: the two slices a tile ends on are the two the next one starts on, slices 4 and 5 never leave
// their slots, and the heads of intervals 2 and 3 stage the slices of intervals 4 and 5 over those of intervals 0 and 1.  Both
// walks are step(i) = fwd(i) + back * sign(i) with sign = +1, +1, 0, 0, -1, -1: ONE program whose direction is a number added to
// three addresses, with the same slot, the same issue order and the same waits either way.
// early: the CODD_I8_EARLY_A mask (bit 0: the corpus loads of interval 2 go out in the tail of interval 1; bit 1: those of 4 in the
// tail of 3).  dps: DMA instructions per wave and slice.
constexpr int kSweepSteps = 6;
constexpr int kSweepCorpusOps = 4;   // vector-memory instructions of one corpus step's fragments (kAPerIv)
constexpr int sweep_fwd(int i) { return i < 3 ? 2 * i : (i == 3 ? 5 : 2 * i - 7); }          // 0 2 4 5 1 3
constexpr int sweep_sign(int i) { return i < 2 ? 1 : (i < 4 ? 0 : -1); }
constexpr int sweep_step(bool back, int i) { return sweep_fwd(i) + (back ? sweep_sign(i) : 0); }   // the K-step interval i computes
constexpr int sweep_slot(int step) { return step < 4 ? step >> 1 : step - 2; }                    // ... and the LDS slot its slice lives in: {0,1} {2,3} {4} {5}
// the slice staged in the head of interval i (-1: none) and its slot
constexpr int sweep_stage(bool sweep, bool back, int i) {
    if (!sweep) return (i + 2) % kSweepSteps;
    return (i == 2 || i == 3) ? sweep_step(back, i + 2) : -1;
}
constexpr int sweep_stage_slot(bool sweep, bool back, int i) { return sweep ? sweep_slot(sweep_stage(sweep, back, i)) : (i + 2) & 3; }
// the loads "of interval i" fetch the fragments interval i + 2 computes: a step of this tile, or (i >= 4) of the next one, which
// walks the other way
constexpr bool sweep_load_next_tile(int i) { return i + 2 >= kSweepSteps; }
constexpr int sweep_load_step(bool sweep, bool back, int i) {
    if (!sweep) return (i + 2) % kSweepSteps;
    return sweep_load_next_tile(i) ? sweep_step(!back, i + 2 - kSweepSteps) : sweep_step(back, i + 2);
}
// the slices the prologue stages, by slot: what a forward tile's first four intervals read
constexpr int sweep_prologue_slice(int slot) { return sweep_fwd(slot); }
constexpr bool sweep_early(int early, int i) { return i >= 2 && i < kSweepSteps && i % 2 == 0 && (early & (i % 4 == 2 ? 1 : 2)) != 0; }
// Issue order of interval i: head = [block metadata (i == 0)] [dps slice DMA (a slice is staged)] [4 corpus loads unless early],
// the wait for the fragments of interval i, its MFMAs, tail = [the 4 corpus loads of interval i + 1 when those are early], and
// behind an odd interval the barrier.  Both directions stage in the same intervals, so the order does not depend on `back`.
constexpr int sweep_head_dma(bool sweep, int i, int dps) { return (i == 0 ? 1 : 0) + (sweep_stage(sweep, false, i) >= 0 ? dps : 0); }
constexpr int sweep_head_ops(bool sweep, int i, int dps, int early) { return sweep_head_dma(sweep, i, dps) + (sweep_early(early, i) ? 0 : kSweepCorpusOps); }
constexpr int sweep_tail_ops(int i, int early) { return sweep_early(early, i + 1) ? kSweepCorpusOps : 0; }
// One walk over two tiles' worth of intervals (the order is periodic in the tile) up to the head (at_barrier = false) or the
// tail (true) of interval i of the second one.  Returns the operations issued behind the last corpus load of interval i - 2
// (at_barrier = false: the vmcnt of the wait in front of interval i's MFMAs) or behind the last DMA — slice or metadata — issued so
// far (true: the vmcnt in front of the barrier that hands the landed slices over).
constexpr int sweep_vm_walk(bool sweep, int i, int dps, int early, bool at_barrier) {
    int pos = 0, after_wanted = 0, after_dma = 0;
    const int end = kSweepSteps + i, wanted = end - 2;
    for (int a = 0; a <= end; ++a) {
        const int j = a % kSweepSteps;
        const int dma = sweep_head_dma(sweep, j, dps);
        pos += dma;
        if (dma) after_dma = pos;
        if (!sweep_early(early, j)) {
            pos += kSweepCorpusOps;
            if (a == wanted) after_wanted = pos;
        }
        if (a == end && !at_barrier) break;
        if (sweep_tail_ops(j, early)) {
            pos += kSweepCorpusOps;
            if (a + 1 == wanted) after_wanted = pos;
        }
    }
    return pos - (at_barrier ? after_dma : after_wanted);
}
constexpr int sweep_vm_corpus_wait(bool sweep, int i, int dps, int early) { return sweep_vm_walk(sweep, i, dps, early, false); }
constexpr int sweep_vm_barrier_wait(bool sweep, int i, int dps, int early) { return sweep_vm_walk(sweep, i, dps, early, true); }

// list_scan_kernels.h
constexpr int kIvfNB = 4;  // queries per work item
// queries per work item: four, as in ivf_scan_shared_kernel; two for 2-byte rows of 4 chunks per lane (four queries' registers would spill)
constexpr int scope_nb(int dt, int niter) { return (dt != DT_F32 && niter == 4) ? 2 : 4; }

}  // namespace codd
