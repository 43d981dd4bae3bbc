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

// list_scan_kernels.h
constexpr int kIvfNB = 4;  // queries per work item
// queries per work item: four, as in ivf_scan_shared_kernel; two for 2-byte rows of 4 chunks per lane (four queries' registers would spill)
constexpr int scope_nb(int dt, int niter) { return (dt != DT_F32 && niter == 4) ? 2 : 4; }

}  // namespace codd
