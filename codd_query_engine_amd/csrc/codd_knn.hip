// codd_knn.hip — HIP kernels (gfx950 / CDNA4, wave64) and the C ABI of include/codd_knn.h.
//
// What runs here is the arithmetic half of ChromaDB on Codd's search_relevant_metrics path
// (reference call sites: codd_dal/metrics/metrics_semantic_metadata_store.py:60-69 create,
// :236-238 upsert, :314-316 query; scoring :336).  Kernels:
//
//   normalize_rows_kernel   ingest + query prep: c <- c/|c| (canonical sum of squares, IEEE sqrt/div),
//                           writes the stored row AND its bf16 shadow in MFMA-fragment order
//   prep_queries_kernel     one launch per batch of <= 256 queries: normalise, pack the MFMA fragments,
//                           clear the pass's control block
//   scan_topk_kernel        exact streaming scan (small batches, fallback): one wave owns 4 rows per
//                           step, 16-B/lane coalesced loads, fmaf chains in canonical order,
//                           wave-distributed top-k lists
//   merge_keys_kernel       integer top-k of packed keys (per-block partials, shard partials)
//   raw_rows_kernel         ingest + query prep of an ip or l2 index: vectors as given, non-finite ones as zeros
//   scan_topk_l2, scan_topk_wide_l2, scope_scan_l2, mask_scan_l2, merge_keys_l2
//                           the squared-L2 forms of the exact-score kernels; ip runs the dot-product ones
//   filter_gemm.h           large batches: bf16 MFMA filter + exact fp32 re-score (finalize)
//
// HBM-bound byte streaming throughout: the corpus is read once per pass, each row by exactly one
// wave, straight into registers; results leave as 8-byte keys.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <atomic>
#include <mutex>
#include <new>
#include <type_traits>
#include <vector>

#include "codd_knn.h"
#include "device_mem.h"

#ifndef CODD_EXPERIMENTS
#define CODD_EXPERIMENTS 0  // 1 (build_variant only): the diagnostic switches that can return wrong results exist
#endif
#include "doc_match.h"
#include "exact_score.h"
#include "filter_gemm.h"
#include "filter_i8.h"
#include "row_traits.h"
#include "text_embed.h"
#include "wave_topk.h"

using namespace codd;

// =============================================================================================
// device code
// =============================================================================================

namespace {

// ---------------------------------------------------------------------------------------------
// normalize_rows_kernel: one wave per input vector.  in: n x d fp32 (row stride d).
// out row = slots ? slots[r] : first_slot + r, width dpad, storage dtype DT.
// Sum of squares in the canonical order with E = 4 (the input is fp32), then IEEE sqrt and
// IEEE division per element; a zero / non-finite norm stores an all-zero row.
// shadow (optional): the bf16 rounding of the STORED value, in fragment order (filter_gemm.h).
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float butterfly_max(float v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, kWave));
    return v;
}
// |x| of one vector by the canonical sum of squares: chunk j of 4 elements belongs to lane j % 64
//
// The squares are taken in fp32, so a vector of finite elements can have a sum of squares that underflows (elements near 1e-23
// and below: the few bits left of a subnormal sum put the stored norm at 0.8 .. 1.2, or at 0) or overflows (elements near 1e18
// and above).  Cosine does not depend on scale: where the sum leaves [2^-100, 2^100] the vector is scaled by the exact power of
// two `sh` that brings its largest magnitude into [1, 2) and the same chain runs on the scaled values; the caller divides
// scaled(x[i], sh) by the returned norm.  Inside the band (every ordinary vector) sh = 0 and nothing changes.  The branch is
// wave-uniform: butterfly_sum and butterfly_max leave the same value in every lane.
// Returns 0 for a vector with a non-finite element or without a non-zero one (the callers' zero row).
constexpr float kNormBandLo = 0x1p-100f, kNormBandHi = 0x1p+100f;
__device__ __forceinline__ float scaled(float t, int sh) { return sh ? __builtin_ldexpf(t, sh) : t; }
// floor(log2 m) of a finite m > 0 from its bits, subnormals included
__device__ __forceinline__ int floor_log2_f32(float m) {
    const uint32_t u = __float_as_uint(m) & 0x7fffffffu;
    const int e = (int)(u >> 23);
    return e ? e - 127 : (31 - __builtin_clz(u)) - 149;
}
__device__ __forceinline__ float canonical_norm(const float* __restrict__ x, int d, int nch, int lane, int& sh) {
    sh = 0;
    float acc = 0.0f;
    for (int j = lane; j < nch; j += kWave) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int i = j * 4 + e;
            const float v = i < d ? x[i] : 0.0f;
            acc = __builtin_fmaf(v, v, acc);
        }
    }
    float n2 = butterfly_sum(acc);
    if (!(n2 >= kNormBandLo && n2 <= kNormBandHi)) {
        float m = 0.0f;
        for (int j = lane; j < nch; j += kWave) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int i = j * 4 + e;
                m = fmaxf(m, fabsf(i < d ? x[i] : 0.0f));
            }
        }
        m = butterfly_max(m);
        // a NaN element makes n2 NaN (fmaxf would skip it); an infinite one makes m infinite
        if (n2 != n2 || !(m > 0.0f) || !(m < INFINITY)) return 0.0f;
        sh = -floor_log2_f32(m);
        acc = 0.0f;
        for (int j = lane; j < nch; j += kWave) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int i = j * 4 + e;
                const float v = i < d ? __builtin_ldexpf(x[i], sh) : 0.0f;
                acc = __builtin_fmaf(v, v, acc);
            }
        }
        n2 = butterfly_sum(acc);
    }
    return __builtin_sqrtf(n2);
}

// Query preparation of one filter pass in ONE launch (B <= 256): q <- q/|q| exactly as normalize_rows_kernel<f32> does
// (qn, for finalize's exact re-scoring), the same values rounded into the MFMA fragment order (qfrag; queries >= B
// are zero), and the pass's control block cleared.  One wave per query slot, 64 blocks.
__global__ __launch_bounds__(256) void prep_queries_kernel(const float* __restrict__ in, int B, int d, int dpad, float* __restrict__ qn,
                                                           uint2* __restrict__ qfrag, unsigned* __restrict__ ctl, int ctl_words) {
    const int lane = lane_id();
    const int q = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    for (int i = (int)blockIdx.x * 256 + (int)threadIdx.x; i < ctl_words; i += (int)gridDim.x * 256) ctl[i] = 0u;
    const int nch = dpad >> 2;
    if (q >= B) {
        for (int j = lane; j < nch; j += kWave) qfrag[codd::qfrag_piece_index(q, j >> 1) * 2 + (j & 1)] = make_uint2(0u, 0u);
        return;
    }
    const float* x = in + (int64_t)q * d;
    int sh;
    const float nrm = canonical_norm(x, d, nch, lane, sh);
    const bool zero_row = !(nrm > 0.0f) || !(nrm < INFINITY);
    for (int j = lane; j < nch; j += kWave) {
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int i = j * 4 + e;
            const float t = i < d ? x[i] : 0.0f;
            v[e] = zero_row ? 0.0f : scaled(t, sh) / nrm;
        }
        reinterpret_cast<float4*>(qn)[(int64_t)q * nch + j] = make_float4(v[0], v[1], v[2], v[3]);
        qfrag[codd::qfrag_piece_index(q, j >> 1) * 2 + (j & 1)] = make_uint2(codd::pack_bf16x2(v[0], v[1]), codd::pack_bf16x2(v[2], v[3]));
    }
}

template <int DT>
__global__ __launch_bounds__(256) void normalize_rows_kernel(const float* __restrict__ in, int64_t n, int d, int dpad,
                                                             int normalize, const int64_t* __restrict__ slots,
                                                             int64_t first_slot, void* __restrict__ out_,
                                                             uint2* __restrict__ shadow) {
    const int lane = lane_id();
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= n) return;
    const float* x = in + r * (int64_t)d;
    const int nch = dpad >> 2;
    const int nsteps = dpad >> 6;
    float scale_div = 1.0f;
    int sh = 0;
    bool zero_row = false;
    if (normalize) {
        const float nrm = canonical_norm(x, d, nch, lane, sh);
        zero_row = !(nrm > 0.0f) || !(nrm < INFINITY);
        scale_div = nrm;
    }
    const int64_t orow = slots ? slots[r] : first_slot + r;
    for (int j = lane; j < nch; j += kWave) {
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int i = j * 4 + e;
            float t = i < d ? x[i] : 0.0f;
            if (normalize) t = zero_row ? 0.0f : scaled(t, sh) / scale_div;
            v[e] = t;
        }
        if (DT == DT_F32) {
            float4* o = reinterpret_cast<float4*>(out_) + orow * (int64_t)nch + j;
            *o = make_float4(v[0], v[1], v[2], v[3]);
        } else {
            uint16_t hb[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                hb[e] = DT == DT_BF16 ? f32_to_bf16_rne(v[e]) : f32_to_f16_rne(v[e]);
                // the shadow approximates the STORED value, whatever the shadow element type is
                v[e] = DT == DT_F16 ? f16_bits_to_f32(hb[e]) : __uint_as_float((uint32_t)hb[e] << 16);
            }
            uint2* o = reinterpret_cast<uint2*>(out_) + orow * (int64_t)nch + j;
            *o = make_uint2((uint32_t)hb[0] | ((uint32_t)hb[1] << 16), (uint32_t)hb[2] | ((uint32_t)hb[3] << 16));
        }
        if (shadow) {
            // elements [4j, 4j+4) = half (j&1) of 16-byte piece c8 = j>>1
            const int64_t piece = shadow_piece_index(orow, j >> 1, nsteps);
            shadow[piece * 2 + (j & 1)] = make_uint2(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]));
        }
    }
}

// raw_rows_kernel: ingest and query prep of an ip or l2 index, one wave per input vector: the vector is used as
// given — padded with zeros to dpad, rounded to the storage dtype DT, not normalised — except that a vector with a NaN or infinite
// element, or without a non-zero one, is stored as zeros.  out row = slots ? slots[r] : first_slot + r, as normalize_rows_kernel.
template <int DT>
__global__ __launch_bounds__(256) void raw_rows_kernel(const float* __restrict__ in, int64_t n, int d, int dpad, const int64_t* __restrict__ slots,
                                                       int64_t first_slot, void* __restrict__ out_) {
    const int lane = lane_id();
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= n) return;
    const float* x = in + r * (int64_t)d;
    const int nch = dpad >> 2;
    bool bad = false, any = false;
    for (int i = lane; i < d; i += kWave) {
        const float v = x[i];
        bad = bad || !(fabsf(v) < INFINITY);   // (NaN compares false too)
        any = any || v != 0.0f;
    }
    const bool zero_row = __ballot(bad) != 0ull || __ballot(any) == 0ull;
    const int64_t orow = slots ? slots[r] : first_slot + r;
    for (int j = lane; j < nch; j += kWave) {
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int i = j * 4 + e;
            v[e] = (i < d && !zero_row) ? x[i] : 0.0f;
        }
        if (DT == DT_F32) {
            reinterpret_cast<float4*>(out_)[orow * (int64_t)nch + j] = make_float4(v[0], v[1], v[2], v[3]);
        } else {
            uint16_t hb[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) hb[e] = DT == DT_BF16 ? f32_to_bf16_rne(v[e]) : f32_to_f16_rne(v[e]);
            reinterpret_cast<uint2*>(out_)[orow * (int64_t)nch + j] = make_uint2((uint32_t)hb[0] | ((uint32_t)hb[1] << 16), (uint32_t)hb[2] | ((uint32_t)hb[3] << 16));
        }
    }
}

// shadow_from_rows_kernel: rebuild the bf16 fragment-order shadow of rows [first, first+n) from the
// stored rows themselves (index load from disk: the rows arrive already normalised and rounded).
template <int DT>
__global__ __launch_bounds__(256) void shadow_from_rows_kernel(const void* __restrict__ rows_, int64_t first, int64_t n, int dpad,
                                                               uint2* __restrict__ shadow) {
    const int lane = lane_id();
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= n) return;
    const int64_t row = first + r;
    const int nch = dpad >> 2, nsteps = dpad >> 6;
    for (int j = lane; j < nch; j += kWave) {
        float v[4];
        if (DT == DT_F32) {
            const float4 x = reinterpret_cast<const float4*>(rows_)[row * (int64_t)nch + j];
            v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
        } else {
            const uint2 x = reinterpret_cast<const uint2*>(rows_)[row * (int64_t)nch + j];
            const uint16_t hb[4] = {(uint16_t)(x.x & 0xffffu), (uint16_t)(x.x >> 16), (uint16_t)(x.y & 0xffffu), (uint16_t)(x.y >> 16)};
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = DT == DT_BF16 ? __uint_as_float((uint32_t)hb[e] << 16) : f16_bits_to_f32(hb[e]);
        }
        const int64_t piece = shadow_piece_index(row, j >> 1, nsteps);
        shadow[piece * 2 + (j & 1)] = make_uint2(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]));
    }
}

// ---------------------------------------------------------------------------------------------
// scan_topk_kernel<DT, NB, NITER, SLOTS>: exact canonical-score scan of the whole row store for
// up to NB queries at once.
//   - a wave owns row group g = 4 consecutive rows per step; NITER 16-byte loads per row per lane
//     (chunk j = lane + 64*it), i.e. 4*NITER loads in flight per lane before the first use;
//   - the NB query fragments live in registers for the whole kernel;
//   - per (row, query): one fmaf chain per lane in canonical order, then the 4-row butterfly;
//   - per (wave, query): a top-k list distributed over the lanes (wave_topk.h);
//   - per block: the 4 wave lists are merged through LDS and written as k packed keys to
//     partial[q][block][0..k).
// ---------------------------------------------------------------------------------------------
// scan_topk_body: the scan as a workgroup of NW waves sees it — workgroup `bid` of `nblocks`, lds = NW * NB * SLOTS * 64 u64.
// `total` queries, dense from qn (qlist == nullptr) or listed (qlist[i] = query slot; `listed` also selects the one-launch
// hand-off to the last block, see below).  Shared by scan_topk_kernel and by the scan role of finalize_fb_kernel.
// the tombstone bits of row group g (rows 4g .. 4g+3: one bitmap word, 4 | 32) in bits 0..3; 0 without a load while nothing was ever
// deleted.  g is wave-uniform: said so to the compiler, the word is a scalar load into a scalar register, not one more vector register
// in a loop that lives at the register limit.
__device__ __forceinline__ uint32_t group_dead_bits(const uint32_t* __restrict__ dead, int64_t g) {
    if (!dead) return 0u;
    const uint32_t gu = (uint32_t)__builtin_amdgcn_readfirstlane((int)g);
    return dead[gu >> 3] >> ((gu & 7u) * 4u);
}

template <int DT, int NB, int NITER, int SLOTS, int NW, int METRIC = kMetricDot>
__device__ __forceinline__ void scan_topk_body(const void* __restrict__ rows_, int64_t n, int dpad, const float* __restrict__ qn, int total, int k,
                                               uint32_t row_base, u64* __restrict__ partial, int64_t partial_stride_q,
                                               const unsigned* __restrict__ qlist, bool listed, unsigned* __restrict__ merge_done,
                                               u64* __restrict__ merged_keys, float* __restrict__ merged_dist, int64_t* __restrict__ merged_rows,
                                               unsigned long long* __restrict__ count_total, int bid, int nblocks, u64* __restrict__ lds,
                                               const uint32_t* __restrict__ dead) {
    typedef RowTraits<DT> RT;
    constexpr int E = RT::E;
    const int lane = lane_id();
    const int wave = (int)(threadIdx.x >> 6);
    const int nchunks = dpad / E;

    // Two ways in: (a) the host names a dense group of nq_arg <= NB queries starting at qn (one pass);
    // (b) LISTED: qcount_ptr / qlist live on the device (the filter's fallback queue) and the kernel walks
    // the queue NB queries at a time — zero queued queries is the common case and costs one empty launch.
    for (int g0 = 0; g0 < total; g0 += NB) {
    const int nq = total - g0 < NB ? total - g0 : NB;

    WaveTopK<SLOTS> L[NB];
    if constexpr (NITER == kWideRows) {
        // wide rows: the group's queries in LDS (where the block merge keeps its lists: the previous group is done with them),
        // every row group walked segment by segment (wide_segment)
        float* qs = reinterpret_cast<float*>(lds);
        const int qstride = wide_qfloats(nchunks, E);
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            const float* src = b < nq ? qn + (qlist ? (int64_t)qlist[g0 + b] : (int64_t)(g0 + b)) * dpad : nullptr;
            wide_stage_query(qs + b * qstride, src, dpad, qstride, (int)threadIdx.x, NW * kWave);
        }
        __syncthreads();
#pragma unroll
        for (int b = 0; b < NB; ++b) L[b].init();
        const uint4* base = reinterpret_cast<const uint4*>(rows_);
        const int64_t ngroups = (n + 3) >> 2;
        const int64_t W = (int64_t)nblocks * NW;
        const int nseg = wide_nseg(nchunks);
        for (int64_t g = (int64_t)bid * NW + wave; g < ngroups; g += W) {
            const uint4* p[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t row = g * 4 + r < n ? g * 4 + r : n - 1;
                p[r] = base + row * (int64_t)nchunks + lane;
            }
            float acc[NB][4];
#pragma unroll
            for (int b = 0; b < NB; ++b)
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[b][r] = 0.0f;
            for (int s = 0; s < nseg; ++s) wide_segment<DT, NB, 4, METRIC>(p, s, nchunks, lane, qs, qstride, acc);
            const uint32_t dm = group_dead_bits(dead, g);
#pragma unroll
            for (int b = 0; b < NB; ++b) {   // (one query's tail and offers at a time: NB x 4 scores at once spill scalar registers)
                const float y = packed4<METRIC>(acc[b], lane);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int64_t row = g * 4 + r;
                    if (row < n && !((dm >> r) & 1u)) L[b].offer(make_key(packed_score(y, r), row_base + (uint32_t)row), k, lane);
                }
            }
        }
        __syncthreads();  // every wave is done with the queries: the lists take their place
    } else {
    float qf[NB][NITER][E];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        load_query_frags(b < nq ? qn + (qlist ? (int64_t)qlist[g0 + b] : (int64_t)(g0 + b)) * dpad : nullptr, nchunks, lane, qf[b]);
        L[b].init();
    }

    const uint4* base = reinterpret_cast<const uint4*>(rows_);
    const int64_t ngroups = (n + 3) >> 2;
    const int64_t W = (int64_t)nblocks * NW;
    for (int64_t g = (int64_t)bid * NW + wave; g < ngroups; g += W) {
        const uint4* p[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) p[r] = base + (g * 4 + r < n ? g * 4 + r : n - 1) * (int64_t)nchunks + lane;
        float w[4][NITER][E];
        fetch4_widened<DT>(p, nchunks, lane, w);
        const uint32_t dm = group_dead_bits(dead, g);
#pragma unroll
        for (int b = 0; b < NB; ++b) {   // (an absent query's fragments are zeros: its list is never read)
            const float y = score4_one<NITER, E, METRIC>(w, qf[b], lane);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t row = g * 4 + r;
                if (row < n && !((dm >> r) & 1u)) L[b].offer(make_key(packed_score(y, r), row_base + (uint32_t)row), k, lane);
            }
        }
    }
    }  // (NITER)

    // block merge through LDS: wave b collects query b's list
#pragma unroll
    for (int b = 0; b < NB; ++b) store_list(lds, wave, NB, b, lane, L[b]);
    __syncthreads();
    for (int b = wave; b < nq; b += NW) {
        WaveTopK<SLOTS> M;
        M.init();
        merge_lists(M, lds, 0, NW, NB, b, k, lane);
        write_keys(M, k, lane, partial + (int64_t)(g0 + b) * partial_stride_q + (int64_t)bid * k);
    }
    __syncthreads();  // the LDS lists are rewritten by the next group
    }  // group loop

    // LISTED mode with `merge_done`: the block that finishes last merges every queued query's per-block partials and writes
    // the answers into the queries' own slots — the fallback is ONE launch (an empty queue, the normal case, costs one
    // empty launch and touches no counter).  Hand-off: every block's stores, a device-scope fence, the arrival ticket;
    // the last arriver fences again before it reads the other blocks' partials.
    if (listed && merge_done && total > 0) {
        __shared__ unsigned s_last;
        __threadfence();
        __syncthreads();
        if (threadIdx.x == 0) s_last = atomicAdd(merge_done, 1u) == (unsigned)nblocks - 1u ? 1u : 0u;
        __syncthreads();
        if (!s_last) return;
        __threadfence();
        if (threadIdx.x == 0) *merge_done = 0u;  // (ready for the next list-driven launch without a clearing pass)
        if (threadIdx.x == 0 && count_total) atomicAdd(count_total, (unsigned long long)total);
        const int64_t m = (int64_t)nblocks * k;
        for (int qi = wave; qi < total; qi += NW) {
            const u64* src = partial + (int64_t)qi * partial_stride_q;
            WaveTopK<SLOTS> M;
            M.init();
            for (int64_t i0 = 0; i0 < m; i0 += kWave) {
                const int64_t i = i0 + lane;
                M.offer_lanes(i < m ? src[i] : 0ull, k, lane);
            }
            const int64_t o = (int64_t)qlist[qi] * k;
            write_ranks<SLOTS, METRIC>(M, k, lane, merged_keys ? merged_keys + o : nullptr, merged_dist ? merged_dist + o : nullptr, merged_rows ? merged_rows + o : nullptr);
        }
    }
}

template <int DT, int NB, int NITER, int SLOTS>
__global__ __launch_bounds__(256) void scan_topk_kernel(const void* __restrict__ rows_, int64_t n, int dpad,
                                                        const float* __restrict__ qn, int nq_arg, int k,
                                                        uint32_t row_base, u64* __restrict__ partial,
                                                        int64_t partial_stride_q, const unsigned* __restrict__ qlist,
                                                        const unsigned* __restrict__ qcount_ptr, unsigned* __restrict__ merge_done = nullptr,
                                                        u64* __restrict__ merged_keys = nullptr, float* __restrict__ merged_dist = nullptr,
                                                        int64_t* __restrict__ merged_rows = nullptr,
                                                        unsigned long long* __restrict__ count_total = nullptr,
                                                        const uint32_t* __restrict__ dead = nullptr) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int total = qcount_ptr ? (int)*qcount_ptr : nq_arg;
    scan_topk_body<DT, NB, NITER, SLOTS, 4>(rows_, n, dpad, qn, total, k, row_base, partial, partial_stride_q, qlist, qcount_ptr != nullptr, merge_done, merged_keys,
                                            merged_dist, merged_rows, count_total, (int)blockIdx.x, (int)gridDim.x, reinterpret_cast<u64*>(smem_raw), dead);
}

// scan_topk_kernel's wide form (more than 4 chunks per lane): the NB queries' full rows are staged in LDS, up to 128 KiB, so ONE
// workgroup of 8 waves per compute unit shares them (2 waves per SIMD, 8 row groups per LDS copy of the queries)
constexpr int kWideScanWaves = 8;
template <int DT, int NB, int SLOTS>
__global__ __launch_bounds__(kWideScanWaves * kWave) void scan_topk_wide_kernel(const void* __restrict__ rows_, int64_t n, int dpad,
                                                                                const float* __restrict__ qn, int nq_arg, int k,
                                                                                uint32_t row_base, u64* __restrict__ partial,
                                                                                int64_t partial_stride_q, const unsigned* __restrict__ qlist,
                                                                                const unsigned* __restrict__ qcount_ptr, unsigned* __restrict__ merge_done,
                                                                                u64* __restrict__ merged_keys, float* __restrict__ merged_dist,
                                                                                int64_t* __restrict__ merged_rows, unsigned long long* __restrict__ count_total,
                                                                                const uint32_t* __restrict__ dead) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int total = qcount_ptr ? (int)*qcount_ptr : nq_arg;
    scan_topk_body<DT, NB, kWideRows, SLOTS, kWideScanWaves>(rows_, n, dpad, qn, total, k, row_base, partial, partial_stride_q, qlist, qcount_ptr != nullptr,
                                                             merge_done, merged_keys, merged_dist, merged_rows, count_total, (int)blockIdx.x, (int)gridDim.x,
                                                             reinterpret_cast<u64*>(smem_raw), dead);
}

// The squared-L2 scans: scan_topk_body under kMetricL2, dense queries only (an l2 index takes no filter leg, so
// the list-driven fallback forms are not built).  Kernels of their own, so that every dot-product kernel stays the code it was.
template <int DT, int NB, int NITER, int SLOTS>
__global__ __launch_bounds__(256) void scan_topk_l2(const void* __restrict__ rows_, int64_t n, int dpad, const float* __restrict__ qn, int nq, int k,
                                                    uint32_t row_base, u64* __restrict__ partial, int64_t partial_stride_q,
                                                    const uint32_t* __restrict__ dead) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    scan_topk_body<DT, NB, NITER, SLOTS, 4, kMetricL2>(rows_, n, dpad, qn, nq, k, row_base, partial, partial_stride_q, nullptr, false, nullptr, nullptr, nullptr,
                                                       nullptr, nullptr, (int)blockIdx.x, (int)gridDim.x, reinterpret_cast<u64*>(smem_raw), dead);
}
template <int DT, int NB, int SLOTS>
__global__ __launch_bounds__(kWideScanWaves * kWave) void scan_topk_wide_l2(const void* __restrict__ rows_, int64_t n, int dpad, const float* __restrict__ qn,
                                                                            int nq, int k, uint32_t row_base, u64* __restrict__ partial,
                                                                            int64_t partial_stride_q, const uint32_t* __restrict__ dead) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    scan_topk_body<DT, NB, kWideRows, SLOTS, kWideScanWaves, kMetricL2>(rows_, n, dpad, qn, nq, k, row_base, partial, partial_stride_q, nullptr, false, nullptr,
                                                                        nullptr, nullptr, nullptr, nullptr, (int)blockIdx.x, (int)gridDim.x,
                                                                        reinterpret_cast<u64*>(smem_raw), dead);
}

// The list-driven squared-distance scan: the exact-scan fallback of an l2 index's filter pass, for the queries
// whose candidate lists were truncated.  scan_topk_body under kMetricL2 walking the device-side queue four queries at a time
// (the role is rare), its last block merging; rows of 1 .. 4 chunks per lane.  A kernel of its own: the dense scans above stay
// the instantiations they were.
template <int DT, int NITER, int SLOTS>
__global__ __launch_bounds__(256) void sqd_listed_scan_kernel(const void* __restrict__ rows_, int64_t n, int dpad, const float* __restrict__ qn, int k,
                                                              uint32_t row_base, u64* __restrict__ partial, int64_t partial_stride_q,
                                                              const unsigned* __restrict__ qlist, const unsigned* __restrict__ qcount_ptr,
                                                              unsigned* __restrict__ merge_done, u64* __restrict__ merged_keys,
                                                              float* __restrict__ merged_dist, int64_t* __restrict__ merged_rows,
                                                              unsigned long long* __restrict__ count_total, const uint32_t* __restrict__ dead) {
    static_assert(NITER != kWideRows, "the squared-distance filter leg serves rows of 1 .. 4 chunks per lane");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    scan_topk_body<DT, 4, NITER, SLOTS, 4, kMetricL2>(rows_, n, dpad, qn, (int)*qcount_ptr, k, row_base, partial, partial_stride_q, qlist, true, merge_done,
                                                      merged_keys, merged_dist, merged_rows, count_total, (int)blockIdx.x, (int)gridDim.x,
                                                      reinterpret_cast<u64*>(smem_raw), dead);
}

// ---------------------------------------------------------------------------------------------
// finalize_fb_kernel: finalize and the exact-scan fallback of a filter pass in ONE launch (round 3: the fallback used to be a
// launch of its own behind finalize — normally empty, still 4 us + a dependent-launch gap of ~10 us on every step).
//   workgroups x < nq  : finalize_kernel's work for query x (share blockIdx.y of its candidates);
//   workgroups x >= nq : the exact scan over the queries whose candidate lists were truncated (hit_cnt > cap_q).  They need
//     nothing from the finalize workgroups: each derives the queue from the counters itself (same order in every workgroup)
//     and leaves at once when it is empty — the normal case.  Otherwise: scan_topk_body over the queue, the last scan
//     workgroup to finish merges the per-workgroup partials and writes the answers into the queries' slots.
// k <= 64 only (one list slot per lane); wider k keeps the two launches.
// ---------------------------------------------------------------------------------------------
template <int DT, int NITER>
__global__ __launch_bounds__(kFinThreads) void finalize_fb_kernel(const void* __restrict__ rows_, int dpad, const float* __restrict__ qn, const u64* __restrict__ hits,
                                                                   const unsigned* __restrict__ hit_cnt, int cap_q, unsigned* __restrict__ flags, int k, float two_eps,
                                                                   uint32_t row_base, u64* __restrict__ out_keys, unsigned long long* __restrict__ stats,
                                                                   const float* __restrict__ two_eps_q, u64* __restrict__ part_keys, float* __restrict__ out_dist,
                                                                   int64_t* __restrict__ out_rows, const float2* __restrict__ bmeta, int nq, int64_t n,
                                                                   u64* __restrict__ fb_partial, int64_t fb_stride_q, unsigned* __restrict__ fb_done,
                                                                   const uint32_t* __restrict__ dead) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    constexpr int kWavesHere = kFinThreads / kWave;
    if ((int)blockIdx.x < nq) {
        const int q = blockIdx.x;
        const unsigned total = hit_cnt[q * kHitCntStride];
        const unsigned part = blockIdx.y, nparts = gridDim.y;
        if (total > (unsigned)cap_q) {  // the candidate list was truncated: the scan workgroups answer this query
            if (threadIdx.x == 0 && part == 0) atomicOr(&flags[FLAG_NEED_FALLBACK], 1u);
            return;
        }
        const float eps1 = bmeta ? two_eps_q[256 + q] : 0.5f * (two_eps_q ? two_eps_q[q] : two_eps);
        const float bq = bmeta ? two_eps_q[512 + q] : 0.0f;
        finalize_body<DT, NITER, 1>(rows_, dpad, qn + (int64_t)q * dpad, hits + (int64_t)q * cap_q, total, part, nparts, k, eps1, bq, bmeta, row_base,
                                    out_keys ? out_keys + (int64_t)q * k : nullptr, out_dist ? out_dist + (int64_t)q * k : nullptr,
                                    out_rows ? out_rows + (int64_t)q * k : nullptr, part_keys ? part_keys + ((int64_t)q * nparts + part) * k : nullptr, stats, dead);
        return;
    }
    if (blockIdx.y != 0) return;
    // the queue: queries with a truncated list, in query order (every scan workgroup computes the same list)
    __shared__ unsigned s_fb[kTileQ];
    __shared__ unsigned s_cnt[kWavesHere + 1];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool over = tid < nq && hit_cnt[tid * kHitCntStride] > (unsigned)cap_q;   // (nq <= 256 < kFinThreads)
    const u64 mask = __ballot(over);
    if (lane == 0) s_cnt[wave] = (unsigned)__popcll(mask);
    __syncthreads();
    unsigned base = 0, total = 0;
    for (int w = 0; w < kWavesHere; ++w) {
        if (w < wave) base += s_cnt[w];
        total += s_cnt[w];
    }
    if (total == 0) return;   // (uniform: nothing was truncated — the normal case)
    if (over) s_fb[base + (unsigned)__popcll(mask & ((1ull << lane) - 1ull))] = (unsigned)tid;
    __syncthreads();
    // (4 queries per pass over the rows, not 8: the role is rare, and its query registers must not push the finalize role into scratch)
    scan_topk_body<DT, 4, NITER, 1, kWavesHere>(rows_, n, dpad, qn, (int)total, k, row_base, fb_partial, fb_stride_q, s_fb, true, fb_done, out_keys, out_dist, out_rows,
                                                 stats ? stats + 2 : nullptr, (int)blockIdx.x - nq, (int)gridDim.x - nq, reinterpret_cast<u64*>(smem_raw), dead);
}

// ---------------------------------------------------------------------------------------------
// merge_keys_kernel: block b reduces in[b][0..m) to its k largest keys (descending) and writes
// keys and/or (distance, row).  Used for the per-block partials of a scan, for the all-gathered
// shard partials, and (m == k) to unpack final keys.
// ---------------------------------------------------------------------------------------------
template <int SLOTS, int METRIC>
__device__ __forceinline__ void merge_keys_body(const u64* __restrict__ in, int64_t m, int64_t in_stride, int64_t seg_len,
                                                int64_t seg_stride, int k, u64* __restrict__ out_keys, float* __restrict__ out_dist,
                                                int64_t* __restrict__ out_rows, const unsigned* __restrict__ out_list,
                                                const unsigned* __restrict__ count_ptr,
                                                unsigned long long* __restrict__ count_total) {
    const int lane = lane_id();
    const int wave = (int)(threadIdx.x >> 6);
    // LISTED (fallback queue): only the first *count_ptr blocks work, block i answers query out_list[i]
    if (count_ptr) {
        const unsigned cnt = *count_ptr;
        if (blockIdx.x == 0 && threadIdx.x == 0 && count_total && cnt) atomicAdd(count_total, (unsigned long long)cnt);
        if (blockIdx.x >= cnt) return;
    }
    const int64_t oblock = out_list ? (int64_t)out_list[blockIdx.x] : (int64_t)blockIdx.x;
    const u64* src = in + (int64_t)blockIdx.x * in_stride;
    WaveTopK<SLOTS> L;
    L.init();
    for (int64_t i0 = (int64_t)wave * kWave; i0 < m; i0 += 256) {
        const int64_t i = i0 + lane;
        // a query's m keys are m / seg_len runs of seg_len keys, seg_stride apart (one run when seg_len == m;
        // one run per shard when the input is an all_gather of [B][k] partials)
        const u64 cand = i < m ? src[(i / seg_len) * seg_stride + (i % seg_len)] : 0ull;
        L.offer_lanes(cand, k, lane);
    }
    __shared__ u64 lds[4 * SLOTS * kWave];
    store_list(lds, wave, 1, 0, lane, L);
    __syncthreads();
    if (wave != 0) return;
    merge_lists(L, lds, 1, 4, 1, 0, k, lane);
    const int64_t o = oblock * k;
    write_ranks<SLOTS, METRIC>(L, k, lane, out_keys ? out_keys + o : nullptr, out_dist ? out_dist + o : nullptr, out_rows ? out_rows + o : nullptr);
}
template <int SLOTS>
__global__ __launch_bounds__(256) void merge_keys_kernel(const u64* __restrict__ in, int64_t m, int64_t in_stride, int64_t seg_len,
                                                         int64_t seg_stride, int k, u64* __restrict__ out_keys, float* __restrict__ out_dist,
                                                         int64_t* __restrict__ out_rows, const unsigned* __restrict__ out_list,
                                                         const unsigned* __restrict__ count_ptr,
                                                         unsigned long long* __restrict__ count_total) {
    merge_keys_body<SLOTS, kMetricDot>(in, m, in_stride, seg_len, seg_stride, k, out_keys, out_dist, out_rows, out_list, count_ptr, count_total);
}
// the same merge for keys of squared-L2 scores: the distance written is 0 - score
template <int SLOTS>
__global__ __launch_bounds__(256) void merge_keys_l2(const u64* __restrict__ in, int64_t m, int64_t in_stride, int64_t seg_len, int64_t seg_stride, int k,
                                                     u64* __restrict__ out_keys, float* __restrict__ out_dist, int64_t* __restrict__ out_rows) {
    merge_keys_body<SLOTS, kMetricL2>(in, m, in_stride, seg_len, seg_stride, k, out_keys, out_dist, out_rows, nullptr, nullptr, nullptr);
}

// ---------------------------------------------------------------------------------------------
// IVF (coarse lists + exact scores), SURVEY.md §8(f)4 / BASELINE config 5.
// gather_rows_kernel: rows_ivf[i] = rows[perm[i]] (rows regrouped by coarse list), one wave per row.
// widen_rows_kernel : stored rows -> fp32 [n][dim] (index build reads the corpus back through it).
// ivf_scan_kernel   : block (x, b) scans slice x%split of the list that query b probes at rank x/split,
//                     canonical exact scores, per-wave top-k, keys carry the ORIGINAL row slot.
// ---------------------------------------------------------------------------------------------
// perm_check_kernel: sets *bad when any perm[i] lies outside [0, n) (codd_knn_ivf_install trusts no caller-built table:
// gather_rows_kernel and ivf_scan_kernel index rows with these values)
__global__ __launch_bounds__(256) void perm_check_kernel(const int64_t* __restrict__ perm, int64_t n, unsigned* __restrict__ bad) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n && (perm[i] < 0 || perm[i] >= n)) atomicOr(bad, 1u);
}

__global__ __launch_bounds__(256) void gather_rows_kernel(const uint4* __restrict__ src, const int64_t* __restrict__ perm, int64_t n,
                                                          int chunks_per_row, uint4* __restrict__ dst, uint32_t* __restrict__ ids) {
    const int lane = lane_id();
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= n) return;
    const int64_t from = perm[r];
    for (int j = lane; j < chunks_per_row; j += kWave) dst[r * chunks_per_row + j] = src[from * chunks_per_row + j];
    if (lane == 0) ids[r] = (uint32_t)from;
}

// ---------------------------------------------------------------------------------------------------------------
// int8 shadow (half the bytes of the bf16 shadow).  Row r is stored as round(c_i / scale_b), scale_b = the largest |c_i| of
// its 32-row block / 127 (rscale[] holds it once per row), in the same fragment order as the bf16 shadow with 16-element pieces and 128-element K-steps.  The
// filter's error bound needs |c - c~| for the worst row: every wave folds its row's error norm into *eps_r (ordered bits).
// ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t quantize4(const float (&v)[4], float inv_scale, float scale, float& err2) {
    uint32_t packed = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        float t = __builtin_rintf(v[e] * inv_scale);
        t = fminf(fmaxf(t, -127.0f), 127.0f);
        const float d = v[e] - t * scale;
        err2 = __builtin_fmaf(d, d, err2);
        packed |= ((uint32_t)(int)t & 0xffu) << (8 * e);
    }
    return packed;
}
// One workgroup quantises one 32-row corpus block (a wave's rows in the filter GEMMs) with ONE scale for the whole block:
// max |c_i| over its 32 rows / 127.  (Round 1 scaled every row by its own maximum.  A scale that is uniform inside a block
// lets the filter's epilogue test accumulators against an integer threshold before any conversion; the price, a coarser
// grid for rows whose own maximum is smaller, is in the measured error norm *eps_r like every other quantisation error.)
// Pass 1 finds the block maximum, pass 2 quantises the block in two halves of 16 rows (4 rows per wave), collects each half in
// LDS and writes its pieces out in fragment order: 16 consecutive lanes = the 16 rows of one piece column = 256 contiguous
// bytes (a wave per row writing its own 16-byte pieces, 256 bytes apart, ran at a tenth of the HBM rate).
template <int DT>
__global__ __launch_bounds__(256) void shadow8_from_rows_kernel(const void* __restrict__ rows_, int64_t first32, int64_t n, int dpad, int dpad8,
                                                                uint4* __restrict__ shadow8, float* __restrict__ rscale,
                                                                float2* __restrict__ bmeta) {
    constexpr int kRowDwords = 516;  // 512 + 4: sixteen rows read column-wise hit 64 different banks
    __shared__ __attribute__((aligned(16))) uint32_t tile[16 * kRowDwords];
    __shared__ float s_max[4];
    __shared__ float s_err[4];
    const int lane = lane_id(), wave = (int)(threadIdx.x >> 6);
    const int64_t row32 = first32 + (int64_t)blockIdx.x * 32;
    const int nch = dpad >> 2, nch8 = dpad8 >> 2, nsteps8 = dpad8 >> 7;
    const int nit = (nch8 + kWave - 1) / kWave;  // chunks of 4 elements per lane and row
    // chunk j = lane + 64 * it of a row (zeros past the row's end and for rows past n)
    auto load_chunk = [&](int64_t row, int it, float (&v)[4]) __attribute__((always_inline)) {
        const int j = lane + kWave * it;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = 0.0f;
        if (j < nch && row < n) {
            if (DT == DT_F32) {
                const float4 x = reinterpret_cast<const float4*>(rows_)[row * (int64_t)nch + j];
                v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
            } else {
                const uint2 x = reinterpret_cast<const uint2*>(rows_)[row * (int64_t)nch + j];
                const uint16_t hb[4] = {(uint16_t)(x.x & 0xffffu), (uint16_t)(x.x >> 16), (uint16_t)(x.y & 0xffffu), (uint16_t)(x.y >> 16)};
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = DT == DT_BF16 ? __uint_as_float((uint32_t)hb[e] << 16) : f16_bits_to_f32(hb[e]);
            }
        }
    };
    // pass 1: the block's largest magnitude.  Chunk-major, the wave's 8 rows inside: eight independent loads in flight per
    // lane (row-major with one row at a time, the kernel was a chain of HBM round trips: 26 ms for 10M x 768 rows)
    float vmax = 0.0f;
    for (int it = 0; it < nit; ++it) {
        float v[8][4];
#pragma unroll
        for (int rr = 0; rr < 8; ++rr) load_chunk(row32 + wave * 8 + rr, it, v[rr]);
#pragma unroll
        for (int rr = 0; rr < 8; ++rr)
#pragma unroll
            for (int e = 0; e < 4; ++e) vmax = fmaxf(vmax, fabsf(v[rr][e]));
    }
    vmax = butterfly_max(vmax);
    if (lane == 0) s_max[wave] = vmax;
    __syncthreads();
    vmax = fmaxf(fmaxf(s_max[0], s_max[1]), fmaxf(s_max[2], s_max[3]));
    const float scale = vmax > 0.0f ? vmax / 127.0f : 1.0f, inv_scale = 1.0f / scale;
    // pass 2: quantise (the rows come from L2 this time), 16 rows at a time, 4 rows per wave; rows wider than the tile (2,048
    // elements) in column slices of kTileDwords dwords.  The scale above and each row's error norm below span the WHOLE row.
    constexpr int kTileDwords = 512;
    float wave_err = 0.0f;  // largest error norm among this wave's rows
    for (int half = 0; half < 2; ++half) {
        const int64_t row16 = row32 + 16 * half;
        float err2[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        for (int c0 = 0; c0 < nch8; c0 += kTileDwords) {
            const int it1 = (c0 + kTileDwords) / kWave < nit ? (c0 + kTileDwords) / kWave : nit;
            for (int it = c0 / kWave; it < it1; ++it) {
                float v[4][4];
#pragma unroll
                for (int rr = 0; rr < 4; ++rr) load_chunk(row16 + wave * 4 + rr, it, v[rr]);
                const int j = lane + kWave * it;
#pragma unroll
                for (int rr = 0; rr < 4; ++rr)
                    if (j < nch8) tile[(wave * 4 + rr) * kRowDwords + (j - c0)] = quantize4(v[rr], inv_scale, scale, err2[rr]);  // (rows past n, chunks past the row: zeros)
            }
            __syncthreads();
            // piece (c16, r) of the half block: 16 bytes of row r at byte 16*c16 (c16 counted from the slice's first piece)
            const int npieces = (nch8 - c0 < kTileDwords ? nch8 - c0 : kTileDwords) >> 2;
            for (int p = (int)threadIdx.x; p < 16 * npieces; p += 256) {
                const int r = p & 15, c16 = p >> 4;
                shadow8[codd::shadow_piece_index(row16 + r, (c0 >> 2) + c16, nsteps8)] = *reinterpret_cast<const uint4*>(&tile[r * kRowDwords + c16 * 4]);
            }
            __syncthreads();
        }
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            const int64_t row = row16 + wave * 4 + rr;
            const float e2 = butterfly_sum(err2[rr]);
            if (row < n) {
                if (lane == 0) rscale[row] = scale;
                wave_err = fmaxf(wave_err, __builtin_sqrtf(e2) * 1.0001f + 1e-7f);  // inflated a little: the norm itself was accumulated in fp32
            }
        }
    }
    // The block's meta data: its scale and the largest quantisation error norm |c - c~| among its rows.  The filter's bound is
    // evaluated PER BLOCK with this norm (round 2 folded every row's norm into one device-wide maximum that could only grow: one
    // badly quantising row widened every query's slack for the life of the index); the device-wide maximum that the
    // first-generation kernels and the host's "is int8 usable at all" test still use is re-derived from these after every
    // build (eps_max_kernel), so it follows the rows that are stored NOW.
    if (lane == 0) s_err[wave] = wave_err;
    __syncthreads();
    if (threadIdx.x == 0 && row32 < n) bmeta[row32 >> 5] = make_float2(scale, fmaxf(fmaxf(s_err[0], s_err[1]), fmaxf(s_err[2], s_err[3])));
}

// eps_max_kernel: *eps_r_bits = the largest block error norm over blocks [0, nblocks) (one workgroup; after every shadow build)
// eps_r_bits[1] = how many blocks lie above `wide` (the host's "int8 bound useless" level): the per-block kernels only pay for those blocks
__global__ __launch_bounds__(1024) void eps_max_kernel(const float2* __restrict__ bmeta, int64_t nblocks, unsigned* __restrict__ eps_r_bits, float wide) {
    __shared__ float s_part[16];
    __shared__ unsigned s_wide;
    if (threadIdx.x == 0) s_wide = 0u;
    __syncthreads();
    float m = 0.0f;
    unsigned nw = 0;
    for (int64_t i = threadIdx.x; i < nblocks; i += 1024) {
        const float e = bmeta[i].y;
        m = fmaxf(m, e);
        nw += e > wide ? 1u : 0u;
    }
    m = butterfly_max(m);
    if (nw) atomicAdd(&s_wide, nw);
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 16; ++w) m = fmaxf(m, s_part[w]);
        eps_r_bits[0] = __float_as_uint(m);
        eps_r_bits[1] = s_wide;
    }
}

// prep_queries_kernel for the int8 filter: qn as always; the query quantised like a row (qfrag8, scale in qmeta[q]);
// qmeta[256 + q] = 2 * eps(q) with eps(q) = |q - q~| (1.01 + eps_r) + 1.001 eps_r + 2e-6 >= |<q~, c~> - <q, c>| for every
// stored row c (|c| <= 1.004 whatever the storage type, |c - c~| <= eps_r, |q| <= 1 + 1e-6; the integer accumulation
// is exact and the two scale multiplications cost < 4e-7)
__global__ __launch_bounds__(256) void prep_queries8_kernel(const float* __restrict__ in, int B, int d, int dpad, int dpad8,
                                                            float* __restrict__ qn, uint32_t* __restrict__ qfrag8, float* __restrict__ qmeta,
                                                            const unsigned* __restrict__ eps_r_bits, unsigned* __restrict__ ctl, int ctl_words,
                                                            float slack_scale) {
    const int lane = lane_id();
    const int q = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    for (int i = (int)blockIdx.x * 256 + (int)threadIdx.x; i < ctl_words; i += (int)gridDim.x * 256) ctl[i] = 0u;
    const int nch = dpad >> 2, nch8 = dpad8 >> 2;
    if (q >= B) {
        for (int j = lane; j < nch8; j += kWave) qfrag8[codd::qfrag_piece_index(q, j >> 2) * 4 + (j & 3)] = 0u;
        if (lane == 0) { qmeta[q] = 0.0f; qmeta[256 + q] = 0.0f; qmeta[512 + q] = 0.0f; qmeta[768 + q] = 0.0f; }
        return;
    }
    const float* x = in + (int64_t)q * d;
    int sh;
    const float nrm = canonical_norm(x, d, nch, lane, sh);
    const bool zero_row = !(nrm > 0.0f) || !(nrm < INFINITY);
    float vmax = 0.0f;
    for (int j = lane; j < nch; j += kWave) {
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int i = j * 4 + e;
            const float t = i < d ? x[i] : 0.0f;
            v[e] = zero_row ? 0.0f : scaled(t, sh) / nrm;
            vmax = fmaxf(vmax, fabsf(v[e]));
        }
        reinterpret_cast<float4*>(qn)[(int64_t)q * nch + j] = make_float4(v[0], v[1], v[2], v[3]);
    }
    vmax = butterfly_max(vmax);
    const float scale = vmax > 0.0f ? vmax / 127.0f : 0.0f, inv_scale = vmax > 0.0f ? 127.0f / vmax : 0.0f;
    float err2 = 0.0f;
    for (int j = lane; j < nch8; j += kWave) {
        float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (j < nch) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int i = j * 4 + e;
                const float t = i < d ? x[i] : 0.0f;
                v[e] = zero_row ? 0.0f : scaled(t, sh) / nrm;
            }
        }
        qfrag8[codd::qfrag_piece_index(q, j >> 2) * 4 + (j & 3)] = quantize4(v, inv_scale, scale, err2);
    }
    err2 = butterfly_sum(err2);
    if (lane == 0) {
        const float eq = __builtin_sqrtf(err2) * 1.0001f + 1e-7f, er = __uint_as_float(*eps_r_bits);
        qmeta[q] = scale;
        qmeta[256 + q] = slack_scale * 2.0f * (eq * (1.01f + er) + 1.001f * er + 2e-6f);
        // the same bound split by what it depends on: eps(q, block) = A(q) + B(q) * e_block, e_block = the block's own error norm
        // (bmeta[].y) in place of the device-wide maximum er — what i8_tile_kernel and finalize evaluate per 32-row block
        qmeta[512 + q] = slack_scale * (eq * 1.01f + 2e-6f);
        qmeta[768 + q] = slack_scale * (eq + 1.001f);
    }
}

// ---------------------------------------------------------------------------------------------------------------
// The int8 filter leg of an ip or l2 index ("space_filter"): rows and queries of ANY norm, so the two constants
// above that stand for |c| and |q| of unit vectors become measured quantities.
// row_sqnorm_kernel<DT>: one wave per stored row of [first, first + m): rnorm2[row] = the canonical sum of squares of the row AS
// STORED (DESIGN.md §3's chain over chunks of RowTraits<DT>::E elements, the butterfly, + 0.0f), and *rmax_bits = max(*rmax_bits,
// R(row)) with R(row) = sqrt(rnorm2) * 1.0001 + 1e-7 >= |c|_2: the chain and the root are off by < 2e-5 relative, squares that
// underflow by < sqrt(dpad) 2^-63 absolute.  The bits of a non-negative float order like the float; a sum that overflowed (or a
// row that is not a number) leaves +inf there, and every query of the index is then answered by the exact re-score of all rows.
// ---------------------------------------------------------------------------------------------------------------
template <int DT>
__global__ __launch_bounds__(256) void row_sqnorm_kernel(const void* __restrict__ rows_, int64_t first, int64_t m, int dpad, float* __restrict__ rnorm2,
                                                         unsigned* __restrict__ rmax_bits) {
    typedef RowTraits<DT> RT;
    constexpr int E = RT::E;
    const int lane = lane_id();
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= m) return;
    const int64_t row = first + r;
    const int nchunks = dpad / E;
    const uint4* p = reinterpret_cast<const uint4*>(rows_) + row * (int64_t)nchunks;
    float a = 0.0f;
    for (int j = lane; j < nchunks; j += kWave) {
        float w[E];
        RT::widen(p[j], w);
#pragma unroll
        for (int e = 0; e < E; ++e) a = __builtin_fmaf(w[e], w[e], a);
    }
    const float n2 = butterfly_sum(a);
    if (lane == 0) {
        rnorm2[row] = n2;
        float R = __builtin_sqrtf(n2) * 1.0001f + 1e-7f;
        if (!(R < INFINITY)) R = INFINITY;
        atomicMax(rmax_bits, __float_as_uint(R));
    }
}

// prep_queries8_raw_kernel: prep_queries8_kernel for an ip (l2 = 0) or l2 (l2 = 1) index.  qn = the query as raw_rows_kernel<f32>
// cleans it (what the exact kernels consume); qfrag8 / qmeta[q]: the same vector quantised with its own scale s_q; qmeta[512 + q]
// = n_q, its canonical sum of squares; qmeta[256 + q] = 2 eps(q) with, for every stored row c (DESIGN.md §21 derives both),
//   e_q = |q - q~| measured, + 2^-23 Q for the fp32 rounding of the measurement, e_r likewise from the rows' measured *eps_r_bits,
//   Q >= |q|, R = *rmax_bits >= |c|, m = dpad / 64 the length of a lane's chain, u = 2^-24:
//   ip: eps = e_q (R + e_r) + Q e_r + (m + 9) u (Q + e_q)(R + e_r)               >= |acc s_blk s_q - score(q, c)|
//   l2: eps = 2 (e_q (R + e_r) + Q e_r) + (2 m + 18) u (Q + R + e_q + e_r)^2     >= |fma(acc s_blk, 2 s_q, -rnorm2) - n_q - score(q, c)|
// every term rounded upward; +inf when R or Q is not finite or the product term leaves [2^-100, 2^100] (the threshold is then
// -inf, every row a hit, and the exact re-score or the overflow fallback answers the query).
__global__ __launch_bounds__(256) void prep_queries8_raw_kernel(const float* __restrict__ in, int B, int d, int dpad, int dpad8, float* __restrict__ qn,
                                                                uint32_t* __restrict__ qfrag8, float* __restrict__ qmeta,
                                                                const unsigned* __restrict__ eps_r_bits, const unsigned* __restrict__ rmax_bits,
                                                                unsigned* __restrict__ ctl, int ctl_words, int l2) {
    const int lane = lane_id();
    const int q = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    for (int i = (int)blockIdx.x * 256 + (int)threadIdx.x; i < ctl_words; i += (int)gridDim.x * 256) ctl[i] = 0u;
    const int nch = dpad >> 2, nch8 = dpad8 >> 2;
    if (q >= B) {
        for (int j = lane; j < nch8; j += kWave) qfrag8[codd::qfrag_piece_index(q, j >> 2) * 4 + (j & 3)] = 0u;
        if (lane == 0) { qmeta[q] = 0.0f; qmeta[256 + q] = 0.0f; qmeta[512 + q] = 0.0f; qmeta[768 + q] = 0.0f; }
        return;
    }
    const float* x = in + (int64_t)q * d;
    bool bad = false, any = false;
    for (int i = lane; i < d; i += kWave) {
        const float v = x[i];
        bad = bad || !(fabsf(v) < INFINITY);   // (NaN compares false too)
        any = any || v != 0.0f;
    }
    const bool zero_row = __ballot(bad) != 0ull || __ballot(any) == 0ull;
    float vmax = 0.0f, a2 = 0.0f;
    for (int j = lane; j < nch; j += kWave) {
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int i = j * 4 + e;
            v[e] = (i < d && !zero_row) ? x[i] : 0.0f;
            vmax = fmaxf(vmax, fabsf(v[e]));
            a2 = __builtin_fmaf(v[e], v[e], a2);
        }
        reinterpret_cast<float4*>(qn)[(int64_t)q * nch + j] = make_float4(v[0], v[1], v[2], v[3]);
    }
    vmax = butterfly_max(vmax);
    const float nq2 = butterfly_sum(a2);
    const float scale = vmax > 0.0f ? vmax / 127.0f : 0.0f, inv_scale = vmax > 0.0f ? 127.0f / vmax : 0.0f;
    float err2 = 0.0f;
    for (int j = lane; j < nch8; j += kWave) {
        float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (j < nch) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int i = j * 4 + e;
                v[e] = (i < d && !zero_row) ? x[i] : 0.0f;
            }
        }
        qfrag8[codd::qfrag_piece_index(q, j >> 2) * 4 + (j & 3)] = quantize4(v, inv_scale, scale, err2);
    }
    err2 = butterfly_sum(err2);
    if (lane == 0) {
        constexpr float up = 1.0001f, u = 5.9604645e-8f, u2 = 1.1920929e-7f;   // 2^-24, 2^-23
        const float m = (float)(dpad >> 6);
        const float R = __uint_as_float(*rmax_bits);
        const float Q = __builtin_sqrtf(nq2) * up + 1e-7f;
        const float eq = __builtin_sqrtf(err2) * up + u2 * Q + 1e-7f;
        const float er = __uint_as_float(*eps_r_bits) * up + u2 * R;
        const float a = (Q + eq) * up, b = (R + er) * up;
        const float quant = (eq * b + Q * er * up) * up;
        float eps, range;
        if (l2) {
            const float s = (a + b) * up;
            range = s * s;
            eps = (2.0f * quant + (2.0f * m + 18.0f) * u * 1.001f * range) * up + 1e-30f;
        } else {
            range = a * b;
            eps = (quant + (m + 9.0f) * u * 1.001f * range) * up + 1e-30f;
        }
        if (!(range >= kNormBandLo && range <= kNormBandHi) || !(eps < INFINITY)) eps = INFINITY;
        qmeta[q] = scale;
        qmeta[256 + q] = 2.0f * eps;
        qmeta[512 + q] = nq2;
        qmeta[768 + q] = Q;
    }
}

// codd_knn_filter_slack: out[q] = eps(q) of the device-wide bound, from the 2 eps(q) a preparation kernel left at two_eps_q[q]
__global__ __launch_bounds__(256) void filter_slack_kernel(const float* __restrict__ two_eps_q, int B, float* __restrict__ out) {
    const int q = (int)threadIdx.x;
    if (q < B) out[q] = 0.5f * two_eps_q[q];
}

// ---------------------------------------------------------------------------------------------------------------
// small_batch_kernel<DT, NITER, NS>: ONE query answered in ONE launch (BASELINE configs[1]: 1M x 768, B = 1).  The filter chain
// of a batch is six dependent launches (query preparation, sample, thresholds, filter, finalize, merge); at B = 1 over 1M rows
// they cost as much again as streaming the int8 shadow once.  Here:
//   every workgroup : wave 0 quantises the query (same arithmetic as prep_queries8_kernel) into LDS while the other waves' first
//     loads are already in flight; then every wave streams its share of the int8 shadow — 16 rows x dpad8 bytes at a time
//     (2 NS contiguous 1-KiB chunks of the fragment order, the next unit's loads issued before this unit's arithmetic);
//     lane (kq, r) holds 16 elements of row r: v_dot4 against the query's 16 bytes from LDS, two cross-lane adds — keeps
//     its best 64 approximate scores (WaveTopK) and publishes the best kSbKeep of them plus `dropmax`, the best key it did NOT
//     publish (0: none);
//   the workgroup that finishes LAST (device-scope fence + arrival ticket) : finalize_body over the published candidates — the
//     k best approximate ones re-scored exactly give L' <= s_k, every row whose approximate score is >= L' - eps(q) is
//     re-scored exactly (canonical fp32 expression), top-k written.  MARGIN TEST: if some wave's dropmax is >= L' - eps(q) a
//     candidate may have been dropped: the query goes to the exact-scan fallback queue (the list-driven scan launch behind
//     this kernel: normally empty).  No thresholds, no sample pass: the bound is the same eps(q) = |q - q~| (1.01 + eps_r) +
//     1.001 eps_r + 2e-6 as the int8 filter's (device-wide eps_r).
// Results are bit-identical to every other path: the survivors' scores are the canonical ones.
// ---------------------------------------------------------------------------------------------------------------
#if !CODD_EXPERIMENTS && (defined(CODD_SB_EXP_NOOFFER) || defined(CODD_SB_EXP_NOSTREAM) || defined(CODD_SB_EXP_NOFINAL))
#error "the CODD_SB_EXP_* switches return wrong results: they exist only in -DCODD_EXPERIMENTS=1 builds (build_variant)"
#endif
constexpr int kSbKeep = 8;        // keys a wave publishes
constexpr int kSbThreads = kFinThreads;
static_assert(kSbThreads == 512, "finalize_body's workgroup");
template <int DT, int NITER, int NS>
__global__ __launch_bounds__(kSbThreads) void small_batch_kernel(const uint4* __restrict__ shadow8, const float2* __restrict__ bmeta, const void* __restrict__ rows_,
                                                                  int64_t n, int d, int dpad, const float* __restrict__ in, int k, uint32_t row_base,
                                                                  const unsigned* __restrict__ eps_r_bits, float* __restrict__ qn, u64* __restrict__ cand,
                                                                  u64* __restrict__ dropmax, unsigned* __restrict__ ticket, unsigned* __restrict__ fb_count,
                                                                  unsigned* __restrict__ fb_list, u64* __restrict__ out_keys, float* __restrict__ out_dist,
                                                                  int64_t* __restrict__ out_rows, unsigned long long* __restrict__ stats,
                                                                  const uint32_t* __restrict__ dead) {
    constexpr int kWaves = kSbThreads / kWave;
    constexpr int kDpad8 = NS * 128;
    typedef unsigned sb_u32x4 __attribute__((ext_vector_type(4)));
    __shared__ __attribute__((aligned(16))) unsigned char s_q8[kDpad8];   // the query's int8 bytes, natural order
    __shared__ float s_qscale, s_eps, s_lo;
    __shared__ unsigned s_last;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nch = dpad >> 2;
    const int64_t G = gridDim.x;
    const int64_t nunits = (n + 15) >> 4;
    const int64_t W = G * kWaves;
    const int64_t wave_global = (int64_t)blockIdx.x * kWaves + wave;

    // the chunks of unit u (16 rows): read-once stream, non-temporal.  A unit index past the end is clamped (the loads are
    // unconditional: a conditional load makes hipcc drain the queue at every join); its results are never offered.
    auto load_unit = [&](sb_u32x4(&c)[2 * NS], float& scale, int64_t u) __attribute__((always_inline)) {
        const int64_t uu = u < nunits ? u : nunits - 1;
        scale = bmeta[uu >> 1].x;   // (in front of the chunks: the queue retires in order, a load issued behind them would drain the prefetch)
        const uint4* src = shadow8 + ((uu >> 1) * NS * 4 + (uu & 1) * 2) * 64 + lane;   // chunk (s, ks) at + (s * 4 + ks) * 64 pieces
#pragma unroll
        for (int j = 0; j < 2 * NS; ++j) c[j] = __builtin_nontemporal_load(reinterpret_cast<const sb_u32x4*>(src + ((j >> 1) * 4 + (j & 1)) * 64));
    };
    sb_u32x4 ca[2 * NS], cb[2 * NS];
    float sa = 0.0f, sb = 0.0f;
    int64_t u = wave_global;
    load_unit(ca, sa, u);

    // ---- the query: normalise (block 0 also stores qn: the last workgroup and the fallback scan read it) and quantise ----
    if (wave == 0) {
        int sh;
        const float nrm = canonical_norm(in, d, nch, lane, sh);
        const bool zero_row = !(nrm > 0.0f) || !(nrm < INFINITY);
        float vmax = 0.0f;
        for (int j = lane; j < nch; j += kWave) {
            float v[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int i = j * 4 + e;
                const float t = i < d ? in[i] : 0.0f;
                v[e] = zero_row ? 0.0f : scaled(t, sh) / nrm;
                vmax = fmaxf(vmax, fabsf(v[e]));
            }
            if (blockIdx.x == 0) reinterpret_cast<float4*>(qn)[j] = make_float4(v[0], v[1], v[2], v[3]);
        }
        vmax = butterfly_max(vmax);
        const float scale = vmax > 0.0f ? vmax / 127.0f : 0.0f, inv_scale = vmax > 0.0f ? 127.0f / vmax : 0.0f;
        float err2 = 0.0f;
        for (int j = lane; j < kDpad8 / 4; j += kWave) {
            float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            if (j < nch) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int i = j * 4 + e;
                    const float t = i < d ? in[i] : 0.0f;
                    v[e] = zero_row ? 0.0f : scaled(t, sh) / nrm;
                }
            }
            reinterpret_cast<uint32_t*>(s_q8)[j] = quantize4(v, inv_scale, scale, err2);
        }
        err2 = butterfly_sum(err2);
        if (lane == 0) {
            const float eq = __builtin_sqrtf(err2) * 1.0001f + 1e-7f, er = __uint_as_float(*eps_r_bits);
            s_qscale = scale;
            s_eps = eq * (1.01f + er) + 1.001f * er + 2e-6f;
        }
    }
    __syncthreads();
    const float qscale = s_qscale;

    // ---- the stream ----
    WaveTopK<1> L;
    L.init();
    const int kq = lane >> 4, r = lane & 15;
    auto score_unit = [&](const sb_u32x4(&c)[2 * NS], float scale, int64_t uu) __attribute__((always_inline)) {
        int acc = 0;
#pragma unroll
        for (int j = 0; j < 2 * NS; ++j) {
            const uint4 b = *reinterpret_cast<const uint4*>(s_q8 + j * 64 + kq * 16);
            acc = __builtin_amdgcn_sdot4((int)c[j][0], (int)b.x, acc, false);
            acc = __builtin_amdgcn_sdot4((int)c[j][1], (int)b.y, acc, false);
            acc = __builtin_amdgcn_sdot4((int)c[j][2], (int)b.z, acc, false);
            acc = __builtin_amdgcn_sdot4((int)c[j][3], (int)b.w, acc, false);
        }
        acc += __shfl_xor(acc, 16);
        acc += __shfl_xor(acc, 32);
        const int64_t block = uu >> 1;
        const int64_t row = (block << 5) + 16 * (uu & 1) + r;
        const float score = (float)acc * scale * qscale;
        // (a deleted row is no candidate: it would only crowd the wave's kSbKeep published keys and trip the margin test)
        const bool live = lane < 16 && row < n && !(dead && row_dead(dead, (uint32_t)row));
        const u64 key = live ? make_key(score, (uint32_t)row) : 0ull;
#ifdef CODD_SB_EXP_NOOFFER
        asm volatile("" ::"v"(key));  // diagnostic: scores computed, no top-k insert
#else
        L.offer_lanes(key, kWave, lane);
#endif
    };
#ifdef CODD_SB_EXP_NOSTREAM
    u = nunits;  // diagnostic: no stream at all
#endif
    while (u < nunits) {
        load_unit(cb, sb, u + W);
        score_unit(ca, sa, u);
        u += W;
        if (u >= nunits) break;
        load_unit(ca, sa, u + W);
        score_unit(cb, sb, u);
        u += W;
    }

    // ---- publish: the wave's best kSbKeep keys and the best key it keeps to itself ----
    if (lane < kSbKeep) cand[wave_global * kSbKeep + lane] = L.v[0];
    const u64 dropped = readlane_u64(L.v[0], kSbKeep);
    if (lane == 0) dropmax[wave_global] = dropped;

    // ---- the last workgroup to arrive answers the query ----
    __threadfence();
    __syncthreads();
    if (tid == 0) s_last = atomicAdd(ticket, 1u) == (unsigned)(G - 1) ? 1u : 0u;
    __syncthreads();
    if (!s_last) return;
    __threadfence();
#ifdef CODD_SB_EXP_NOFINAL
    if (tid == 0) { *ticket = 0u; *fb_count = 0u; }
    return;  // diagnostic: nothing behind the arrival ticket (results are garbage)
#endif
    if (tid == 0) {
        *ticket = 0u;    // (the next search finds the ticket at zero: no clearing launch)
        *fb_count = 0u;  // (the fallback queue of THIS search starts empty; the scan behind this kernel reads it)
    }
    __syncthreads();
    finalize_body<DT, NITER, 1>(rows_, dpad, qn, cand, (unsigned)(W * kSbKeep), 0u, 1u, k, s_eps, 0.0f, nullptr, row_base, out_keys, out_dist, out_rows, nullptr, stats,
                                dead, &s_lo);
    // margin test: could a wave have kept a row to itself that belongs among the survivors?
    const float lo = s_lo;
    unsigned bad = 0;
    for (int64_t i = tid; i < W; i += kSbThreads) {
        const u64 dm = dropmax[i];
        if (dm && key_score(dm) >= lo) bad = 1u;
    }
    if (__syncthreads_or((int)bad) && tid == 0) fb_list[atomicAdd(fb_count, 1u)] = 0u;
}

// row_norm_check_kernel: largest | |c| - 1 | over stored rows [first, first + n) that are not all-zero, folded into *dev_bits
// (non-negative floats order as their bits).  codd_knn_load_rows trusts nothing it is handed: both filters' bounds assume unit
// rows, and rows written with normalize = 0 (or a damaged rows.bin) must switch them off, not return wrong neighbours.
template <int DT>
__global__ __launch_bounds__(256) void row_norm_check_kernel(const void* __restrict__ rows_, int64_t first, int64_t n, int dpad,
                                                             unsigned* __restrict__ dev_bits) {
    typedef RowTraits<DT> RT;
    constexpr int E = RT::E;
    const int lane = lane_id();
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= n) return;
    const int nchunks = dpad / E;
    const uint4* p = reinterpret_cast<const uint4*>(rows_) + (first + r) * (int64_t)nchunks;
    float acc = 0.0f;
    for (int j = lane; j < nchunks; j += kWave) {
        float w[E];
        RT::widen(p[j], w);
#pragma unroll
        for (int e = 0; e < E; ++e) acc = __builtin_fmaf(w[e], w[e], acc);
    }
    const float nrm = __builtin_sqrtf(butterfly_sum(acc));
    if (lane == 0 && nrm != 0.0f) {
        const float dev = nrm == nrm ? fabsf(nrm - 1.0f) : INFINITY;  // NaN rows count as infinitely far from unit
        atomicMax(dev_bits, __float_as_uint(dev));
    }
}

template <int DT>
__global__ __launch_bounds__(256) void widen_rows_kernel(const void* __restrict__ rows_, int64_t first, int64_t n, int dim, int dpad,
                                                         float* __restrict__ out) {
    typedef RowTraits<DT> RT;
    constexpr int E = RT::E;
    const int lane = lane_id();
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= n) return;
    const int nchunks = dpad / E;
    const uint4* p = reinterpret_cast<const uint4*>(rows_) + (first + r) * (int64_t)nchunks;
    for (int j = lane; j < nchunks; j += kWave) {
        float w[E];
        RT::widen(p[j], w);
#pragma unroll
        for (int e = 0; e < E; ++e)
            if (j * E + e < dim) out[r * (int64_t)dim + j * E + e] = w[e];
    }
}

template <int DT, int NITER, int SLOTS>
__global__ __launch_bounds__(256) void ivf_scan_kernel(const void* __restrict__ rows_, const uint32_t* __restrict__ ids,
                                                       const int64_t* __restrict__ offsets, const u64* __restrict__ probe_keys,
                                                       int nprobe, int split, int dpad, const float* __restrict__ qn, int k,
                                                       uint32_t row_base, u64* __restrict__ partial, const uint32_t* __restrict__ dead) {
    // dead: the tombstone bits of the ORIGINAL row slots (ids[] carries them), null = none: a delete leaves the list layout valid
    typedef RowTraits<DT> RT;
    constexpr int E = RT::E;
    const int lane = lane_id();
    const int wave = (int)(threadIdx.x >> 6);
    const int b = blockIdx.y, x = blockIdx.x;
    const int nchunks = dpad / E;
    u64* dst = partial + ((int64_t)b * nprobe * split + x) * k;

    WaveTopK<SLOTS> L;
    L.init();
    const u64 pk = probe_keys[(int64_t)b * nprobe + x / split];
    if (pk != 0ull) {  // block-uniform: fewer lists than nprobe leave empty probe slots
        const uint32_t list = key_row(pk);
        const int64_t lo = offsets[list], hi = offsets[list + 1];
        const int64_t len = hi - lo, part = (len + split - 1) / split;
        const int64_t begin = lo + (x % split) * part;
        const int64_t end = begin + part < hi ? begin + part : hi;

        const uint4* base = reinterpret_cast<const uint4*>(rows_);
        [[maybe_unused]] float qf[1][NITER > 0 ? NITER : 1][E];
        [[maybe_unused]] float* lds_q = nullptr;
        if constexpr (NITER == kWideRows) {  // wide rows: the query in LDS
            __shared__ __attribute__((aligned(16))) float lds_qw[kWideMaxFloats];
            lds_q = lds_qw;
            wide_stage_query(lds_q, qn + (int64_t)b * dpad, dpad, wide_qfloats(nchunks, E), (int)threadIdx.x, 256);
            __syncthreads();
        } else {
            load_query_frags(qn + (int64_t)b * dpad, nchunks, lane, qf[0]);
        }
        for (int64_t g = begin + wave * 4; g < end; g += 16) {
            const uint4* p[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) p[r] = base + (g + r < end ? g + r : end - 1) * (int64_t)nchunks + lane;
            float sc[1][4];
            if constexpr (NITER == kWideRows) {
                wide_scores<DT, 1, 1>(p, nchunks, lane, lds_q, 0, 1, sc);
            } else {
                uint4 c[4][NITER];
                fetch4(p, nchunks, lane, c);
                score4<DT, 1, NITER>(c, qf, 1, lane, sc);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (g + r < end && !(dead && row_dead(dead, ids[g + r]))) L.offer(make_key(sc[0][r], row_base + ids[g + r]), k, lane);
        }
    }
    __shared__ u64 lds[4 * SLOTS * kWave];
    store_list(lds, wave, 1, 0, lane, L);
    __syncthreads();
    if (wave != 0) return;
    merge_lists(L, lds, 1, 4, 1, 0, k, lane);
    write_keys(L, k, lane, dst);
}

// ivf_scan_sq: ivf_scan_kernel for an l2 index ("space_ivf"): the same block per (query, probe rank, slice), the same
// loads and lists, the score is §20's canonical squared distance (score4 / wide_scores under kMetricL2: key score 0 - distance) of the
// RAW prepared query.  A kernel of its own beside its twin, not a shared body: ivf_scan_kernel keeps its resource line that way.
// (waves per SIMD: wide f32 rows with two list slots come out at 130 VGPRs, two above the four waves of the twin, unless hipcc is told
// to aim for four — then 128, no spill; every other form is left at the default, one wave at least)
template <int DT, int NITER, int SLOTS>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(DT == DT_F32 && NITER == kWideRows && SLOTS == 2 ? 4 : 1)))
void ivf_scan_sq(const void* __restrict__ rows_, const uint32_t* __restrict__ ids, const int64_t* __restrict__ offsets,
                 const u64* __restrict__ probe_keys, int nprobe, int split, int dpad, const float* __restrict__ qn, int k, uint32_t row_base,
                 u64* __restrict__ partial, const uint32_t* __restrict__ dead) {
    typedef RowTraits<DT> RT;
    constexpr int E = RT::E;
    const int lane = lane_id();
    const int wave = (int)(threadIdx.x >> 6);
    const int b = blockIdx.y, x = blockIdx.x;
    const int nchunks = dpad / E;
    u64* dst = partial + ((int64_t)b * nprobe * split + x) * k;

    WaveTopK<SLOTS> L;
    L.init();
    const u64 pk = probe_keys[(int64_t)b * nprobe + x / split];
    if (pk != 0ull) {  // block-uniform: fewer lists than nprobe leave empty probe slots
        const uint32_t list = key_row(pk);
        const int64_t lo = offsets[list], hi = offsets[list + 1];
        const int64_t len = hi - lo, part = (len + split - 1) / split;
        const int64_t begin = lo + (x % split) * part;
        const int64_t end = begin + part < hi ? begin + part : hi;

        const uint4* base = reinterpret_cast<const uint4*>(rows_);
        [[maybe_unused]] float qf[1][NITER > 0 ? NITER : 1][E];
        [[maybe_unused]] float* lds_q = nullptr;
        if constexpr (NITER == kWideRows) {  // wide rows: the query in LDS
            __shared__ __attribute__((aligned(16))) float lds_qw[kWideMaxFloats];
            lds_q = lds_qw;
            wide_stage_query(lds_q, qn + (int64_t)b * dpad, dpad, wide_qfloats(nchunks, E), (int)threadIdx.x, 256);
            __syncthreads();
        } else {
            load_query_frags(qn + (int64_t)b * dpad, nchunks, lane, qf[0]);
        }
        for (int64_t g = begin + wave * 4; g < end; g += 16) {
            const uint4* p[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) p[r] = base + (g + r < end ? g + r : end - 1) * (int64_t)nchunks + lane;
            float sc[1][4];
            if constexpr (NITER == kWideRows) {
                wide_scores<DT, 1, 1, kMetricL2, 1>(p, nchunks, lane, lds_q, 0, 1, sc);   // (USER 1: an instantiation of its own, exact_score.h)
            } else {
                uint4 c[4][NITER];
                fetch4(p, nchunks, lane, c);
                score4<DT, 1, NITER, kMetricL2>(c, qf, 1, lane, sc);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (g + r < end && !(dead && row_dead(dead, ids[g + r]))) L.offer(make_key(sc[0][r], row_base + ids[g + r]), k, lane);
        }
    }
    __shared__ u64 lds[4 * SLOTS * kWave];
    store_list(lds, wave, 1, 0, lane, L);
    __syncthreads();
    if (wave != 0) return;
    merge_lists(L, lds, 1, 4, 1, 0, k, lane);
    write_keys(L, k, lane, dst);
}

// ---------------------------------------------------------------------------------------------
// IVF at batch (round 3): a probed list is scanned ONCE for all the queries of the batch that probe it.  ivf_scan_kernel reads a
// list once per (query, list) pair — 256 queries x 32 probes over 2,048 lists read every list four times.  Here the pairs are
// grouped by list on the device (count, prefix sums, scatter: three tiny launches), every work item is (list, up to kIvfNB
// pairs): the list's rows enter registers once and are scored against the item's queries with the canonical exact expression.
// The item writes each pair's top-k to the pair's own slot of the partial buffer, so the merge behind it is the same launch
// as for the unshared scan and the results are the same bits.
// ---------------------------------------------------------------------------------------------
constexpr int kIvfNB = 4;  // queries per work item
__global__ __launch_bounds__(256) void ivf_pair_count_kernel(const u64* __restrict__ probe_keys, int npairs, unsigned* __restrict__ cnt) {
    const int p = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (p < npairs && probe_keys[p] != 0ull) atomicAdd(&cnt[key_row(probe_keys[p])], 1u);
}
// one workgroup: exclusive prefix sums over the lists — pair_start[l] (where list l's pairs go) and item_start[l] (its work
// items: ceil(cnt / kIvfNB)); cnt[] is cleared on the way (the scatter reuses it as its fill counters); nitems at item_start[nlist]
__global__ __launch_bounds__(1024) void ivf_pair_offsets_kernel(unsigned* __restrict__ cnt, int nlist, unsigned* __restrict__ pair_start,
                                                                unsigned* __restrict__ item_start) {
    __shared__ unsigned s_p[1024], s_i[1024];
    const int tid = (int)threadIdx.x;
    const int per = (nlist + 1023) / 1024;
    unsigned sp = 0, si = 0;
    for (int j = 0; j < per; ++j) {
        const int l = tid * per + j;
        const unsigned c = l < nlist ? cnt[l] : 0u;
        sp += c;
        si += (c + kIvfNB - 1) / kIvfNB;
    }
    s_p[tid] = sp;
    s_i[tid] = si;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {   // Hillis-Steele inclusive scan
        const unsigned a = tid >= off ? s_p[tid - off] : 0u, b = tid >= off ? s_i[tid - off] : 0u;
        __syncthreads();
        s_p[tid] += a;
        s_i[tid] += b;
        __syncthreads();
    }
    unsigned bp = s_p[tid] - sp, bi = s_i[tid] - si;   // exclusive bases of this thread's lists
    for (int j = 0; j < per; ++j) {
        const int l = tid * per + j;
        if (l < nlist) {
            const unsigned c = cnt[l];
            pair_start[l] = bp;
            item_start[l] = bi;
            bp += c;
            bi += (c + kIvfNB - 1) / kIvfNB;
            cnt[l] = 0u;
        }
    }
    if (tid == 1023) {
        pair_start[nlist] = s_p[1023];
        item_start[nlist] = s_i[1023];
    }
}
__global__ __launch_bounds__(256) void ivf_pair_scatter_kernel(const u64* __restrict__ probe_keys, int npairs, const unsigned* __restrict__ pair_start,
                                                               unsigned* __restrict__ fill, unsigned* __restrict__ sorted_pairs) {
    const int p = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (p >= npairs || probe_keys[p] == 0ull) return;
    const uint32_t l = key_row(probe_keys[p]);
    sorted_pairs[pair_start[l] + atomicAdd(&fill[l], 1u)] = (unsigned)p;
}
// list_scan_body: one workgroup of 4 waves scores positions [begin, end) of a row list against up to NB queries (q[b]: the query's
// normalised row, null = absent) and writes query b's k best keys to dst_of(b); a wave owns 4 positions per step.
//   GATHER = false (IVF): position i IS row i of the regrouped store and reports ids[i]; the next step's rows are on their way while
//                  this step is scored (raw 16-byte chunks: half the registers of widened rows)
//   GATHER = true (scopes): position i names row ids[i] of the original store and reports it.  Two steps of look-ahead: the row
//                  slots of step g + 32 and the rows of step g + 16 (whose slots arrived a step ago) are in flight
//   dead: the tombstone bits of the reported ids, null = no mask
template <int DT, int NB, int NITER, int SLOTS, bool GATHER, int METRIC = kMetricDot, class DstOf>
__device__ __forceinline__ void list_scan_body(const void* __restrict__ rows_, const uint32_t* __restrict__ ids, int64_t begin, int64_t end, int dpad,
                                               const float* const (&q)[NB], int nq, int k, uint32_t row_base, const uint32_t* __restrict__ dead,
                                               DstOf dst_of) {
    typedef RowTraits<DT> RT;
    constexpr int E = RT::E;
    const int lane = lane_id();
    const int wave = (int)(threadIdx.x >> 6);
    const int nchunks = dpad / E;
    const uint4* base = reinterpret_cast<const uint4*>(rows_);
    WaveTopK<SLOTS> L[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) L[b].init();
    auto load_ids = [&](int64_t g, uint32_t (&dst)[4]) {   // (g < end)
#pragma unroll
        for (int r = 0; r < 4; ++r) dst[r] = ids[g + r < end ? g + r : end - 1];
    };
    // where the rows of step g are: by position (clamped into the list), or by the slots `id` that load_ids(g) brought
    auto row_ptrs = [&](int64_t g, const uint32_t (&id)[4], const uint4* (&p)[4]) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            int64_t row = id[r];
            if constexpr (!GATHER) {
                row = g + r < end ? g + r : end - 1;
                row = row < begin ? begin : row;
            }
            p[r] = base + row * (int64_t)nchunks + lane;
        }
    };
    auto offer4 = [&](int64_t g, const uint32_t (&id)[4], const float (&sc)[NB][4]) {
#pragma unroll
        for (int b = 0; b < NB; ++b)
            if (b < nq) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    if constexpr (GATHER) {
                        if (g + r < end && !(dead && row_dead(dead, id[r]))) L[b].offer(make_key(sc[b][r], row_base + id[r]), k, lane);
                    } else {
                        if (g + r < end && !(dead && row_dead(dead, ids[g + r]))) L[b].offer(make_key(sc[b][r], row_base + ids[g + r]), k, lane);
                    }
                }
            }
    };
    const int64_t g0 = begin + wave * 4;
    uint32_t id0[4] = {0u, 0u, 0u, 0u}, id1[4] = {0u, 0u, 0u, 0u};
    if constexpr (NITER == kWideRows) {  // wide rows: the queries in LDS (64 KiB at most); the next step's row slots on their way
        __shared__ __attribute__((aligned(16))) float lds_q[NB * kWideMaxFloats];
        const int qstride = wide_qfloats(nchunks, E);
#pragma unroll
        for (int b = 0; b < NB; ++b) wide_stage_query(lds_q + b * qstride, q[b], dpad, qstride, (int)threadIdx.x, 256);
        __syncthreads();
        if (GATHER && g0 < end) load_ids(g0, id0);
        for (int64_t g = g0; g < end; g += 16) {
            if (GATHER && g + 16 < end) load_ids(g + 16, id1);
            const uint4* p[4];
            row_ptrs(g, id0, p);
            float sc[NB][4];
            wide_scores<DT, NB, 1, METRIC>(p, nchunks, lane, lds_q, qstride, nq, sc);
            offer4(g, id0, sc);
#pragma unroll
            for (int r = 0; r < 4; ++r) id0[r] = id1[r];
        }
    } else {
        float qf[NB][NITER][E];
#pragma unroll
        for (int b = 0; b < NB; ++b) load_query_frags(q[b], nchunks, lane, qf[b]);
        uint4 cur[4][NITER], nxt[4][NITER];
        const uint4* p[4];
        if (g0 < end) {
            if constexpr (GATHER) {
                load_ids(g0, id0);
                if (g0 + 16 < end) load_ids(g0 + 16, id1);
            }
            row_ptrs(g0, id0, p);
            fetch4(p, nchunks, lane, cur);
        }
        for (int64_t g = g0; g < end; g += 16) {
            uint32_t id2[4] = {0u, 0u, 0u, 0u};
            if (GATHER && g + 32 < end) load_ids(g + 32, id2);
            if (g + 16 < end) {
                row_ptrs(g + 16, id1, p);
                fetch4(p, nchunks, lane, nxt);
            }
            float sc[NB][4];
            score4<DT, NB, NITER, METRIC>(cur, qf, nq, lane, sc);
            offer4(g, id0, sc);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
#pragma unroll
                for (int it = 0; it < NITER; ++it) cur[r][it] = nxt[r][it];
                id0[r] = id1[r];
                id1[r] = id2[r];
            }
        }
    }
    __shared__ u64 lds[4 * NB * SLOTS * kWave];
#pragma unroll
    for (int b = 0; b < NB; ++b) store_list(lds, wave, NB, b, lane, L[b]);
    __syncthreads();
    for (int b = wave; b < nq; b += 4) {
        WaveTopK<SLOTS> M;
        M.init();
        merge_lists(M, lds, 0, 4, NB, b, k, lane);
        write_keys(M, k, lane, dst_of(b));
    }
}

// one work item per workgroup: item -> (list, its kIvfNB-pair group) by binary search in item_start
template <int DT, int NITER, int SLOTS>
__global__ __launch_bounds__(256) void ivf_scan_shared_kernel(const void* __restrict__ rows_, const uint32_t* __restrict__ ids, const int64_t* __restrict__ offsets,
                                                              const unsigned* __restrict__ pair_start, const unsigned* __restrict__ item_start,
                                                              const unsigned* __restrict__ sorted_pairs, int nlist, int nprobe, int dpad,
                                                              const float* __restrict__ qn, int k, uint32_t row_base, u64* __restrict__ partial,
                                                              const uint32_t* __restrict__ dead) {
    const unsigned item = blockIdx.x;
    if (item >= item_start[nlist]) return;   // (the grid is sized for the worst case: one item per pair)
    int lo_l = 0, hi_l = nlist;              // the last list whose item_start <= item
    while (hi_l - lo_l > 1) {
        const int mid = (lo_l + hi_l) >> 1;
        if (item_start[mid] <= item) lo_l = mid; else hi_l = mid;
    }
    const int list = lo_l;
    const unsigned g = item - item_start[list];
    const unsigned p0 = pair_start[list] + g * kIvfNB, p1e = pair_start[list + 1];
    const int nq = (int)((p1e - p0) < (unsigned)kIvfNB ? (p1e - p0) : (unsigned)kIvfNB);
    unsigned pair[kIvfNB];
    const float* q[kIvfNB];
#pragma unroll
    for (int b = 0; b < kIvfNB; ++b) {
        pair[b] = b < nq ? sorted_pairs[p0 + b] : 0u;
        q[b] = b < nq ? qn + (int64_t)(pair[b] / (unsigned)nprobe) * dpad : nullptr;
    }
    // the pair's own slot of the partial buffer: [query][probe rank][k]
    list_scan_body<DT, kIvfNB, NITER, SLOTS, false>(rows_, ids, offsets[list], offsets[list + 1], dpad, q, nq, k, row_base, dead,
                                                    [&](int b) { return partial + (int64_t)pair[b] * k; });
}
// ivf_shared_sq: the same work items for an l2 index: list_scan_body under kMetricL2
template <int DT, int NITER, int SLOTS>
__global__ __launch_bounds__(256) void ivf_shared_sq(const void* __restrict__ rows_, const uint32_t* __restrict__ ids, const int64_t* __restrict__ offsets,
                                                     const unsigned* __restrict__ pair_start, const unsigned* __restrict__ item_start,
                                                     const unsigned* __restrict__ sorted_pairs, int nlist, int nprobe, int dpad, const float* __restrict__ qn, int k,
                                                     uint32_t row_base, u64* __restrict__ partial, const uint32_t* __restrict__ dead) {
    const unsigned item = blockIdx.x;
    if (item >= item_start[nlist]) return;   // (the grid is sized for the worst case: one item per pair)
    int lo_l = 0, hi_l = nlist;              // the last list whose item_start <= item
    while (hi_l - lo_l > 1) {
        const int mid = (lo_l + hi_l) >> 1;
        if (item_start[mid] <= item) lo_l = mid; else hi_l = mid;
    }
    const int list = lo_l;
    const unsigned g = item - item_start[list];
    const unsigned p0 = pair_start[list] + g * kIvfNB, p1e = pair_start[list + 1];
    const int nq = (int)((p1e - p0) < (unsigned)kIvfNB ? (p1e - p0) : (unsigned)kIvfNB);
    unsigned pair[kIvfNB];
    const float* q[kIvfNB];
#pragma unroll
    for (int b = 0; b < kIvfNB; ++b) {
        pair[b] = b < nq ? sorted_pairs[p0 + b] : 0u;
        q[b] = b < nq ? qn + (int64_t)(pair[b] / (unsigned)nprobe) * dpad : nullptr;
    }
    list_scan_body<DT, kIvfNB, NITER, SLOTS, false, kMetricL2>(rows_, ids, offsets[list], offsets[list + 1], dpad, q, nq, k, row_base, dead,
                                                               [&](int b) { return partial + (int64_t)pair[b] * k; });
}

// ---------------------------------------------------------------------------------------------
// Scopes: a 32-bit label per row slot, 0 = none.  A scoped query sees only the rows of its scope.
//   scope_of[capacity]          the label of every slot (codd_knn_set_scopes_host)
//   scope_perm[count]           row slots grouped by scope, scope_offsets[nlist + 1] where each group starts (nlist = highest
//                               scope + 1; group 0 = the unlabelled rows).  Built lazily by the first scoped search after labels
//                               or the row count changed: count, prefix sums, scatter.  The order inside a group is whatever the
//                               atomics give: keys carry the row, so the top-k does not depend on it.
//   scope_scan_kernel           (scope, up to NB of the batch's queries with that scope, one of `split` parts of its group):
//                               gathers the group's rows from the ORIGINAL row store by slot and scores them with the canonical
//                               expression; one partial list per (query, part), merge_keys_kernel behind it.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void scope_set_kernel(const int64_t* __restrict__ packed, int64_t n, uint32_t* __restrict__ scope_of) {
    const int64_t i = (int64_t)blockIdx.x * 256 + (int64_t)threadIdx.x;
    if (i < n) scope_of[(uint32_t)(packed[i] & 0xffffffffll)] = (uint32_t)((u64)packed[i] >> 32);   // (slot in the low word, scope in the high one)
}
// A wave whose 64 rows carry one scope (labels assigned in runs, as the indexer job writes them) costs one atomic, not 64.
// (dead: the tombstone bits, null = none: deleted rows are left out of the lists, so scope_scan_kernel needs no mask of its own)
__global__ __launch_bounds__(256) void scope_count_kernel(const uint32_t* __restrict__ scope_of, int64_t n, int nlist, unsigned* __restrict__ cnt,
                                                          const uint32_t* __restrict__ dead) {
    const int64_t r = (int64_t)blockIdx.x * 256 + (int64_t)threadIdx.x;
    const bool valid = r < n && !(dead && row_dead(dead, (uint32_t)r));
    uint32_t s = valid ? scope_of[r] : 0u;
    if (s >= (uint32_t)nlist) s = 0u;   // (cannot happen: nlist covers every label ever set)
    const uint32_t first = (uint32_t)__builtin_amdgcn_readfirstlane((int)s);
    const u64 act = __ballot(valid), same = __ballot(valid && s == first);
    if (same == act) {
        if (lane_id() == 0 && act != 0ull) atomicAdd(&cnt[first], (unsigned)__popcll(act));
    } else if (valid) {
        atomicAdd(&cnt[s], 1u);
    }
}
// one workgroup: start[l] = exclusive prefix sum of cnt[], the total at start[nlist]; cnt[] is cleared on the way (the scatter's fill counters)
__global__ __launch_bounds__(1024) void scope_offsets_kernel(unsigned* __restrict__ cnt, int nlist, unsigned* __restrict__ start) {
    __shared__ unsigned s_p[1024];
    const int tid = (int)threadIdx.x;
    const int per = (nlist + 1023) / 1024;
    unsigned sp = 0;
    for (int j = 0; j < per; ++j) {
        const int l = tid * per + j;
        sp += l < nlist ? cnt[l] : 0u;
    }
    s_p[tid] = sp;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {   // Hillis-Steele inclusive scan
        const unsigned a = tid >= off ? s_p[tid - off] : 0u;
        __syncthreads();
        s_p[tid] += a;
        __syncthreads();
    }
    unsigned bp = s_p[tid] - sp;
    for (int j = 0; j < per; ++j) {
        const int l = tid * per + j;
        if (l < nlist) {
            const unsigned c = cnt[l];
            start[l] = bp;
            bp += c;
            cnt[l] = 0u;
        }
    }
    if (tid == 1023) start[nlist] = s_p[1023];
}
__global__ __launch_bounds__(256) void scope_scatter_kernel(const uint32_t* __restrict__ scope_of, int64_t n, int nlist, const unsigned* __restrict__ start,
                                                            unsigned* __restrict__ fill, uint32_t* __restrict__ perm, const uint32_t* __restrict__ dead) {
    const int64_t r = (int64_t)blockIdx.x * 256 + (int64_t)threadIdx.x;
    const bool valid = r < n && !(dead && row_dead(dead, (uint32_t)r));
    uint32_t s = valid ? scope_of[r] : 0u;
    if (s >= (uint32_t)nlist) s = 0u;
    const uint32_t first = (uint32_t)__builtin_amdgcn_readfirstlane((int)s);
    const u64 act = __ballot(valid), same = __ballot(valid && s == first);
    if (same == act) {   // (a valid lane's place: its rank among the valid lanes — deleted rows leave gaps)
        unsigned base = 0u;
        if (lane_id() == 0 && act != 0ull) base = atomicAdd(&fill[first], (unsigned)__popcll(act));
        base = (unsigned)__builtin_amdgcn_readfirstlane((int)base);
        if (valid) perm[start[first] + base + (unsigned)__popcll(act & ((1ull << lane_id()) - 1ull))] = (uint32_t)r;
    } else if (valid) {
        perm[start[s] + atomicAdd(&fill[s], 1u)] = (uint32_t)r;
    }
}
// One workgroup groups the batch's queries by scope: position p of the order (scope, query) holds query sorted_q[p], the rank[p]-th of its
// scope.  Counting ranks over LDS (B <= 1,024 broadcast reads per thread): the cost does not depend on how many scopes exist, where
// the count / prefix-sum / scatter of ivf_pair_* would walk a table of up to 2^20 scopes per search.
__global__ __launch_bounds__(1024) void scope_group_kernel(const uint32_t* __restrict__ scopes, int B, unsigned* __restrict__ sorted_q, unsigned* __restrict__ rank) {
    __shared__ uint32_t s_sc[CODD_KNN_MAX_BATCH];
    const int tid = (int)threadIdx.x;
    const uint32_t mine = tid < B ? scopes[tid] : 0xffffffffu;
    s_sc[tid] = mine;
    __syncthreads();
    if (tid >= B) return;
    unsigned lower = 0u, before = 0u;   // queries of a lower scope; ... plus those of this scope that come earlier in the batch
    for (int j = 0; j < B; ++j) {
        const uint32_t sj = s_sc[j];
        lower += sj < mine ? 1u : 0u;
        before += (sj < mine || (sj == mine && j < tid)) ? 1u : 0u;
    }
    sorted_q[before] = (unsigned)tid;
    rank[before] = before - lower;
}

// queries per work item: four, as in ivf_scan_shared_kernel; two for 2-byte rows of 4 chunks per lane (four queries' registers would spill)
constexpr int scope_nb(int dt, int niter) { return (dt != DT_F32 && niter == 4) ? 2 : 4; }
// rows per part: a whole number of workgroup steps (4 waves x 4 rows)
__host__ __device__ constexpr int64_t scope_part_rows(int64_t len, int split) { return ((len + split - 1) / split + 15) / 16 * 16; }

// grid (B, split): workgroup (p, part) serves the queries at positions p .. p + NB-1 of the grouped order when p opens a group of NB
// (rank[p] % NB == 0) and leaves at once otherwise.
template <int DT, int NITER, int SLOTS, int METRIC>
__device__ __forceinline__ void scope_scan_body(const void* __restrict__ rows_, const uint32_t* __restrict__ perm, const unsigned* __restrict__ offsets,
                                                int64_t count, uint32_t max_scope, const uint32_t* __restrict__ scopes,
                                                const unsigned* __restrict__ sorted_q, const unsigned* __restrict__ rank, int B, int split, int dpad,
                                                const float* __restrict__ qn, int k, uint32_t row_base, u64* __restrict__ partial) {
    constexpr int NB = scope_nb(DT, NITER);
    const int p0 = (int)blockIdx.x, part = (int)blockIdx.y;
    const unsigned r0 = rank[p0];
    if (r0 % NB != 0u) return;
    int nq = 1;
    while (nq < NB && p0 + nq < B && rank[p0 + nq] == r0 + (unsigned)nq) ++nq;   // (ranks count up inside a scope and restart at 0)
    const float* q[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) q[b] = b < nq ? qn + (int64_t)sorted_q[p0 + b] * dpad : nullptr;
    const uint32_t scope = scopes[sorted_q[p0]];
    int64_t lo = 0, hi = 0;   // the scope's rows: scope_perm[lo, hi); scope 0 = every listed row (`count`: the live rows); a scope nobody carries = none
    if (scope == 0u) hi = count;
    else if (scope <= max_scope) { lo = offsets[scope]; hi = offsets[scope + 1]; }
    const int64_t per = scope_part_rows(hi - lo, split);
    const int64_t begin = lo + part * per < hi ? lo + part * per : hi;
    const int64_t end = begin + per < hi ? begin + per : hi;
    // no mask: the lists hold live rows only.  Query b's part of the partial buffer: [query][part][k]
    list_scan_body<DT, NB, NITER, SLOTS, true, METRIC>(rows_, perm, begin, end, dpad, q, nq, k, row_base, nullptr,
                                                       [&](int b) { return partial + ((int64_t)sorted_q[p0 + b] * split + part) * k; });
}
template <int DT, int NITER, int SLOTS>
__global__ __launch_bounds__(256) void scope_scan_kernel(const void* __restrict__ rows_, const uint32_t* __restrict__ perm, const unsigned* __restrict__ offsets,
                                                         int64_t count, uint32_t max_scope, const uint32_t* __restrict__ scopes,
                                                         const unsigned* __restrict__ sorted_q, const unsigned* __restrict__ rank, int B, int split, int dpad,
                                                         const float* __restrict__ qn, int k, uint32_t row_base, u64* __restrict__ partial) {
    scope_scan_body<DT, NITER, SLOTS, kMetricDot>(rows_, perm, offsets, count, max_scope, scopes, sorted_q, rank, B, split, dpad, qn, k, row_base, partial);
}
template <int DT, int NITER, int SLOTS>
__global__ __launch_bounds__(256) void scope_scan_l2(const void* __restrict__ rows_, const uint32_t* __restrict__ perm, const unsigned* __restrict__ offsets,
                                                     int64_t count, uint32_t max_scope, const uint32_t* __restrict__ scopes,
                                                     const unsigned* __restrict__ sorted_q, const unsigned* __restrict__ rank, int B, int split, int dpad,
                                                     const float* __restrict__ qn, int k, uint32_t row_base, u64* __restrict__ partial) {
    scope_scan_body<DT, NITER, SLOTS, kMetricL2>(rows_, perm, offsets, count, max_scope, scopes, sorted_q, rank, B, split, dpad, qn, k, row_base, partial);
}

// ---------------------------------------------------------------------------------------------
// Tombstones and compaction.
//   dead_set_kernel        sets the bits of n row slots (vector atomics: several slots may share a word)
//   live_prefix_kernel     per bitmap word: the live slots of its 256-word block that lie below it (popcount, Hillis-Steele scan
//                          in LDS), and the block's total; scope_offsets_kernel turns the totals into block bases.  New slot of a
//                          live row r = base[block] + prefix[word] + live bits of its word below r: its rank among the live rows.
//   compact_gather_kernel  one wave per source row of a chunk [s0, s1), whole 16-byte pieces as gather_rows_kernel moves them: a
//                          live row goes to the bounce buffer at (new slot - dbase), dbase = the chunk's first destination; its
//                          scope label goes along.  The host then copies the bounce buffer to rows [dbase, dbase + live rows of
//                          the chunk): rows only move down, and that range ends at or before s1, the next chunk's first source.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void dead_set_kernel(const int64_t* __restrict__ slots, int64_t n, uint32_t* __restrict__ dead) {
    const int64_t i = (int64_t)blockIdx.x * 256 + (int64_t)threadIdx.x;
    if (i < n) atomicOr(&dead[slots[i] >> 5], 1u << (uint32_t)(slots[i] & 31));
}
// live slots of bitmap word w among rows [0, n)
__device__ __forceinline__ uint32_t live_bits(const uint32_t* __restrict__ dead, int64_t w, int64_t n) {
    const int64_t left = n - w * 32;
    const uint32_t in_range = left >= 32 ? 0xffffffffu : (left > 0 ? (1u << (uint32_t)left) - 1u : 0u);
    return ~dead[w] & in_range;
}
__global__ __launch_bounds__(256) void live_prefix_kernel(const uint32_t* __restrict__ dead, int64_t n, int64_t nwords, unsigned* __restrict__ prefix,
                                                          unsigned* __restrict__ block_total) {
    __shared__ unsigned s_p[256];
    const int tid = (int)threadIdx.x;
    const int64_t w = (int64_t)blockIdx.x * 256 + tid;
    const unsigned mine = w < nwords ? (unsigned)__popc(live_bits(dead, w, n)) : 0u;
    s_p[tid] = mine;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {   // Hillis-Steele inclusive scan
        const unsigned a = tid >= off ? s_p[tid - off] : 0u;
        __syncthreads();
        s_p[tid] += a;
        __syncthreads();
    }
    if (w < nwords) prefix[w] = s_p[tid] - mine;
    if (tid == 255) block_total[blockIdx.x] = s_p[255];
}
__global__ __launch_bounds__(256) void compact_gather_kernel(const uint4* __restrict__ rows, const uint32_t* __restrict__ dead, int64_t n,
                                                             const unsigned* __restrict__ prefix, const unsigned* __restrict__ block_base,
                                                             const uint32_t* __restrict__ scope_of, int64_t s0, int64_t s1, int64_t dbase,
                                                             int64_t bounce_rows, int chunks_per_row, uint4* __restrict__ bounce,
                                                             uint32_t* __restrict__ bounce_scope) {
    const int lane = lane_id();
    const int64_t r = s0 + (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= s1 || row_dead(dead, (uint32_t)r)) return;
    const int64_t w = r >> 5;
    const int64_t to = (int64_t)block_base[w >> 8] + prefix[w] + __popc(live_bits(dead, w, n) & ((1u << (uint32_t)(r & 31)) - 1u)) - dbase;
    if (to < 0 || to >= bounce_rows) return;   // (cannot happen: the host sized the chunk from the same bits)
    for (int j = lane; j < chunks_per_row; j += kWave) bounce[to * chunks_per_row + j] = rows[r * chunks_per_row + j];
    if (lane == 0 && scope_of) bounce_scope[to] = scope_of[r];
}

// ---------------------------------------------------------------------------------------------
// Masked search: one bitmap of ALLOWED row slots per call, shared by the batch's queries.
//   mask_deny_kernel     dense route: deny[w] = ~allow[w] | dead[w], all ones from the mask's last word on — the bitmap every
//                        exact-score kernel takes where it takes the tombstone bits (§14 with "dead" read as "denied")
//   mask_prefix_kernel   list route: per bitmap word the visible (allowed, live) slots of its 256-word block that lie below it, and
//                        the block's total (live_prefix_kernel's shape); scope_offsets_kernel turns the totals into block bases
//   mask_scatter_kernel  ... and each word writes its visible slots, ascending, from base[block] + prefix[word]: the list is the
//                        visible row slots in slot order, the same for every run
//   mask_scan_kernel     (group of up to NB of the batch's queries, one of `split` parts of the list): list_scan_body's gathering
//                        form, as scope_scan_kernel runs it; one partial list per (query, part), merge_keys_kernel behind it
// ---------------------------------------------------------------------------------------------
// the slots of bitmap word w among rows [0, n) that a masked search may return (dead: the tombstone bits, null = none)
__device__ __forceinline__ uint32_t visible_bits(const uint32_t* __restrict__ allow, const uint32_t* __restrict__ dead, int64_t w, int64_t n) {
    const int64_t left = n - w * 32;
    const uint32_t in_range = left >= 32 ? 0xffffffffu : (left > 0 ? (1u << (uint32_t)left) - 1u : 0u);
    return allow[w] & in_range & ~(dead ? dead[w] : 0u);
}
__global__ __launch_bounds__(256) void mask_deny_kernel(const uint32_t* __restrict__ allow, const uint32_t* __restrict__ dead, int64_t n, int64_t nwords,
                                                        int64_t total_words, uint32_t* __restrict__ deny) {
    const int64_t w = (int64_t)blockIdx.x * 256 + (int64_t)threadIdx.x;
    if (w < total_words) deny[w] = w < nwords ? ~visible_bits(allow, dead, w, n) : 0xffffffffu;
}
__global__ __launch_bounds__(256) void mask_prefix_kernel(const uint32_t* __restrict__ allow, const uint32_t* __restrict__ dead, int64_t n, int64_t nwords,
                                                          unsigned* __restrict__ prefix, unsigned* __restrict__ block_total) {
    __shared__ unsigned s_p[256];
    const int tid = (int)threadIdx.x;
    const int64_t w = (int64_t)blockIdx.x * 256 + tid;
    const unsigned mine = w < nwords ? (unsigned)__popc(visible_bits(allow, dead, w, n)) : 0u;
    s_p[tid] = mine;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {   // Hillis-Steele inclusive scan
        const unsigned a = tid >= off ? s_p[tid - off] : 0u;
        __syncthreads();
        s_p[tid] += a;
        __syncthreads();
    }
    if (w < nwords) prefix[w] = s_p[tid] - mine;
    if (tid == 255) block_total[blockIdx.x] = s_p[255];
}
__global__ __launch_bounds__(256) void mask_scatter_kernel(const uint32_t* __restrict__ allow, const uint32_t* __restrict__ dead, int64_t n, int64_t nwords,
                                                           const unsigned* __restrict__ prefix, const unsigned* __restrict__ block_base, int64_t m,
                                                           uint32_t* __restrict__ list) {
    const int64_t w = (int64_t)blockIdx.x * 256 + (int64_t)threadIdx.x;
    if (w >= nwords) return;
    uint32_t v = visible_bits(allow, dead, w, n);
    int64_t at = (int64_t)block_base[w >> 8] + prefix[w];
    for (; v != 0u; v &= v - 1u, ++at)
        if (at < m) list[at] = (uint32_t)(w * 32) + (uint32_t)(__ffs((int)v) - 1);   // (at < m always: the host counted the same bits)
}
// grid (ceil(B / NB), split): workgroup (g, part) serves queries g * NB .. g * NB + NB-1 over part `part` of list[0, m)
template <int DT, int NITER, int SLOTS, int METRIC>
__device__ __forceinline__ void mask_scan_body(const void* __restrict__ rows_, const uint32_t* __restrict__ list, int64_t m, int B, int split,
                                               int dpad, const float* __restrict__ qn, int k, uint32_t row_base, u64* __restrict__ partial) {
    constexpr int NB = scope_nb(DT, NITER);
    const int q0 = (int)blockIdx.x * NB, part = (int)blockIdx.y;
    const int nq = B - q0 < NB ? B - q0 : NB;
    const float* q[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) q[b] = b < nq ? qn + (int64_t)(q0 + b) * dpad : nullptr;
    const int64_t per = scope_part_rows(m, split);
    const int64_t begin = part * per < m ? part * per : m;
    const int64_t end = begin + per < m ? begin + per : m;
    // no mask: the list holds visible rows only.  Query b's part of the partial buffer: [query][part][k]
    list_scan_body<DT, NB, NITER, SLOTS, true, METRIC>(rows_, list, begin, end, dpad, q, nq, k, row_base, nullptr,
                                                       [&](int b) { return partial + ((int64_t)(q0 + b) * split + part) * k; });
}
template <int DT, int NITER, int SLOTS>
__global__ __launch_bounds__(256) void mask_scan_kernel(const void* __restrict__ rows_, const uint32_t* __restrict__ list, int64_t m, int B, int split,
                                                        int dpad, const float* __restrict__ qn, int k, uint32_t row_base, u64* __restrict__ partial) {
    mask_scan_body<DT, NITER, SLOTS, kMetricDot>(rows_, list, m, B, split, dpad, qn, k, row_base, partial);
}
template <int DT, int NITER, int SLOTS>
__global__ __launch_bounds__(256) void mask_scan_l2(const void* __restrict__ rows_, const uint32_t* __restrict__ list, int64_t m, int B, int split,
                                                    int dpad, const float* __restrict__ qn, int k, uint32_t row_base, u64* __restrict__ partial) {
    mask_scan_body<DT, NITER, SLOTS, kMetricL2>(rows_, list, m, B, split, dpad, qn, k, row_base, partial);
}

}  // namespace

// =============================================================================================
// host side: the index object and the C ABI
// =============================================================================================

enum { EV_SCAN = 0, EV_FILTER = 1, EV_SAMPLE = 2, EV_FINALIZE = 3, EV_KINDS = 4 };
static const char* const kEvNames[EV_KINDS] = {"scan", "filter", "sample", "finalize"};

// device control block of one filter pass (zeroed by ONE memset per pass)
struct FilterCtl {
    unsigned hit_cnt[kTileQ * kHitCntStride];
    unsigned flags[FLAG_WORDS];
    unsigned fb_count;         // queries queued for the exact-scan fallback ...
    unsigned fb_done;          // ... blocks of the fallback scan that have finished (the last one merges)
    unsigned sb_ticket;        // small_batch_kernel's arrival counter (its last workgroup puts it back to zero)
    unsigned pad_[1];
    unsigned fb_list[kTileQ];  // ... and which ones
};

// Search workspace.  An index keeps up to kMaxWork of them, one per HIP stream that searches it, so that searches
// issued on different streams (the next batch while this batch's small kernels and its collective are still in
// flight) never share scratch memory.  The index inherits one set of these fields: WorkScope loads the calling
// stream's set into them for the duration of one call and stores it back (a swap each way: one owner at any time).
struct WorkBufs {
    // (grown on demand, never inside a captured region after warm-up)
    DevBuf<float> qn;             // [B][dpad] normalised queries
    DevBuf<u64> partial;          // [B][blocks][k]
    DevBuf<u64> keys_tmp;         // [B][k]
    DevBuf<uint4> qfrag;          // pieces
    DevBuf<float> thr;            // [512]: thr[256], thr0[256]
    DevBuf<u64> bucket_max;       // [256][sample tiles] best (score, row) key per sampled tile
    DevBuf<u64> hits;             // [256][hit_cap_q]
    DevBuf<FilterCtl> ctl;        // device
    DevBuf<u64> fb_partial;       // [256][blocks][k] partials of the fallback scan
    DevBuf<uint4> qfrag8;         // int8 query fragments (pieces)
    DevBuf<float> qmeta;          // [1024]: per query: scale, 2*eps (device-wide bound), A, B (eps per block = A + B e_block)
    DevBuf<u64> sb_cand;          // small_batch_kernel: [waves][kSbKeep] published keys, then [waves] dropmax
    DevBuf<u64> probe_keys;       // IVF: [B][nprobe] coarse keys
    DevBuf<u64> ivf_partial;
    DevBuf<unsigned> ivf_group;   // IVF at batch: [nlist] counters, [nlist+1] pair starts, [nlist+1] item starts, [B*nprobe] pairs by list
    DevBuf<unsigned> scope_group; // scoped search: [B] queries in (scope, query) order, [B] their ranks inside the scope
    // masked search: the call's allow bits, and what the two routes derive from them
    PinnedBuf<uint32_t> mask_host;  // pinned staging of the allow words; mask_uploaded: its last copy to the device
    Event mask_uploaded; bool mask_upload_pending = false;
    DevBuf<uint32_t> mask_allow;    // [ceil(count / 32)] device copy of the allow words
    DevBuf<uint32_t> mask_deny;     // dense route: [ceil(capacity / 32)] ~allow | dead, ones past the mask
    DevBuf<unsigned> mask_prefix;   // list route: [words] prefixes, [blocks] totals, [blocks + 1] bases
    DevBuf<uint32_t> mask_list;     // list route: [m] visible row slots, ascending
    // codd_knn_search_masked_dev: the visible rows of a device mask, counted on the device and read back through pinned memory
    DevBuf<unsigned long long> mask_m_dev;
    PinnedBuf<unsigned long long> mask_m_host;
};
static_assert(!std::is_copy_constructible<WorkBufs>::value, "a workspace has one owner (WorkScope swaps, never copies)");
constexpr int kMaxWork = 4;
struct WorkSlot {
    WorkBufs bufs;
    hipStream_t stream = nullptr;
    Event handover;                 // recorded on the old stream when the slot changes hands
    bool used = false;
    uint64_t tick = 0;              // last use (LRU)
};

struct codd_knn_index : WorkBufs {
    int device = 0;
    int dim = 0;
    int dpad = 0;
    int dtype = 0;
    int metric = 0;
    int num_cus = 256;
    int scan_blocks_per_cu = 4;
    int64_t capacity = 0;  // row slots allocated
    int64_t count = 0;     // highest written slot + 1
    DevBuf<unsigned char> rows;  // [capacity][dpad] storage dtype, as bytes; zero at and past `count` (a never-written slot below the count is a zero row)
    // bf16 fragment-order copy, whole 256-row tiles.  Derived data like the int8 shadow: built lazily from the stored rows by the
    // first search that needs it (batches above 256 queries, an index with the int8 filter off or cooling down, the IVF
    // build), brought up to date incrementally over the rows written since
    DevBuf<uint4> shadow;
    int64_t shadow_rows = 0;       // rows the shadow allocation covers (multiple of 256)
    int64_t shadow_epoch = -1;
    int64_t dirty16_lo = 0, dirty16_hi = 0;
    hipStream_t shadow_stream = nullptr;
    Event shadow_ready;
    int64_t stat_shadow_builds = 0;
    int64_t shadow_nomem_epoch = -1;   // row epoch at which allocating the bf16 shadow failed: not retried until rows change
    int64_t stat_shadow_nomem = 0;
    int debug_fail_shadow_alloc = 0;   // test hook ("debug_fail_shadow_alloc"): the next bf16-shadow allocation reports out of memory
    // stored rows written on a caller's stream (upsert_device): searches on other streams wait for this on the device
    Event rows_ready;
    hipStream_t rows_stream = nullptr;
    bool rows_event_set = false;
    // ... and rows read on a caller's stream outside a search (copy_rows_f32): the next writer on another stream waits for it
    Event reader_done;
    hipStream_t reader_stream = nullptr;
    bool reader_event_set = false;
    // staging of codd_knn_upsert_host (kept between calls: the indexer job upserts in small batches)
    DevBuf<float> stage_vec;
    DevBuf<int64_t> stage_slot;
    bool all_normalized = true;    // false once a caller stored rows with normalize = 0

    // filter path knobs
    int filter_enabled = 1;
    int64_t filter_min_rows = 1;             // batches >= filter_min_batch: only the tile-count condition applies
    int64_t filter_min_rows_small = 100000;  // batches below filter_min_batch: filter when rows * B reaches this
    int filter_min_batch = 9;
    int sample_tiles = 4096;  // upper bound on sampled tiles (reached from 42M rows on)
    int sample_div = 40;      // sample about 1/40 of the tiles (2.5 % extra GEMM work), see sample_tile_count()
    int hit_cap_q = 131072;  // candidates kept per query before it falls back to the exact scan (256 MiB per searching stream at 256 queries:
                             // a cluster of 60,000 near-identical rows — closer to each other than either filter's slack — stays on the filter path)

    DevBuf<unsigned long long> dstats;                     // device counters: hits, survivors, fallback queries

    // int8 shadow for small batches (optional; rebuilt lazily from the stored rows when they have changed)
    int shadow8_enabled = 1;
    int shadow8_max_batch = 256;  // batches up to this size (one query pass) take the int8 filter
    int resident_q = 1;           // rows of <= 512 int8 elements: the query block stays in LDS ("resident_q" option)
    int i8v2 = 2;                 // batches of 65..256 queries on rows of >= 384 elements (3 K-steps) take i8_tile_kernel (filter_i8.h); 1: only rows of
                                  // more than 512 elements (below, the first-generation kernel keeps the query block resident in LDS: 6-12 % slower); 0: never
    int i8v2_half = 1;            // ... and so do batches of 65..128 queries (its 8-query-block instantiation)
    int ivf_share = 1;            // IVF search: from 1,024 (query, list) pairs on, a probed list is scanned once for all its queries ("ivf_share": 0 = per pair)
    int fuse_fallback = 1;        // batches above 64 queries, k <= 64: finalize and the exact-scan fallback in one launch ("fuse_fallback": 0 = two launches)
    int small_batch_max = 0;      // 1: a single query is answered in one launch by small_batch_kernel where it applies.  OFF by default: measured SLOWER than the
                                  // six-launch chain (1M x 768, B = 1: kernel 0.27 ms, p50 0.33 ms against 0.25 ms; profiles/r3/small_batch_latency.txt)
    int64_t stat_small_batch = 0;
    int per_block = 7;            // the int8 bound per 32-row block: bit 0 in i8_tile_kernel, bit 1 in finalize ("per_block" option; 0 = the device-wide bound everywhere;
                                  // bit 2 chose between block metadata and per-row scales in the tile kernel's filter pass until the per-row path was removed: ignored)
    int i8_pair = 2;              // rows of 6, 12, ... K-steps: the staged tile program with one workgroup barrier per two K-steps ("i8_pair" option: 0 = one per K-step;
                                  // 2 = ... and rows of exactly 6 K-steps its static form, i8_tile_kernel<., 3, ., false>)
    int sample_div8 = 28;         // its thresholds come from a larger sample (the int8 slack is ~5x the bf16 one)
    int sample_rounds8 = 2;       // ... of at least this many rounds of workgroups (one tile each) when the batch has more than 32 queries (3 until the round-3 epilogue:
                                  // at 1.25M rows two rounds trade 13 us of sample for 7 us of filter, gpurun_out/r3n/ab_sample_1p25m.txt)
    DevBuf<uint4> shadow8;
    int64_t shadow8_rows = 0;     // rows the allocation covers (multiple of 256)
    DevBuf<float> rscale;         // [shadow8_rows]
    DevBuf<float2> bmeta;         // [shadow8_rows / 32]: per 32-row block {scale, largest error norm |c - c~| of its rows}; NaN scale: no row of the block exists
    DevBuf<unsigned> eps_r_bits;     // device scalar: max row error norm (float bits)
    // the int8 filter leg of an ip or l2 index ("space_filter" option, off by default).  Derived with the int8 shadow,
    // over the same dirty rows, and only for such an index: rnorm2[row] = the row's canonical sum of squares; *rmax_bits = the float
    // bits of R >= |c| for every row ever stored (it only grows: delete and compact never lower it)
    int space_filter = 0;
    // IVF on an ip or l2 index ("space_ivf" option, off by default): the coarse index in the index's own space, raw
    // centroids, the list scans by the index's metric.  No effect on a cosine index.
    int space_ivf = 0;
    DevBuf<float> rnorm2;            // [shadow8_rows]
    DevBuf<unsigned> rmax_bits;
    int64_t shadow8_epoch = -1;
    int64_t dirty_lo = 0, dirty_hi = 0;  // rows written since the int8 shadow was last brought up to date: [lo, hi)
    hipStream_t shadow8_stream = nullptr;  // the stream the last rebuild ran on, and its completion
    Event shadow8_ready;
    int64_t stat_shadow8_builds = 0, stat_shadow8_passes = 0, stat_i8v2_passes = 0, stat_f16_tile_passes = 0;
    int f16_tile = 1;             // the 2-byte filter of 129..256 queries over rows of 6, 12, ... 64-element K-steps (768 elements: 12) runs the tile program of
                                  // filter_i8.h on fp16 operands ("f16_tile" option; 0 = gemm_filter_kernel)
    // the worst row's quantisation error, copied back asynchronously after every build: a corpus with badly
    // quantisable rows (one large element, many small ones) would make the int8 bound useless and send every small batch
    // to the exact-scan fallback, so such an index keeps the bf16 filter.  Performance only: never needed for exactness.
    PinnedBuf<float> eps_r_host;
    Event eps_r_copied;
    float eps_r_known = 0.0f;
    int64_t wide_blocks_known = 0;      // blocks whose error norm exceeds shadow8_max_eps, as last read back
    float shadow8_max_eps = 0.04f;
    // Which filter suits the DATA is watched too: on corpora with dense clusters the wider int8 slack lets thousands of
    // rows per query through to the exact re-scoring, where the bf16 filter (a fifth of the slack) is the faster one
    // (profiles/r1/clustered_data_check.txt).  The device counters of the filter passes are copied back
    // asynchronously; when the int8 passes since the last look left more than shadow8_max_surv survivors per query, or
    // sent queries to the fallback, the next shadow8_cooldown searches take the bf16 filter, then the int8 one is
    // tried again.  Performance only: either filter returns the same bits.
    PinnedBuf<unsigned long long> watch_host;  // copy of dstats[0..3]
    Event watch_copied;
    bool watch_pending = false;
    unsigned long long watch_surv = 0, watch_fb = 0;  // counter values at the last look
    int64_t watch_q8 = 0, watch_q16 = 0;              // queries filtered since then, by path
    int64_t watch_q8_sent = 0, watch_q16_sent = 0;    // ... as of the copy in flight
    int shadow8_max_surv = 4000;
    int shadow8_cooldown = 256;
    int cooldown_left = 0;
    int64_t stat_cooldowns = 0;
    double cooldown_surv8 = 0.0;          // survivors per query of the int8 passes that started the current cooldown
    int64_t cooldown_useless_epoch = -1;  // row epoch at which the bf16 filter was seen to leave as many survivors as the int8 one: no more cooldowns until rows change
    float exp_slack_scale = 1.0f;  // always 1 in the shipped library; "exp_slack_pct" exists only in -DCODD_EXPERIMENTS=1 builds

    // IVF (optional): rows regrouped by coarse list, original slots, list offsets, the coarse index
    codd_knn_index* coarse = nullptr;  // nlist centroids, f32 (owned: destroyed through codd_knn_destroy)
    DevBuf<unsigned char> rows_ivf;
    DevBuf<uint32_t> ivf_ids;
    DevBuf<int64_t> ivf_offsets;       // [nlist + 1]
    int64_t ivf_count = 0;             // rows covered by the IVF layout (must equal count to be fresh)
    int ivf_nlist = 0;
    int64_t ivf_epoch = -1, epoch = 0;  // epoch bumps on every row write; search requires ivf_epoch == epoch

    // scopes (optional): a label per row slot and, derived from it like the shadows, the row slots grouped by label
    DevBuf<uint32_t> scope_of;         // [capacity], 0 = no label; allocated by the first call that needs it
    DevBuf<uint32_t> scope_perm;       // [count] row slots grouped by scope
    DevBuf<unsigned> scope_offsets;    // [nlist + 1] group starts, then [nlist] counters of the build
    uint32_t max_scope = 0;            // highest label ever set
    int64_t scope_gen = 0;             // bumps on every codd_knn_set_scopes_host
    int64_t scope_built_gen = -1, scope_built_count = -1;  // what scope_perm / scope_offsets were built from
    hipStream_t scope_stream = nullptr;  // the stream the last build ran on, and its completion
    Event scope_ready;
    int64_t stat_scoped_searches = 0, stat_scope_builds = 0;

    // masked search
    int mask_route = 0;        // "mask_route": 0 = by the routing rule, 1 = always the list route, 2 = always the dense route
    int mask_list_pct = 100;   // "mask_list_pct": the list route's side of the cost comparison, in percent (100 = the derived rule)
    DevBuf<unsigned long long> mask_dstats;     // the device counters of the dense masked passes: kept apart from dstats, which the filter watch reads
    int64_t stat_masked_searches = 0, stat_mask_list = 0, stat_mask_dense = 0, stat_last_mask_rows = 0;
    int64_t stat_masked_dev = 0;   // ... those of them whose mask was on the device already (codd_knn_search_masked_dev)

    // document snapshot (optional, derived data like the shadows): every row slot's document in one byte arena, a 0x00
    // behind each, zeros to the end of the allocation (csrc/doc_match.h), and the [count + 1] arena offsets.  Valid while the row
    // epoch and the count are what they were when codd_knn_set_documents_host took it.
    DevBuf<uint8_t> doc_arena;
    DevBuf<int64_t> doc_offsets;
    int64_t doc_bytes = 0;             // the arena: the documents' bytes plus one separator each
    int64_t doc_count = -1, doc_epoch = -1;
    int64_t stat_doc_matches = 0;

    // tombstones: one bit per row slot, set = deleted.  Null until the first codd_knn_delete_host — the kernels
    // take a null pointer as "nothing was ever deleted" and load nothing.  The host keeps a mirror: the write paths refuse dead
    // slots from it and compaction derives the row mapping from it, so nothing is ever read back.
    DevBuf<uint32_t> dead_bits;                                     // [ceil(capacity / 32)] device words
    std::vector<uint32_t> dead_host;                                // the same bits
    int64_t dead_count = 0;                                         // dead slots below `count`
    int64_t first_dead = INT64_MAX;                                 // lowest dead slot
    int64_t compact_chunk_rows = 0;                                 // "compact_chunk_rows" option: source rows per compaction chunk (0 = what 64 MiB hold)
    int64_t stat_delete_calls = 0, stat_compactions = 0;

    int64_t stat_searches = 0, stat_scan_launches = 0, stat_last_scan_blocks = 0;
    int64_t stat_last_scan_group = 0;       // queries per pass over the rows of the last exact scan (1, 4 or 8; wide 2-byte rows: at most 4)
    int64_t stat_last_finalize_parts = 0;   // workgroups per query of the last filter pass's finalize
    int64_t stat_ivf_shared = 0;            // IVF searches that scanned each probed list once for all its queries (ivf_scan_shared_kernel)
    int64_t stat_ivf_masked = 0;            // IVF searches under a row mask (codd_knn_ivf_search_masked, _masked_dev: DESIGN.md §17)
    int64_t stat_filter_passes = 0;

    // optional HIP-event timing of the heavy kernels (bench.py's roofline figure): one (start, stop)
    // pair per launch, recorded on the launch stream, read after a sync
    bool profile = false;
    std::vector<Event> ev;  // 2 * pairs
    std::vector<int> ev_kind;
    int ev_used = 0;

    WorkSlot slots[kMaxWork];
    uint64_t tick = 0;
    std::mutex mu;  // one host thread at a time enqueues a search (the launches themselves are asynchronous)

    // (the members free themselves: the caller has made `device` current and idle, see codd_knn_destroy)
    ~codd_knn_index() { (void)codd_knn_destroy(coarse); }
};
static_assert(!std::is_copy_constructible<codd_knn_index>::value, "an index owns its device memory");

// The device embedder: no index behind it — an index does not exist before the first upsert fixes the width.
// One pinned staging buffer and its device copy, both laid out [n + 1 offsets][bytes]; `uploaded` frees the staging buffer for
// the next call, `embedded` orders a call on another stream behind the kernel that still reads the device copy.
struct codd_knn_embedder {
    int device = 0;
    int dim = 0;
    float trigram_weight = 0.0f;
    bool device_seen = false;          // the first call that embeds checks that `device` exists; create and destroy touch no device before
    PinnedBuf<unsigned char> stage_host;
    DevBuf<unsigned char> stage_dev;
    Event uploaded, embedded;
    bool upload_pending = false, embedded_set = false;
    hipStream_t last_stream = nullptr;
    std::mutex mu;                     // one host thread at a time stages and enqueues
};

namespace {

thread_local char g_err[512] = "";

int fail(int code, const char* fmt, const char* detail = "") {
    snprintf(g_err, sizeof(g_err), fmt, detail);
    return code;
}

// every row write: bumps the epoch (IVF / int8 shadow staleness) and widens the dirty row range
void rows_written(codd_knn_index* ix, int64_t lo, int64_t hi) {
    ix->epoch++;
    if (ix->dirty_hi <= ix->dirty_lo) { ix->dirty_lo = lo; ix->dirty_hi = hi; }
    else {
        if (lo < ix->dirty_lo) ix->dirty_lo = lo;
        if (hi > ix->dirty_hi) ix->dirty_hi = hi;
    }
    if (ix->dirty16_hi <= ix->dirty16_lo) { ix->dirty16_lo = lo; ix->dirty16_hi = hi; }
    else {
        if (lo < ix->dirty16_lo) ix->dirty16_lo = lo;
        if (hi > ix->dirty16_hi) ix->dirty16_hi = hi;
    }
}

// the end of every write of row slots inside [lo, hi): raises the count, then rows_written.  A write that starts above the count
// brings the slots in between into existence unwritten.  They are zero rows: the row store holds zeros at and
// past the count (grow_rows, codd_knn_compact), but both shadows still hold there whatever they held — int8 block meta data that
// reads NaN since the allocation, rows from before a compaction — so they are dirty from the old count on.
void slots_written(codd_knn_index* ix, int64_t lo, int64_t hi) {
    if (hi > ix->count) {
        if (lo > ix->count) lo = ix->count;
        ix->count = hi;
    }
    rows_written(ix, lo, hi);
}

#define HIP_TRY(expr)                                                                        \
    do {                                                                                     \
        hipError_t e__ = (expr);                                                             \
        if (e__ != hipSuccess) {                                                             \
            snprintf(g_err, sizeof(g_err), "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__), __FILE__, __LINE__); \
            return e__ == hipErrorOutOfMemory ? CODD_KNN_ENOMEM : CODD_KNN_EDEVICE;          \
        }                                                                                    \
    } while (0)

struct DeviceGuard {
    int prev = -1;
    bool changed = false;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) == hipSuccess && prev != dev) changed = hipSetDevice(dev) == hipSuccess;
    }
    ~DeviceGuard() {
        if (changed) (void)hipSetDevice(prev);
    }
};

struct EvScope {  // records a (start, stop) pair around one launch when profiling is on
    codd_knn_index* ix;
    hipStream_t st;
    int slot = -1;
    EvScope(codd_knn_index* ix_, int kind, hipStream_t st_) : ix(ix_), st(st_) {
        if (ix->profile && 2 * (ix->ev_used + 1) <= (int)ix->ev.size()) {
            slot = ix->ev_used++;
            ix->ev_kind[slot] = kind;
            (void)hipEventRecord(ix->ev[2 * slot], st);
        }
    }
    ~EvScope() {
        if (slot >= 0) (void)hipEventRecord(ix->ev[2 * slot + 1], st);
    }
};

// Loads the calling stream's workspace into the index for one call (see WorkBufs).  A stream keeps its slot; a new
// stream takes a free slot, or the least recently used one after making itself wait for everything the previous
// owner has enqueued so far (no host synchronisation; if that stream no longer exists the device is drained instead).
struct WorkScope {
    codd_knn_index* ix;
    int slot = 0;
    WorkScope(codd_knn_index* ix_, hipStream_t st) : ix(ix_) {
        ix->mu.lock();
        int free_slot = -1, lru = 0;
        slot = -1;
        for (int i = 0; i < kMaxWork; ++i) {
            WorkSlot& w = ix->slots[i];
            if (w.used && w.stream == st) { slot = i; break; }
            if (!w.used && free_slot < 0) free_slot = i;
            if (w.used && ix->slots[lru].used && w.tick < ix->slots[lru].tick) lru = i;
        }
        if (slot < 0 && free_slot >= 0) slot = free_slot;
        if (slot < 0) {
            slot = lru;
            WorkSlot& w = ix->slots[slot];
            bool ordered = false;
            (void)w.handover.ensure();
            if (w.handover && hipEventRecord(w.handover, w.stream) == hipSuccess) ordered = hipStreamWaitEvent(st, w.handover, 0) == hipSuccess;
            if (!ordered) {
                (void)hipGetLastError();
                (void)hipDeviceSynchronize();
            }
        }
        WorkSlot& w = ix->slots[slot];
        w.used = true;
        w.stream = st;
        w.tick = ++ix->tick;
        std::swap(static_cast<WorkBufs&>(*ix), w.bufs);
    }
    ~WorkScope() {
        std::swap(static_cast<WorkBufs&>(*ix), ix->slots[slot].bufs);
        ix->mu.unlock();
    }
    WorkScope(const WorkScope&) = delete;
    WorkScope& operator=(const WorkScope&) = delete;
};

size_t elem_size(int dtype) { return dtype == DT_F32 ? 4 : 2; }
int elems_per_chunk(int dtype) { return dtype == DT_F32 ? 4 : 8; }

int grow_dead_bits(codd_knn_index* ix, int64_t slots);

// (re)allocate row storage for at least `need` slots, preserving contents (the shadows are derived data with their own
// allocations: ensure_shadow / ensure_shadow8)
int grow_rows(codd_knn_index* ix, int64_t need, bool exact) {
    if (need <= ix->capacity) return CODD_KNN_OK;
    int64_t cap = need;
    if (!exact) {
        cap = ix->capacity > 0 ? ix->capacity : 1024;
        while (cap < need) cap += cap / 2 + 1024;
    }
    const size_t row_bytes = (size_t)ix->dpad * elem_size(ix->dtype);
    DevBuf<unsigned char> fresh;
    HIP_TRY(fresh.reset(cap * (int64_t)row_bytes));
    hipError_t e = hipMemset(fresh, 0, (size_t)cap * row_bytes);
    if (e == hipSuccess && ix->rows && ix->count > 0) e = hipMemcpy(fresh, ix->rows, (size_t)ix->count * row_bytes, hipMemcpyDeviceToDevice);
    if (e != hipSuccess) return fail(CODD_KNN_EDEVICE, "row copy on growth failed: %s", hipGetErrorString(e));
    if (ix->scope_of && ix->scope_of.cap() < cap) {  // the labels grow with the row store: new slots start with scope 0
        DevBuf<uint32_t> labels;
        e = labels.reset(cap);
        if (e == hipSuccess) e = hipMemset(labels, 0, (size_t)cap * sizeof(uint32_t));
        if (e == hipSuccess) e = hipMemcpy(labels, ix->scope_of, (size_t)ix->scope_of.bytes(), hipMemcpyDeviceToDevice);
        if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? CODD_KNN_ENOMEM : CODD_KNN_EDEVICE, "growing the scope labels failed: %s", hipGetErrorString(e));
        ix->scope_of = std::move(labels);
    }
    if (ix->dead_bits) {  // ... and so do the tombstone bits, once they exist
        const int rc = grow_dead_bits(ix, cap);
        if (rc != 0) return rc;
    }
    ix->rows = std::move(fresh);
    ix->capacity = cap;
    return CODD_KNN_OK;
}

// the tombstone bits cover `slots` row slots (device words and host mirror; contents kept, new words zero).  Exclusive callers only.
int grow_dead_bits(codd_knn_index* ix, int64_t slots) {
    const int64_t words = (slots + 31) / 32;
    if (words <= ix->dead_bits.cap()) return CODD_KNN_OK;
    try {
        ix->dead_host.resize((size_t)words, 0u);
    } catch (const std::bad_alloc&) {
        return fail(CODD_KNN_ENOMEM, "host allocation failed%s");
    }
    DevBuf<uint32_t> fresh;
    hipError_t e = fresh.reset(words);
    if (e == hipSuccess) e = hipMemset(fresh, 0, (size_t)words * sizeof(uint32_t));
    if (e == hipSuccess && ix->dead_bits) e = hipMemcpy(fresh, ix->dead_bits, (size_t)ix->dead_bits.bytes(), hipMemcpyDeviceToDevice);
    if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? CODD_KNN_ENOMEM : CODD_KNN_EDEVICE, "growing the tombstone bits failed: %s", hipGetErrorString(e));
    ix->dead_bits = std::move(fresh);
    return CODD_KNN_OK;
}

bool slot_dead(const codd_knn_index* ix, int64_t slot) {
    return ix->dead_count > 0 && slot >= 0 && (slot >> 5) < (int64_t)ix->dead_host.size() && ((ix->dead_host[(size_t)(slot >> 5)] >> (slot & 31)) & 1u);
}
// any dead slot in [lo, hi)?  (the write paths: a dead slot stays dead until codd_knn_compact)
bool range_has_dead(const codd_knn_index* ix, int64_t lo, int64_t hi) {
    if (ix->dead_count == 0 || hi <= ix->first_dead) return false;
    for (int64_t r = lo > ix->first_dead ? lo : ix->first_dead; r < hi && r < ix->count; ++r)
        if (slot_dead(ix, r)) return true;
    return false;
}
// live slots in [lo, hi), from the host mirror
int64_t live_in_range(const codd_knn_index* ix, int64_t lo, int64_t hi) {
    int64_t dead = 0;
    for (int64_t r = lo; r < hi;) {
        if ((r & 31) == 0 && r + 32 <= hi) { dead += __builtin_popcount(ix->dead_host[(size_t)(r >> 5)]); r += 32; }
        else { dead += (ix->dead_host[(size_t)(r >> 5)] >> (r & 31)) & 1u; ++r; }
    }
    return (hi - lo) - dead;
}

// ---- kernel dispatch -------------------------------------------------------------------------
// Each run-time choice of a template argument is made in one place: a with_* helper calls the generic lambda `f` with a
// std::integral_constant of the chosen value (usable as a template argument inside f) and returns what f returns (a
// CODD_KNN_* code).  A value no kernel is built for is an error.

template <int V>
using IntC = std::integral_constant<int, V>;

// f(IntC<V>) for the V of Vs that equals v, else EINVAL with `unsupported` (a fail() format)
template <int... Vs, typename F>
int with_int(int v, const char* unsupported, F&& f) {
    bool found = false;
    int rc = CODD_KNN_OK;
    ((v == Vs ? (found = true, rc = f(IntC<Vs>{})) : 0), ...);
    return found ? rc : fail(CODD_KNN_EINVAL, unsupported);
}

template <typename F>
int with_dtype(int dtype, F&& f) {
    return with_int<DT_F32, DT_BF16, DT_F16>(dtype, "unknown dtype%s", f);
}

// the NITER values the wide forms serve: rows of 5 .. 16 chunks per lane (f32: 1,025 .. 4,096 elements; 2-byte: 2,049 .. 4,096)
constexpr int kMaxNiter = 16;

// chunks of the padded row per lane: the NITER of the exact-score row kernels
int niter_of(const codd_knn_index* ix) { return (ix->dpad / elems_per_chunk(ix->dtype) + kWave - 1) / kWave; }

// 1 .. 4 chunks per lane: NITER itself; 5 .. kMaxNiter: the wide form (kWideRows); wider: ENOTSUP with `too_wide`
template <typename F>
int with_niter(int niter, const char* too_wide, F&& f) {
    switch (niter) {
        case 1: return f(IntC<1>{});
        case 2: return f(IntC<2>{});
        case 3: return f(IntC<3>{});
        case 4: return f(IntC<4>{});
    }
    if (niter > 4 && niter <= kMaxNiter) return f(IntC<kWideRows>{});
    return fail(CODD_KNN_ENOTSUP, too_wide);
}

// list slots per lane of a top-k list: one for k <= 64, else two
template <typename F>
int with_slots(int k, F&& f) {
    return k <= 64 ? f(IntC<1>{}) : f(IntC<2>{});
}

// 32-query blocks of a filter pass
template <typename F>
int with_nbq(int nbq, F&& f) {
    return with_int<1, 2, 4, 8>(nbq, "bad query block count%s", f);
}

// f(DT, NITER, SLOTS): the form of an exact-score row kernel for the index's rows and k
template <typename F>
int with_row_form(const codd_knn_index* ix, int k, const char* too_wide, F&& f) {
    return with_dtype(ix->dtype, [&](auto dt) {
        return with_niter(niter_of(ix), too_wide, [&](auto ni) {
            return with_slots(k, [&](auto sl) { return f(dt, ni, sl); });
        });
    });
}

// Dynamic LDS above 64 KiB needs the instantiation's opt-in, once per device (the caller's DeviceGuard has made the index's
// device current).  `bytes` must be at least what any launch of `Kernel` asks for.
template <auto Kernel>
int opt_in_lds(size_t bytes) {
    static std::atomic<uint64_t> done{0};  // one bit per device
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    const uint64_t bit = dev < 64 ? 1ull << dev : 0ull;
    if (!bit || !(done.load(std::memory_order_acquire) & bit)) {
        HIP_TRY(hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
        done.fetch_or(bit, std::memory_order_acq_rel);
    }
    return CODD_KNN_OK;
}

// dynamic LDS of a launch, and what its kernel opts in to when that is above 64 KiB (by default the same: a kernel launched
// with one size only)
struct Lds {
    size_t bytes, opt_in;
    Lds(size_t b) : bytes(b), opt_in(b) {}
    Lds(size_t b, size_t most) : bytes(b), opt_in(most) {}
};
constexpr size_t kLdsNoOptIn = 64 * 1024;

// every launch of a template kernel, and every launch with dynamic LDS; the caller checks hipGetLastError
template <auto Kernel, typename... Args>
int launch_kernel(dim3 grid, dim3 block, Lds lds, hipStream_t st, Args&&... args) {  // (by reference: an owning buffer converts to its pointer at the launch itself)
    int rc;
    if (lds.bytes > kLdsNoOptIn && (rc = opt_in_lds<Kernel>(lds.opt_in)) != 0) return rc;
    hipLaunchKernelGGL(Kernel, grid, block, lds.bytes, st, args...);
    return CODD_KNN_OK;
}

int launch_normalize(int dtype, const float* in, int64_t n, int d, int dpad, int normalize, const int64_t* slots,
                     int64_t first_slot, void* out, uint2* shadow, hipStream_t st) {
    if (n <= 0) return CODD_KNN_OK;
    const dim3 grid((unsigned)((n + 3) / 4)), block(256);
    const int rc = with_dtype(dtype, [&](auto dt) {
        return launch_kernel<normalize_rows_kernel<dt>>(grid, block, 0, st, in, n, d, dpad, normalize, slots, first_slot, out, shadow);
    });
    if (rc != 0) return rc;
    HIP_TRY(hipGetLastError());
    return CODD_KNN_OK;
}

// raw_rows_kernel: vectors as given (non-finite and all-zero ones as zeros), padded and rounded to `dtype`
int launch_raw_rows(int dtype, const float* in, int64_t n, int d, int dpad, const int64_t* slots, int64_t first_slot, void* out, hipStream_t st) {
    if (n <= 0) return CODD_KNN_OK;
    const dim3 grid((unsigned)((n + 3) / 4)), block(256);
    const int rc = with_dtype(dtype, [&](auto dt) { return launch_kernel<raw_rows_kernel<dt>>(grid, block, 0, st, in, n, d, dpad, slots, first_slot, out); });
    if (rc != 0) return rc;
    HIP_TRY(hipGetLastError());
    return CODD_KNN_OK;
}

// the metric of an index as its exact-score kernels see it: ip scores with the dot-product kernels that cosine runs
static_assert(kMetricDot == CODD_KNN_METRIC_COSINE && kMetricL2 == CODD_KNN_METRIC_L2, "exact_score.h and codd_knn.h disagree");
bool metric_is_cosine(const codd_knn_index* ix) { return ix->metric == CODD_KNN_METRIC_COSINE; }
// IVF: cosine always; ip and l2 with "space_ivf" on
bool ivf_allowed(const codd_knn_index* ix) { return metric_is_cosine(ix) || ix->space_ivf; }
int kernel_metric(int metric) { return metric == CODD_KNN_METRIC_L2 ? kMetricL2 : kMetricDot; }

// the ingest launch of every upsert.  normalize = 0 on an ip or l2 index still zeroes non-finite rows (the contract of those
// spaces); on a cosine index it stores the values as they come, as it always did
int launch_ingest(const codd_knn_index* ix, const float* in, int64_t n, int normalize, const int64_t* slots, int64_t first_slot, hipStream_t st) {
    if (!normalize && !metric_is_cosine(ix)) return launch_raw_rows(ix->dtype, in, n, ix->dim, ix->dpad, slots, first_slot, ix->rows.get(), st);
    return launch_normalize(ix->dtype, in, n, ix->dim, ix->dpad, normalize, slots, first_slot, ix->rows.get(), nullptr, st);
}

// the queries of an exact-score pass, fp32 [B][dpad] in ix->qn: normalised for cosine, as given for ip and l2
int prep_exact_queries(codd_knn_index* ix, const float* dev_queries, int B, hipStream_t st) {
    if (metric_is_cosine(ix)) return launch_normalize(DT_F32, dev_queries, B, ix->dim, ix->dpad, 1, nullptr, 0, ix->qn, nullptr, st);
    return launch_raw_rows(DT_F32, dev_queries, B, ix->dim, ix->dpad, nullptr, 0, ix->qn.get(), st);
}

// ---- exact scan dispatch ---------------------------------------------------------------------

struct ScanArgs {
    const void* rows;
    int64_t n;
    int dpad;
    const float* qn;
    int nq, k;
    uint32_t row_base;
    u64* partial;
    int64_t stride_q;
    const unsigned* qlist = nullptr;   // LISTED mode (device-side fallback queue)
    const unsigned* qcount = nullptr;
    unsigned* merge_done = nullptr;    // LISTED mode: the last block merges and writes the answers (one launch)
    u64* merged_keys = nullptr;
    float* merged_dist = nullptr;
    int64_t* merged_rows = nullptr;
    unsigned long long* count_total = nullptr;
    const uint32_t* dead = nullptr;    // tombstone bits (null: nothing was ever deleted)
};

// queries per pass of the wide scan: 2-byte rows take at most 4 (8 would spill: the kernel walks a larger batch 4 queries at a time)
constexpr int wide_scan_nb(int dt, int nb) { return dt == DT_F32 || nb < 4 ? nb : 4; }
// ... and of the wide l2 scan: the same, but 2-byte rows with two list slots per lane (k > 64) take 2 (the subtraction's temporaries on top
// of 4 queries' accumulators and 8 list registers spill one vector register in scan_topk_wide_l2<bf16, 4, 2>)
constexpr int wide_scan_nb_l2(int dt, int nb, int slots) { return dt != DT_F32 && slots == 2 && nb >= 4 ? 2 : wide_scan_nb(dt, nb); }

// one exact-scan launch, queries in groups of `nb` (1, 4 or 8) per pass over the rows
// (l2: the squared-distance kernels, dense queries only)
int launch_scan(int dtype, int nb, int niter, dim3 grid, hipStream_t st, const ScanArgs& a, int metric = kMetricDot) {
    if (metric == kMetricL2 && (a.qlist || a.qcount)) return fail(CODD_KNN_EINVAL, "the l2 scan takes dense queries only%s");
    return with_dtype(dtype, [&](auto dt) {
        constexpr int DT = decltype(dt)::value;
        return with_int<1, 4, 8>(nb, "bad query group%s", [&](auto nbc) {
            constexpr int NB = decltype(nbc)::value;
            return with_slots(a.k, [&](auto sl) {
                constexpr int SLOTS = decltype(sl)::value;
                return with_niter(niter, "row too wide for the scan kernel%s", [&](auto ni) {
                    constexpr int NITER = decltype(ni)::value;
                    if constexpr (NITER == kWideRows) {
                        // rows of more than 4 chunks per lane: scan_topk_wide_kernel, one 8-wave workgroup per compute unit (scan_geometry sizes the grid)
                        constexpr int NBW = wide_scan_nb(DT, NB);
                        constexpr int E = RowTraits<DT>::E;
                        if (metric == kMetricL2) {
                            constexpr int NBL = wide_scan_nb_l2(DT, NB, SLOTS);
                            const size_t qbytes = (size_t)NBL * wide_qfloats(a.dpad / E, E) * sizeof(float);
                            const size_t lbytes = (size_t)kWideScanWaves * NBL * SLOTS * kWave * sizeof(u64);
                            return launch_kernel<scan_topk_wide_l2<DT, NBL, SLOTS>>(grid, dim3(kWideScanWaves * kWave),
                                                                                    Lds(qbytes > lbytes ? qbytes : lbytes, (size_t)NBL * kWideMaxFloats * sizeof(float)),
                                                                                    st, a.rows, a.n, a.dpad, a.qn, a.nq, a.k, a.row_base, a.partial, a.stride_q, a.dead);
                        }
                        const size_t qbytes = (size_t)NBW * wide_qfloats(a.dpad / E, E) * sizeof(float);
                        const size_t lbytes = (size_t)kWideScanWaves * NBW * SLOTS * kWave * sizeof(u64);
                        const size_t lds = qbytes > lbytes ? qbytes : lbytes;   // the lists take the queries' place once a group is scanned
                        return launch_kernel<scan_topk_wide_kernel<DT, NBW, SLOTS>>(
                            grid, dim3(kWideScanWaves * kWave), Lds(lds, (size_t)NBW * kWideMaxFloats * sizeof(float)), st, a.rows, a.n, a.dpad, a.qn, a.nq,
                            a.k, a.row_base, a.partial, a.stride_q, a.qlist, a.qcount, a.merge_done, a.merged_keys, a.merged_dist, a.merged_rows, a.count_total, a.dead);
                    } else {
                        const size_t lds = (size_t)4 * NB * SLOTS * kWave * sizeof(u64);
                        if (metric == kMetricL2)
                            return launch_kernel<scan_topk_l2<DT, NB, NITER, SLOTS>>(grid, dim3(256), lds, st, a.rows, a.n, a.dpad, a.qn, a.nq, a.k, a.row_base,
                                                                                     a.partial, a.stride_q, a.dead);
                        return launch_kernel<scan_topk_kernel<DT, NB, NITER, SLOTS>>(
                            grid, dim3(256), lds, st, a.rows, a.n, a.dpad, a.qn, a.nq, a.k, a.row_base, a.partial, a.stride_q, a.qlist, a.qcount,
                            a.merge_done, a.merged_keys, a.merged_dist, a.merged_rows, a.count_total, a.dead);
                    }
                });
            });
        });
    });
}

int launch_merge(const u64* in, int B, int64_t m, int64_t in_stride, int k, u64* out_keys, float* out_dist, int64_t* out_rows,
                 hipStream_t st, const unsigned* out_list = nullptr, const unsigned* count_ptr = nullptr,
                 unsigned long long* count_total = nullptr, int64_t seg_len = 0, int64_t seg_stride = 0, int metric = kMetricDot) {
    if (seg_len <= 0) seg_len = m > 0 ? m : 1;
    if (metric == kMetricL2 && (out_list || count_ptr)) return fail(CODD_KNN_EINVAL, "the l2 merge takes no query list%s");
    const int rc = with_slots(k, [&](auto sl) {
        if (metric == kMetricL2)
            return launch_kernel<merge_keys_l2<sl>>(dim3(B), dim3(256), 0, st, in, m, in_stride, seg_len, seg_stride, k, out_keys, out_dist, out_rows);
        return launch_kernel<merge_keys_kernel<sl>>(dim3(B), dim3(256), 0, st, in, m, in_stride, seg_len, seg_stride, k, out_keys, out_dist, out_rows,
                                                    out_list, count_ptr, count_total);
    });
    if (rc != 0) return rc;
    HIP_TRY(hipGetLastError());
    return CODD_KNN_OK;
}

// the merge behind an index's own exact-score passes: distances by the index's metric
int launch_merge_of(const codd_knn_index* ix, const u64* in, int B, int64_t m, int k, u64* out_keys, float* out_dist, int64_t* out_rows, hipStream_t st) {
    return launch_merge(in, B, m, m, k, out_keys, out_dist, out_rows, st, nullptr, nullptr, nullptr, 0, 0, kernel_metric(ix->metric));
}

int scan_geometry(const codd_knn_index* ix, int64_t n, int* niter, int64_t* blocks) {
    *niter = niter_of(ix);
    if (*niter > kMaxNiter) return fail(CODD_KNN_ENOTSUP, "dim too large (<= 4096 elements)%s");
    const int64_t ngroups = (n + 3) / 4;
    if (*niter > 4) {  // scan_topk_wide_kernel: workgroups of 8 waves, one per compute unit (its query block fills the LDS)
        int64_t b = (ngroups + kWideScanWaves - 1) / kWideScanWaves;
        if (b > ix->num_cus) b = ix->num_cus;
        *blocks = b < 1 ? 1 : b;
        return CODD_KNN_OK;
    }
    int64_t b = (ngroups + 3) / 4;
    const int64_t cap_blocks = (int64_t)ix->num_cus * ix->scan_blocks_per_cu;
    if (b > cap_blocks) b = cap_blocks;
    if (b < 1) b = 1;
    *blocks = b;
    return CODD_KNN_OK;
}

// exact scan of `nqueries` dense normalised queries -> keys_out[nqueries][k]
// (deny: the bitmap of rows no answer may hold — the tombstone bits, or a masked search's ~allow | dead; null = none)
int exact_scan(codd_knn_index* ix, const float* qn, int nqueries, int k, uint32_t row_base, u64* keys_out, float* dist_out,
               int64_t* rows_out, hipStream_t st, const uint32_t* deny) {
    const int64_t n = ix->count;
    int niter;
    int64_t blocks;
    int rc = scan_geometry(ix, n, &niter, &blocks);
    if (rc != 0) return rc;
    ix->stat_last_scan_blocks = blocks;
    const int64_t stride_q = blocks * k;
    HIP_TRY(ix->partial.ensure((int64_t)nqueries * stride_q));
    {
        // ONE launch: up to 8 queries ride along per pass over the rows; a larger batch loops over groups
        // of 8 inside the kernel (small corpora stay L2-resident across the groups, and a batch costs one
        // launch instead of B/8)
        const int nb = nqueries == 1 ? 1 : (nqueries <= 4 ? 4 : 8);
        ix->stat_last_scan_group = niter <= 4 ? nb : (ix->metric == CODD_KNN_METRIC_L2 ? wide_scan_nb_l2(ix->dtype, nb, k <= 64 ? 1 : 2) : wide_scan_nb(ix->dtype, nb));
        ScanArgs a{ix->rows, n, ix->dpad, qn, nqueries, k, row_base, ix->partial, stride_q};
        a.dead = deny;
        {
            EvScope ev(ix, EV_SCAN, st);
            rc = launch_scan(ix->dtype, nb, niter, dim3((unsigned)blocks), st, a, kernel_metric(ix->metric));
        }
        if (rc != 0) return rc;
        HIP_TRY(hipGetLastError());
        ix->stat_scan_launches++;
    }
    return launch_merge_of(ix, ix->partial, nqueries, stride_q, k, keys_out, dist_out, rows_out, st);
}

// ---- filter path -----------------------------------------------------------------------------

float filter_eps(const codd_knn_index* ix) {
    // |approx - exact| for unit-norm q and c.  u = unit roundoff of the shadow element type under round-to-nearest:
    // half the spacing of the significand grid relative to the value (bf16: 8 significant bits, spacing 2^-7 -> u = 2^-8;
    // fp16: 11 significant bits -> u = 2^-11).  Round 1 shipped 2^-9 for bf16, half the true bound: a unit vector of 239
    // equal entries scores 0.99286 against itself in bf16 (error 0.0071 > the old eps 0.0040):
    //   rounding  : (2u + u^2) when q and the stored row are both rounded (Cauchy-Schwarz over the
    //               element-wise relative errors); u when the stored rows already are exactly
    //               representable (bf16 rows under a bf16 shadow, f16 rows under an fp16 shadow);
    //   subnormal : fp16 only — below 2^-14 the grid is absolute (2^-25 per element, <= sqrt(dpad) * 2^-25
    //               per operand after Cauchy-Schwarz against a unit vector);
    //   summation : two fp32 accumulations of <= dpad terms whose magnitudes sum to <= 1: dpad * 2^-24 each.
#if CODD_SHADOW_F16
    const float u = 4.8828125e-4f;
    const bool exact_rows = ix->dtype == DT_F16;
    const float subnormal = 2.0f * sqrtf((float)ix->dpad) * 2.9802322e-8f;
#else
    const float u = 0.00390625f;
    const bool exact_rows = ix->dtype == DT_BF16;
    const float subnormal = 0.0f;
#endif
    const float rounding = exact_rows ? u : 2.0f * u + u * u;
    const float summation = (float)ix->dpad * 1.1920929e-7f;  // dpad * 2^-23
    return (rounding + subnormal + summation) * 1.001f;
}

size_t filter_lds_bytes(int mode) {
    return (size_t)kLdsQBytes + kLdsWords * 4 + (mode == MODE_FILTER ? (size_t)kHitCap * 12 : 0);
}

int ensure_filter_workspace(codd_knn_index* ix) {
    HIP_TRY(ix->qfrag.ensure((int64_t)kTileQ * (ix->dpad / 8)));
    HIP_TRY(ix->bucket_max.ensure((int64_t)ix->sample_tiles * kTileQ));
    HIP_TRY(ix->hits.ensure((int64_t)kTileQ * ix->hit_cap_q));
    if (!ix->thr) HIP_TRY(ix->thr.reset(2 * kTileQ));  // thr[q], then thr0[q] (per-block form, int8 tile kernel)
    if (!ix->ctl) {
        HIP_TRY(ix->ctl.reset(1));
        HIP_TRY(hipMemset(ix->ctl, 0, sizeof(FilterCtl)));  // (the filter passes clear it per pass; small_batch_kernel relies on zeros left behind)
    }
    if (!ix->dstats) {
        HIP_TRY(ix->dstats.reset(4));
        HIP_TRY(hipMemset(ix->dstats, 0, 4 * sizeof(unsigned long long)));
    }
    return CODD_KNN_OK;
}

// how many evenly spaced tiles set the thresholds: ~ntiles/sample_div (so the sample costs a fixed
// fraction of the main pass at every shard size and the hit volume per query stays ~k*sample_div),
// at least max(64, 4k) where the corpus has that many tiles, at most sample_tiles
int64_t sample_tile_count(const codd_knn_index* ix, int64_t ntiles, int k, bool use8 = false, int nbq = 8) {
    int64_t ts = ntiles / (use8 ? (nbq == 1 ? 2 * ix->sample_div8 : ix->sample_div8) : ix->sample_div);
    if (use8) {
        // the int8 filter pays more per hit (wider slack, more of them) and less per sampled tile: "sample_rounds8" rounds of
        // workgroups (2 since round 3's cheaper epilogue; 3 before) where that is still under a quarter of the corpus
        // (1/10 of a 1.25M-row shard, 1/28 of 10M rows; twice as sparse for <= 32 queries, whose sample is a pure byte stream)
        const int64_t rounds = (nbq == 1 ? 1 : ix->sample_rounds8) * (int64_t)ix->num_cus;
        const int64_t floor8 = rounds < ntiles / 4 ? rounds : ntiles / 4;
        if (ts < floor8) ts = floor8;
    }
    const int64_t lo = 4 * (int64_t)k > 64 ? 4 * (int64_t)k : 64;
    if (ts < lo) ts = lo;
    // a sample of fewer tiles than there are CUs takes as long as one full round of workgroups (one tile each), and a
    // bigger sample means a tighter threshold: fewer hits for the filter's epilogue (scripts/rows_sweep.py)
    if (ts < ix->num_cus && ntiles >= 2 * (int64_t)ix->num_cus) ts = ix->num_cus;
    // whole rounds of workgroups: the last round costs a round whether it is full or not
    if (ts > ix->num_cus) ts = (ts + ix->num_cus - 1) / ix->num_cus * ix->num_cus;
    if (ts > ix->sample_tiles) ts = ix->sample_tiles;
    if (ts > ntiles) ts = ntiles;
    return ts < 1 ? 1 : ts;
}

int dpad8_of(const codd_knn_index* ix) { return (ix->dpad + 127) / 128 * 128; }

// Searches on a stream other than the one rows were last written on (codd_knn_upsert_device is asynchronous on the caller's
// stream) wait for that write on the device before they read rows or rebuild a shadow from them.
int wait_rows(codd_knn_index* ix, hipStream_t st) {
    if (ix->rows_event_set && st != ix->rows_stream) HIP_TRY(hipStreamWaitEvent(st, ix->rows_ready, 0));
    return CODD_KNN_OK;
}

// Before a derived buffer is freed (a shadow outgrown by the corpus): wait on the host for the streams that search THIS index
// — what they have enqueued so far may still read the old allocation — not for the whole device.  (Growth is the one
// place where a search call blocks; steady-state searches never do.)
int wait_searching_streams(codd_knn_index* ix) {
    for (WorkSlot& w : ix->slots) {
        if (!w.used) continue;
        HIP_TRY(w.handover.ensure());
        if (hipEventRecord(w.handover, w.stream) == hipSuccess) HIP_TRY(hipEventSynchronize(w.handover));
        else (void)hipGetLastError();  // (a stream that no longer exists has nothing in flight)
    }
    return CODD_KNN_OK;
}

// The bf16 shadow, like the int8 one, is derived data: (re)built from the stored rows on the searching stream whenever rows
// have been written since the last build, over the dirty row range only.  An index that only ever sees batches of <= 256
// queries (the int8 filter) never allocates it: 38 GB instead of 54 GB for the 10M x 768 fp32 corpus.
int ensure_shadow(codd_knn_index* ix, hipStream_t st) {
    const int64_t n = ix->count;
    if (ix->shadow_epoch == ix->epoch && ix->shadow) {
        if (st != ix->shadow_stream && ix->shadow_ready) HIP_TRY(hipStreamWaitEvent(st, ix->shadow_ready, 0));
        return CODD_KNN_OK;
    }
    const int64_t need = (n + kTileRows - 1) / kTileRows * kTileRows;
    int64_t first = ix->dirty16_lo, m = ix->dirty16_hi - ix->dirty16_lo;
    if (first + m > n) m = n > first ? n - first : 0;  // (never past the count: the allocation below is only checked against it)
    if (need > ix->shadow_rows) {
        // A failed allocation is remembered until rows change (no multi-GB hipMalloc retried by every search); the caller
        // answers the search another way (search_impl: the int8 filter or the exact scan).
        if (ix->shadow_nomem_epoch == ix->epoch) return CODD_KNN_ENOMEM;
        int rc;
        if ((rc = wait_searching_streams(ix)) != 0) return rc;
        (void)ix->shadow.reset();
        ix->shadow_rows = 0;
        const int64_t rows = need + need / 8;
        const int64_t rows_al = (rows + kTileRows - 1) / kTileRows * kTileRows;
        hipError_t me = ix->debug_fail_shadow_alloc ? hipErrorOutOfMemory : ix->shadow.reset(rows_al * ix->dpad * 2 / (int64_t)sizeof(uint4));
        if (me != hipSuccess) {
            (void)hipGetLastError();
            ix->shadow_nomem_epoch = ix->epoch;
            ix->stat_shadow_nomem++;
            return fail(CODD_KNN_ENOMEM, "bf16 shadow: %s", hipGetErrorString(me));
        }
        ix->shadow_rows = rows_al;
        HIP_TRY(hipMemsetAsync(ix->shadow, 0, (size_t)rows_al * ix->dpad * 2, st));  // rows beyond the count are masked, their bytes only have to be defined
        first = 0; m = n;
    }
    HIP_TRY(ix->shadow_ready.ensure());
    if (m > 0) {
        const dim3 grid((unsigned)((m + 3) / 4)), block(256);
        uint2* sh = reinterpret_cast<uint2*>(ix->shadow.get());
        const int rc = with_dtype(ix->dtype, [&](auto dt) {
            return launch_kernel<shadow_from_rows_kernel<dt>>(grid, block, 0, st, ix->rows, first, m, ix->dpad, sh);
        });
        if (rc != 0) return rc;
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(ix->shadow_ready, st));
    ix->shadow_stream = st;
    ix->shadow_epoch = ix->epoch;
    ix->dirty16_lo = ix->dirty16_hi = 0;
    ix->stat_shadow_builds++;
    return CODD_KNN_OK;
}

// The int8 shadow is derived data: (re)built from the stored rows on the searching stream whenever rows have been
// written since the last build.  Other streams that search before the build has finished wait for it on the device.
int ensure_shadow8(codd_knn_index* ix, hipStream_t st) {
    const int64_t n = ix->count;
    const int dpad8 = dpad8_of(ix);
    if (ix->shadow8_epoch == ix->epoch && ix->shadow8) {
        if (st != ix->shadow8_stream && ix->shadow8_ready) HIP_TRY(hipStreamWaitEvent(st, ix->shadow8_ready, 0));
        return CODD_KNN_OK;
    }
    const int64_t need = (n + kTileRows - 1) / kTileRows * kTileRows;
    int64_t first = ix->dirty_lo, m = ix->dirty_hi - ix->dirty_lo;  // rows to (re)quantise
    if (first + m > n) m = n > first ? n - first : 0;  // (never past the count: the allocation below is only checked against it)
    if (!ix->eps_r_bits) {
        HIP_TRY(ix->eps_r_bits.reset(2));
        HIP_TRY(hipMemsetAsync(ix->eps_r_bits, 0, 2 * sizeof(unsigned), st));
    }
    const bool norms = !metric_is_cosine(ix);  // (an ip or l2 index comes here through its filter leg only: the norms follow the shadow)
    if (norms && !ix->rmax_bits) {
        HIP_TRY(ix->rmax_bits.reset(1));
        HIP_TRY(hipMemsetAsync(ix->rmax_bits, 0, sizeof(unsigned), st));
    }
    if (need > ix->shadow8_rows) {
        // (every stream that may still read the old allocation has to be done with it)
        int rcw;
        if ((rcw = wait_searching_streams(ix)) != 0) return rcw;
        (void)ix->shadow8.reset();
        (void)ix->rscale.reset();
        (void)ix->bmeta.reset();
        ix->shadow8_rows = 0;
        const int64_t rows = need + need / 8;  // head room: appends do not reallocate every time
        const int64_t rows_al = (rows + kTileRows - 1) / kTileRows * kTileRows;
        // the three belong together: built in locals, handed over together (a failure leaves the index without an int8 shadow, not with a third of one)
        DevBuf<uint4> s8;
        DevBuf<float> rs;
        DevBuf<float2> bm;
        HIP_TRY(s8.reset(rows_al * dpad8 / (int64_t)sizeof(uint4)));
        HIP_TRY(rs.reset(rows_al));
        HIP_TRY(bm.reset(rows_al / 32 + 64));  // (+64: a wave's DMA reads 32 blocks from a tile's first one)
        if (norms) {
            (void)ix->rnorm2.reset();
            HIP_TRY(ix->rnorm2.reset(rows_al));
        }
        ix->shadow8 = std::move(s8);
        ix->rscale = std::move(rs);
        ix->bmeta = std::move(bm);
        HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)ix->bmeta.get(), (int)0x7fc00000, (size_t)(rows_al / 32 + 64) * 2, st));  // NaN: no such block yet
        ix->shadow8_rows = rows_al;
        // rows beyond the count are masked (row < n), their bytes only have to be defined
        HIP_TRY(hipMemsetAsync(ix->shadow8, 0, (size_t)rows_al * dpad8, st));
        HIP_TRY(hipMemsetAsync(ix->eps_r_bits, 0, 2 * sizeof(unsigned), st));
        first = 0; m = n;  // a fresh allocation holds nothing yet
    }
    HIP_TRY(ix->shadow8_ready.ensure());
    if (m > 0) {
        // Whole 32-row blocks (one scale per block): the rows that share a block with the dirty range are quantised again,
        // with the block's new scale, and the block's error norm is measured again.
        const int64_t last = first + m;
        first = first / 32 * 32;
        m = (last + 31) / 32 * 32 - first;
        const dim3 grid((unsigned)(m / 32)), block(256);
        uint4* s8 = ix->shadow8;
        const int rc = with_dtype(ix->dtype, [&](auto dt) {
            return launch_kernel<shadow8_from_rows_kernel<dt>>(grid, block, 0, st, ix->rows, first, n, ix->dpad, dpad8, s8, ix->rscale, ix->bmeta);
        });
        if (rc != 0) return rc;
        HIP_TRY(hipGetLastError());
        // the device-wide maximum of the block error norms, over the rows stored now (not a running maximum)
        hipLaunchKernelGGL(eps_max_kernel, dim3(1), dim3(1024), 0, st, ix->bmeta, (n + 31) / 32, ix->eps_r_bits, ix->shadow8_max_eps);
        HIP_TRY(hipGetLastError());
        if (norms) {  // the same rows' sums of squares, and the bound on every row's norm
            const int64_t mn = first + m > n ? n - first : m;
            const int rcn = with_dtype(ix->dtype, [&](auto dt) {
                return launch_kernel<row_sqnorm_kernel<dt>>(dim3((unsigned)((mn + 3) / 4)), block, 0, st, ix->rows, first, mn, ix->dpad, ix->rnorm2, ix->rmax_bits);
            });
            if (rcn != 0) return rcn;
            HIP_TRY(hipGetLastError());
        }
    }
    {
        // i8_tile_kernel reads whole tiles of scales: rows past the count carry NaN (`acc * NaN >= thr` is false for every
        // threshold, so its epilogue needs no row < count test).  Rows appended later get real scales from the build above.
        const int64_t pad = need - n;
        if (pad > 0) HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)(ix->rscale + n), (int)0x7fc00000, (size_t)pad, st));
    }
    HIP_TRY(hipEventRecord(ix->shadow8_ready, st));
    if (!ix->eps_r_host) {
        HIP_TRY(ix->eps_r_host.reset(2));
        ix->eps_r_host[0] = 0.0f;
        ix->eps_r_host[1] = 0.0f;
        HIP_TRY(ix->eps_r_copied.ensure());
    }
    HIP_TRY(hipMemcpyAsync(ix->eps_r_host, ix->eps_r_bits, 2 * sizeof(float), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipEventRecord(ix->eps_r_copied, st));
    ix->shadow8_stream = st;
    ix->shadow8_epoch = ix->epoch;
    ix->dirty_lo = ix->dirty_hi = 0;
    ix->stat_shadow8_builds++;
    return CODD_KNN_OK;
}

// The program a filter pass runs, chosen once per pass (filter_program); its sample launch and its filter launch both read it.
//   GEMM      gemm_filter_kernel<MODE, nbq, el, res>: el = 1 int8 operands; res = 1 the whole int8 query block resident in LDS,
//             res = 2 two of its six slices (768 elements, 4 query blocks)
//   TILE      i8_tile_kernel<MODE, ts, 2 * nbq, res> (filter_i8.h: the int8 tile program, 16-query blocks; res: the query block
//             resident in LDS); the sample pass runs ts = 0
//   TILE_F16  i8_tile_kernel<MODE_FILTER, ts, 16, false, true>: the same program on fp16 operands; the sample pass is GEMM's
//             gemm_filter_kernel<MODE_SAMPLE, 8>
struct FilterProgram {
    enum Family { GEMM, TILE, TILE_F16 };
    Family family = GEMM;
    int nbq = 8;  // 32-query blocks the GEMM multiplies
    int ts = 0, res = 0, el = 0;
    bool sqd = false;  // sqd_filter_kernel<MODE, nbq>: the squared-distance epilogue of an l2 index
};

FilterProgram filter_program(const codd_knn_index* ix, int nq, int nsteps, bool use8) {
    FilterProgram p;
    p.nbq = nq <= 32 ? 1 : (nq <= 64 ? 2 : (nq <= 128 ? 4 : 8));
    p.el = use8 ? 1 : 0;
    // an ip or l2 index: the GEMM family on int8 operands whatever "i8v2" / "f16_tile" say — the tile programs evaluate
    // the per-block, unit-norm form of the bound — and for l2 its staged form with the squared-distance epilogue
    const bool space = !metric_is_cosine(ix);
    p.sqd = space && ix->metric == CODD_KNN_METRIC_L2;
    const bool resident = use8 && nsteps <= 4 && ix->resident_q && !p.sqd;
    // 65..128 queries only: with <= 64 the kernel is a byte stream (nothing to gain); with 8 query blocks the six-step body
    // needs more than the 256 registers of a wave (hipcc spills, no gain measured)
    const bool partial6 = use8 && nsteps == 6 && nq > 64 && nq <= 128 && ix->resident_q && !p.sqd;
    // full query blocks: the second-generation int8 kernel (filter_i8.h); rows whose query block fits the LDS keep the resident one
    const bool tile_v2 = !space && use8 && (p.nbq == 8 || (p.nbq == 4 && ix->i8v2_half)) && ((ix->i8v2 == 1 && !resident && nsteps >= 3) || (ix->i8v2 == 2 && nsteps >= 3));
    // the 2-byte filter (dense clusters the int8 slack cannot separate, the int8 filter switched off): the same tile program on fp16 operands
    const bool tile_f16 = !space && CODD_SHADOW_F16 && CODD_MFMA16 && !use8 && p.nbq == 8 && nsteps % 6 == 0 && ix->f16_tile;
    if (tile_f16) {
        p.family = FilterProgram::TILE_F16;
        // rows of 768 elements are 12 K-steps of 64, rows of 384 are 6: the static forms of the tile program ("i8_pair" = 2); 18, 24, ...: run-time cursors
        if (nsteps == 12 && ix->i8_pair == 2) p.ts = 4;
        else if (nsteps == 6 && ix->i8_pair == 2) p.ts = 3;
        else p.ts = 2;
    } else if (tile_v2) {
        p.family = FilterProgram::TILE;
        p.res = i8_tile_resident(nsteps, p.nbq) && ix->resident_q;  // the query block fits the four LDS slices: loaded once per workgroup
        // tile structure: rows of 6, 12, ... K-steps (768 elements: the headline shape) run the staged program with one barrier
        // per TWO K-steps; other multiples of 3 one per K-step; the rest the generic interval loop
        // ("i8_pair" = 2, the default: rows of exactly 6 K-steps take that program with every cursor a compile-time constant)
        const bool pair = nsteps % 6 == 0 && ix->i8_pair;
        const bool static6 = nsteps == 6 && ix->i8_pair == 2;
        if (p.res) p.ts = nsteps % 3 == 0 ? 1 : 0;
        else if (static6) p.ts = 3;
        else if (pair) p.ts = 2;
        else p.ts = nsteps % 3 == 0 ? 1 : 0;
    } else if (partial6) {  // 768 int8 elements: two of the six query slices stay in LDS
        p.res = 2;
    } else if (resident) {  // the whole int8 query block fits the LDS slices: loaded once per workgroup
        p.res = 1;
    }
    return p;
}

// the arguments gemm_filter_kernel and i8_tile_kernel share, in their order; each launch expands them into its kernel's list
struct FilterArgs {
    const uint4* shadow;
    const uint4* qfrag;
    int64_t n;
    int nsteps;
    int64_t ntiles_run, tile_stride;
    const float* thr;
    u64* bucket_key;
    u64* hits;
    unsigned* hit_cnt;
    int cap_q;
    unsigned* flags;
    const float* rscale;  // int8 operands only
    const float* qscale;
    const float2* bmeta;  // i8_tile_kernel only
    float eb_scale;
    const float* rnorm2 = nullptr;  // sqd_filter_kernel only: the rows' and the queries' sums of squares
    const float* qn2 = nullptr;
};

// one launch of program `p` in pass MODE (MODE_SAMPLE or MODE_FILTER)
template <int MODE>
int launch_filter_program(const FilterProgram& p, dim3 grid, hipStream_t st, const FilterArgs& a) {
    using No = std::false_type;
    using Yes = std::true_type;
    const dim3 block(kFilterThreads);
    auto gemm = [&](auto nbq, auto el, auto res) {
        return launch_kernel<gemm_filter_kernel<MODE, nbq, el, res>>(grid, block, filter_lds_bytes(MODE), st, a.shadow, a.qfrag, a.n, a.nsteps,
                                                                     a.ntiles_run, a.tile_stride, a.thr, a.bucket_key, a.hits, a.hit_cnt, a.cap_q,
                                                                     a.flags, (float*)nullptr, a.rscale, a.qscale);
    };
    auto tile = [&](auto ts, auto nqb, auto res, auto f16) {
        return launch_kernel<i8_tile_kernel<MODE, ts, nqb, res, f16>>(grid, block, i8_lds_bytes(MODE), st, a.shadow, a.qfrag, a.n, a.nsteps,
                                                                      a.ntiles_run, a.tile_stride, a.thr, a.bucket_key, a.hits, a.hit_cnt, a.cap_q,
                                                                      a.flags, a.rscale, a.qscale, a.bmeta, a.eb_scale);
    };
    if (p.sqd) {
        return with_nbq(p.nbq, [&](auto nbq) {
            return launch_kernel<sqd_filter_kernel<MODE, nbq>>(grid, block, filter_lds_bytes(MODE), st, a.shadow, a.qfrag, a.n, a.nsteps, a.ntiles_run,
                                                               a.tile_stride, a.thr, a.bucket_key, a.hits, a.hit_cnt, a.cap_q, a.flags, (float*)nullptr, a.rscale,
                                                               a.qscale, a.rnorm2, a.qn2);
        });
    }
    if (p.family == FilterProgram::TILE) {
        return with_int<4, 8>(p.nbq, "bad query block count%s", [&](auto nbq) {
            const IntC<2 * decltype(nbq)::value> nqb;
            if constexpr (MODE == MODE_SAMPLE) {
                // (the sample pass keeps the generic program: its tile-structured instantiations — the static six-step one too, tried in round 3 —
                //  spill inside the loop: the fold's registers on top of two corpus ring slots in flight)
                return p.res ? tile(IntC<0>{}, nqb, Yes{}, No{}) : tile(IntC<0>{}, nqb, No{}, No{});
            } else if (p.res) {  // (the pair programs stage the query block)
                return with_int<0, 1>(p.ts, "bad tile program%s", [&](auto ts) { return tile(ts, nqb, Yes{}, No{}); });
            } else {
                return with_int<0, 1, 2, 3>(p.ts, "bad tile program%s", [&](auto ts) { return tile(ts, nqb, No{}, No{}); });
            }
        });
    }
    if constexpr (MODE == MODE_FILTER) {
        if (p.family == FilterProgram::TILE_F16)
            return with_int<2, 3, 4>(p.ts, "bad tile program%s", [&](auto ts) { return tile(ts, IntC<16>{}, No{}, Yes{}); });
    }
    // GEMM (and TILE_F16's sample pass: 8 query blocks, 2-byte operands)
    if (p.el == 0) return with_nbq(p.nbq, [&](auto nbq) { return gemm(nbq, IntC<0>{}, IntC<0>{}); });
    if (p.res == 2) return gemm(IntC<4>{}, IntC<1>{}, IntC<2>{});
    return with_nbq(p.nbq, [&](auto nbq) { return p.res ? gemm(nbq, IntC<1>{}, IntC<1>{}) : gemm(nbq, IntC<1>{}, IntC<0>{}); });
}

// The list-driven exact-scan fallback: at most one workgroup per compute unit (bounds the queue's partial buffer) and the
// buffer of its per-block partials.
int fallback_geometry(codd_knn_index* ix, int k, int64_t* blocks, int64_t* stride_q) {
    int niter, rc;
    if ((rc = scan_geometry(ix, ix->count, &niter, blocks)) != 0) return rc;
    if (*blocks > ix->num_cus) *blocks = ix->num_cus;
    *stride_q = *blocks * k;
    HIP_TRY(ix->fb_partial.ensure((int64_t)kTileQ * *stride_q));
    return CODD_KNN_OK;
}

// exact-scan fallback for the queries a pass queued (normally none), entirely on the device and in ONE launch: the scan walks
// the queue (an empty queue costs one empty launch), its last block merges the per-block partials and writes each answer into
// its query's slot.  No host round trip: the whole search stays asynchronous on `st`.
int listed_fallback(codd_knn_index* ix, const float* qn, int k, uint32_t row_base, u64* keys_out, float* dist_out, int64_t* rows_out,
                    hipStream_t st, const uint32_t* deny, int metric = kMetricDot) {
    int64_t blocks, stride_q;
    int rc;
    if ((rc = fallback_geometry(ix, k, &blocks, &stride_q)) != 0) return rc;
    if (metric == kMetricL2) {  // the list-driven squared-distance scan (the dense l2 scans take no query list)
        FilterCtl* c = ix->ctl;
        {
            EvScope ev(ix, EV_SCAN, st);
            rc = with_row_form(ix, k, "row too wide for the listed squared-distance scan%s", [&](auto dt, auto ni, auto sl) {
                if constexpr (decltype(ni)::value == kWideRows) {
                    return fail(CODD_KNN_ENOTSUP, "row too wide for the listed squared-distance scan%s");
                } else {
                    return launch_kernel<sqd_listed_scan_kernel<dt, ni, sl>>(dim3((unsigned)blocks), dim3(256), (size_t)4 * 4 * decltype(sl)::value * kWave * sizeof(u64), st,
                                                                            ix->rows, ix->count, ix->dpad, qn, k, row_base, ix->fb_partial, stride_q, c->fb_list,
                                                                            &c->fb_count, &c->fb_done, keys_out, dist_out, rows_out, &ix->dstats[2], deny);
                }
            });
        }
        if (rc != 0) return rc;
        HIP_TRY(hipGetLastError());
        return CODD_KNN_OK;
    }
    ScanArgs a{ix->rows, ix->count, ix->dpad, qn, 0, k, row_base, ix->fb_partial, stride_q, ix->ctl->fb_list, &ix->ctl->fb_count};
    a.merge_done = &ix->ctl->fb_done;
    a.merged_keys = keys_out;
    a.merged_dist = dist_out;
    a.merged_rows = rows_out;
    a.count_total = &ix->dstats[2];
    a.dead = deny;
    {
        EvScope ev(ix, EV_SCAN, st);
        rc = launch_scan(ix->dtype, 8, niter_of(ix), dim3((unsigned)blocks), st, a);
    }
    if (rc != 0) return rc;
    HIP_TRY(hipGetLastError());
    return CODD_KNN_OK;
}

// one pass of <= 256 queries through sample -> threshold -> filter -> finalize (+ exact fallback)
// keys_out and / or (dist_out, rows_out): what the caller wants written per query (any may be null)
int filter_pass(codd_knn_index* ix, const float* qn, int nq, int k, uint32_t row_base, u64* keys_out, float* dist_out, int64_t* rows_out,
                hipStream_t st, const uint32_t* deny, bool prepared = false, bool use8 = false) {
    const int64_t n = ix->count;
    const int nsteps = use8 ? dpad8_of(ix) / 128 : ix->dpad / 64;
    const uint4* shadow = use8 ? ix->shadow8 : ix->shadow;
    const uint4* qfrag = use8 ? ix->qfrag8 : ix->qfrag;
    const float* slack_q = use8 ? ix->qmeta + 256 : nullptr;  // int8: 2*eps per query, written by prep_queries8_kernel
    const float* rscale = use8 ? ix->rscale : nullptr;
    const float* qscale = use8 ? ix->qmeta : nullptr;
    const bool cosine = metric_is_cosine(ix);
    if (use8) ix->stat_shadow8_passes++;
    const int64_t ntiles = (n + kTileRows - 1) / kTileRows;
    const int slots = k <= 64 ? 1 : 2;
    const float eps = filter_eps(ix);
    int rc;
    ix->stat_filter_passes++;

    if (!prepared) {  // (a batch of <= 256 queries arrives with its fragments and a cleared control block: prep_queries_kernel)
        hipLaunchKernelGGL(qfrag_kernel, dim3((kTileQ * (ix->dpad / 8) + 255) / 256), dim3(256), 0, st, qn, nq, ix->dpad, ix->qfrag,
                           reinterpret_cast<unsigned*>(ix->ctl.get()), (int)(sizeof(FilterCtl) / 4));
        HIP_TRY(hipGetLastError());
    }

    const FilterProgram prog = filter_program(ix, nq, nsteps, use8);
    if (prog.family == FilterProgram::TILE) ix->stat_i8v2_passes++;
    if (prog.family == FilterProgram::TILE_F16) ix->stat_f16_tile_passes++;
    // sample: every `stride`-th tile
    const int64_t ts = sample_tile_count(ix, ntiles, k, use8, prog.nbq);
    const int64_t stride = ntiles / ts;
    {
        EvScope ev(ix, EV_SAMPLE, st);
        const dim3 g((unsigned)(ts < ix->num_cus ? ts : ix->num_cus));
        FilterArgs sa{shadow, qfrag, n, nsteps, ts, stride, nullptr, ix->bucket_max, nullptr, nullptr, 0, nullptr, rscale, qscale, nullptr, 1.0f};
        if (prog.sqd) { sa.rnorm2 = ix->rnorm2; sa.qn2 = ix->qmeta + 512; }
        if ((rc = launch_filter_program<MODE_SAMPLE>(prog, g, st, sa)) != 0) return rc;
    }
    HIP_TRY(hipGetLastError());
    // thresholds anchored on the exact scores of the k best sampled rows (anchor_thr_kernel)
    rc = with_row_form(ix, k, "row too wide for the threshold kernel%s", [&](auto dt, auto ni, auto sl) {
        if constexpr (decltype(ni)::value != kWideRows) {
            if (prog.sqd)
                return launch_kernel<sqd_thr_kernel<dt, ni, sl>>(dim3(kTileQ), dim3(kAnchorWaves * kWave), 0, st, ix->bucket_max, ts, nq, k, ix->rows, ix->dpad,
                                                                        qn, slack_q, ix->thr, deny);
        }
        return launch_kernel<anchor_thr_kernel<dt, ni, sl>>(dim3(kTileQ), dim3(kAnchorWaves * kWave), 0, st, ix->bucket_max, ts, nq, k, ix->rows,
                                                            ix->dpad, qn, eps, slack_q, ix->thr, use8 ? ix->thr + kTileQ : nullptr, deny);
    });
    if (rc != 0) return rc;
    HIP_TRY(hipGetLastError());
    {
        EvScope ev(ix, EV_FILTER, st);
        const dim3 g((unsigned)(ntiles < ix->num_cus ? ntiles : ix->num_cus));
        FilterArgs fa{shadow, qfrag, n, nsteps, ntiles, 1, ix->thr, nullptr, ix->hits, ix->ctl->hit_cnt, ix->hit_cap_q, ix->ctl->flags, rscale, qscale, nullptr, 0.0f};
        if (prog.sqd) { fa.rnorm2 = ix->rnorm2; fa.qn2 = ix->qmeta + 512; }
        if (prog.family == FilterProgram::TILE) {
            // the per-block bound (per_block & 1): thr0[q] and the blocks' error norms
            fa.thr = (ix->per_block & 1) ? ix->thr + kTileQ : ix->thr;
            fa.bmeta = ix->bmeta;
            fa.eb_scale = (ix->per_block & 1) ? 1.0f : 0.0f;
#ifdef CODD_I8_EXP_STAMPS  // (diagnostic build: the filter pass writes its per-wave phase stamps over the sample's bucket keys, which anchor_thr has consumed)
            fa.bucket_key = ix->bucket_max;
#endif
        } else if (prog.family == FilterProgram::TILE_F16) {
            // (thr doubles as the 256 readable bytes the kernel's per-tile metadata request needs; fp16 operands carry no scales)
            fa.bmeta = reinterpret_cast<const float2*>(ix->thr.get());
        }
        if ((rc = launch_filter_program<MODE_FILTER>(prog, g, st, fa)) != 0) return rc;
    }
    HIP_TRY(hipGetLastError());
    const int niter = niter_of(ix);
    // the int8 filter leaves thousands of survivors per query and is only used for a handful of queries: share each
    // query's re-scoring out between several workgroups, then merge their lists
    const int nparts = use8 ? (nq <= 8 ? 16 : (nq <= 32 ? 8 : (nq <= 64 ? 4 : 1))) : 1;
    ix->stat_last_finalize_parts = nparts;
    if (nparts > 1) HIP_TRY(ix->partial.ensure((int64_t)nq * nparts * k));
    const float2* bm = slack_q && (ix->per_block & 2) && cosine ? ix->bmeta : nullptr;  // (the int8 passes: slack per 32-row block; ip, l2: the device-wide bound)
    FilterCtl* c = ix->ctl;
    // one list slot per lane and one workgroup per query (the large batches): finalize and the exact-scan fallback share ONE
    // launch — the scan workgroups derive the queue from the hit counters and leave at once when it is empty
    if (slots == 1 && nparts == 1 && ix->fuse_fallback && niter <= 4 && !(ix->dtype != DT_F32 && niter == 4) && !prog.sqd) {  // (2-byte rows above 1536 elements: the fused kernel spills; wide rows take the separate fallback launch)
        int64_t blocks, stride_q;
        if ((rc = fallback_geometry(ix, k, &blocks, &stride_q)) != 0) return rc;
        EvScope ev(ix, EV_FINALIZE, st);
        const dim3 grid((unsigned)(nq + blocks), 1);
        const size_t lds = (size_t)(kFinThreads / kWave) * 4 * kWave * sizeof(u64);   // the scan role's lists: 8 waves x 4 queries x 64 keys
        rc = with_dtype(ix->dtype, [&](auto dt) {
            return with_niter(niter, "row too wide for the finalize kernel%s", [&](auto ni) {
                if constexpr (decltype(ni)::value == kWideRows) {
                    return fail(CODD_KNN_ENOTSUP, "row too wide for the finalize kernel%s");
                } else {
                    return launch_kernel<finalize_fb_kernel<decltype(dt)::value, ni>>(
                        grid, dim3(kFinThreads), lds, st, ix->rows, ix->dpad, qn, ix->hits, c->hit_cnt, ix->hit_cap_q, c->flags, k, 2.0f * eps, row_base,
                        keys_out, ix->dstats, slack_q, (u64*)nullptr, dist_out, rows_out, bm, nq, n, ix->fb_partial, stride_q, &c->fb_done, deny);
                }
            });
        });
        if (rc != 0) return rc;
        HIP_TRY(hipGetLastError());
        return CODD_KNN_OK;
    }
    {
        EvScope ev(ix, EV_FINALIZE, st);
        rc = with_row_form(ix, k, "row too wide for the finalize kernel%s", [&](auto dt, auto ni, auto sl) {
            if constexpr (decltype(ni)::value != kWideRows) {
                if (prog.sqd)
                    return launch_kernel<sqd_fin_kernel<dt, ni, sl>>(dim3(nq, nparts), dim3(kFinThreads), 0, st, ix->rows, ix->dpad, qn, ix->hits, c->hit_cnt,
                                                                          ix->hit_cap_q, c->flags, k, row_base, keys_out, &c->fb_count, c->fb_list, ix->dstats, slack_q,
                                                                          ix->partial, dist_out, rows_out, deny);
            }
            return launch_kernel<finalize_kernel<dt, ni, sl>>(dim3(nq, nparts), dim3(kFinThreads), 0, st, ix->rows, ix->dpad, qn, ix->hits, c->hit_cnt,
                                                              ix->hit_cap_q, c->flags, k, 2.0f * eps, row_base, keys_out, &c->fb_count, c->fb_list,
                                                              ix->dstats, slack_q, ix->partial, dist_out, rows_out, bm, deny);
        });
    }
    if (rc != 0) return rc;
    HIP_TRY(hipGetLastError());
    const int km = prog.sqd ? kMetricL2 : kMetricDot;
    if (nparts > 1 && (rc = launch_merge(ix->partial, nq, (int64_t)nparts * k, (int64_t)nparts * k, k, keys_out, dist_out, rows_out, st, nullptr, nullptr, nullptr, 0, 0, km)) != 0)
        return rc;
    return listed_fallback(ix, qn, k, row_base, keys_out, dist_out, rows_out, st, deny, km);
}

// ---- one launch for a single query (small_batch_kernel) + the (normally empty) list-driven fallback scan ----
template <int DT, int NS>
int launch_small_batch(int64_t nunits, hipStream_t st, const codd_knn_index* ix, const float* dev_queries, int k, uint32_t row_base, u64* cand,
                       u64* out_keys, float* out_dist, int64_t* out_rows, const uint32_t* deny) {
    constexpr int E = DT == DT_F32 ? 4 : 8;
    constexpr int NITER = (NS * 128 / E + kWave - 1) / kWave;  // chunks of the PADDED row per lane (dpad <= NS * 128)
    constexpr int kWavesPerWg = kSbThreads / kWave;
    // one round of workgroups: as many as are resident at once (the last one to arrive answers the query)
    static std::atomic<int> per_cu{0};
    int nb = per_cu.load(std::memory_order_relaxed);
    if (nb == 0) {
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, (const void*)&small_batch_kernel<DT, NITER, NS>, kSbThreads, 0) != hipSuccess || nb < 1) nb = 1;
        if (nb > 2) nb = 2;
        (void)hipGetLastError();
        per_cu.store(nb, std::memory_order_relaxed);
    }
    int64_t G = (int64_t)nb * ix->num_cus;
    if (G * kWavesPerWg > nunits) G = (nunits + kWavesPerWg - 1) / kWavesPerWg;
    const dim3 grid((unsigned)G);
    u64* dropmax = cand + G * kWavesPerWg * kSbKeep;
    FilterCtl* c = ix->ctl;
    return launch_kernel<small_batch_kernel<DT, NITER, NS>>(grid, dim3(kSbThreads), 0, st, ix->shadow8, ix->bmeta, ix->rows, ix->count, ix->dim, ix->dpad,
                                                            dev_queries, k, row_base, ix->eps_r_bits, ix->qn, cand, dropmax, &c->sb_ticket, &c->fb_count,
                                                            c->fb_list, out_keys, out_dist, out_rows, ix->dstats, deny);
}
bool small_batch_applies(const codd_knn_index* ix, int B, int k) {
    const int ns = dpad8_of(ix) / 128;
    return ix->small_batch_max > 0 && B == 1 && k <= kWave && (ns == 3 || ns == 4 || ns == 6 || ns == 8) && ix->count >= 4096;
}
int small_batch_search(codd_knn_index* ix, const float* dev_queries, int B, int k, uint32_t row_base, u64* out_keys, float* out_dist, int64_t* out_rows,
                       hipStream_t st, const uint32_t* deny) {
    (void)B;
    const int ns = dpad8_of(ix) / 128;
    const int64_t n = ix->count;
    constexpr int kWavesPerWg = kSbThreads / kWave;
    const int64_t nunits = (n + 15) / 16;
    int rc;
    HIP_TRY(ix->sb_cand.ensure((int64_t)(2 * ix->num_cus) * kWavesPerWg * (kSbKeep + 1)));
    u64* cand = ix->sb_cand;
    ix->stat_small_batch++;
    {
        EvScope ev(ix, EV_FILTER, st);
        rc = with_dtype(ix->dtype, [&](auto dt) {
            return with_int<3, 4, 6, 8>(ns, "small batch: unsupported row width%s", [&](auto nsc) {
                return launch_small_batch<decltype(dt)::value, nsc>(nunits, st, ix, dev_queries, k, row_base, cand, out_keys, out_dist, out_rows, deny);
            });
        });
    }
    if (rc != 0) return rc;
    HIP_TRY(hipGetLastError());
    // a query the margin test could not clear (normally none): the list-driven exact scan, its last block merges
    return listed_fallback(ix, ix->qn, k, row_base, out_keys, out_dist, out_rows, st, deny);
}

bool filter_applies(const codd_knn_index* ix, int B, int k) {
    // the thresholds come from the k-th largest of the sampled tile maxima: need comfortably more tiles than k
    const int64_t ntiles = (ix->count + kTileRows - 1) / kTileRows;
    const int64_t ts = sample_tile_count(ix, ntiles, k);
    if (!(ix->filter_enabled && ix->all_normalized) || ts < 2 * (int64_t)k) return false;
    // measured on MI355X (scripts/crossover.py, d = 768): with more than 8 queries the filter wins at every size
    // it is sound for; up to 8 queries the exact scan's single launch wins until rows * B reaches ~100k
    if (B >= ix->filter_min_batch) return ix->count >= ix->filter_min_rows;
    return ix->count * (int64_t)B >= ix->filter_min_rows_small;
}

// The int8 filter leg of an ip or l2 index: opt-in ("space_filter"), batches of filter_min_batch queries and more
// over filter_min_rows rows and more whose sample holds 2k tiles, both "filter" and "shadow8" on, a build with the int8 MFMA.
// l2 rows wider than 4 chunks per lane stay on the scan.  No usefulness heuristic: a loose bound is slow, never wrong.
bool space_filter_applies(const codd_knn_index* ix, int B, int k) {
    if (metric_is_cosine(ix) || !ix->space_filter || !CODD_MFMA16 || !ix->filter_enabled || !ix->shadow8_enabled) return false;
    if (ix->metric == CODD_KNN_METRIC_L2 && niter_of(ix) > 4) return false;
    const int64_t ntiles = (ix->count + kTileRows - 1) / kTileRows;
    if (sample_tile_count(ix, ntiles, k) < 2 * (int64_t)k) return false;
    return B >= ix->filter_min_batch && ix->count >= ix->filter_min_rows;
}

int launch_prep_raw(codd_knn_index* ix, const float* dev_queries, int nq, float* qn, hipStream_t st) {
    hipLaunchKernelGGL(prep_queries8_raw_kernel, dim3(kTileQ / 4), dim3(256), 0, st, dev_queries, nq, ix->dim, ix->dpad, dpad8_of(ix), qn,
                       reinterpret_cast<uint32_t*>(ix->qfrag8.get()), ix->qmeta, ix->eps_r_bits, ix->rmax_bits, reinterpret_cast<unsigned*>(ix->ctl.get()),
                       (int)(sizeof(FilterCtl) / 4), ix->metric == CODD_KNN_METRIC_L2 ? 1 : 0);
    HIP_TRY(hipGetLastError());
    return CODD_KNN_OK;
}

// what an int8 pass of an ip or l2 index needs beside the rows: the workspace, the shadow with the rows' norms, the query buffers
int ensure_space_filter(codd_knn_index* ix, hipStream_t st) {
    int rc;
    if ((rc = ensure_filter_workspace(ix)) != 0) return rc;
    if ((rc = ensure_shadow8(ix, st)) != 0) return rc;
    HIP_TRY(ix->qfrag8.ensure((int64_t)kTileQ * (dpad8_of(ix) / 16)));
    if (!ix->qmeta) HIP_TRY(ix->qmeta.reset(1024));
    return CODD_KNN_OK;
}

// ... and the search: ceil(B / 256) passes, each with its own preparation.  The survivor watch, the cooldown and the eps_r switch to
// the 2-byte filter never engage: they are unit-norm quantities, and the 2-byte filter's analytic bound does not hold here.
int space_filter_search(codd_knn_index* ix, const float* dev_queries, int B, int k, uint32_t row_base, u64* out_keys, float* out_dist, int64_t* out_rows,
                        hipStream_t st, const uint32_t* deny) {
    int rc;
    if ((rc = ensure_space_filter(ix, st)) != 0) return rc;
    for (int q0 = 0; q0 < B; q0 += kTileQ) {
        const int nq = B - q0 < kTileQ ? B - q0 : kTileQ;
        float* qn = ix->qn + (int64_t)q0 * ix->dpad;
        if ((rc = launch_prep_raw(ix, dev_queries + (int64_t)q0 * ix->dim, nq, qn, st)) != 0) return rc;
        if ((rc = filter_pass(ix, qn, nq, k, row_base, out_keys ? out_keys + (int64_t)q0 * k : nullptr, out_dist ? out_dist + (int64_t)q0 * k : nullptr,
                              out_rows ? out_rows + (int64_t)q0 * k : nullptr, st, deny, true, true)) != 0)
            return rc;
    }
    return CODD_KNN_OK;
}

// the index looks at its own device counters now and then (one look in flight; after its first 32 searches only every 8th:
// the copy is a launch of its own on the searching stream)
int after_filter_search(codd_knn_index* ix, int B, bool use8, hipStream_t st) {
    (use8 ? ix->watch_q8 : ix->watch_q16) += B;
    if (ix->shadow8_enabled && !ix->watch_pending && ix->dstats && (ix->stat_searches <= 32 || (ix->stat_searches & 7) == 0)) {
        if (!ix->watch_host) {
            HIP_TRY(ix->watch_host.reset(4));
            HIP_TRY(ix->watch_copied.ensure());
        }
        HIP_TRY(hipMemcpyAsync(ix->watch_host, ix->dstats, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipEventRecord(ix->watch_copied, st));
        ix->watch_pending = true;
        ix->watch_q8_sent = ix->watch_q8;
        ix->watch_q16_sent = ix->watch_q16;
    }
    return CODD_KNN_OK;
}

// the whole shard-local search: normalise queries, then filter passes or exact scans, keys out.
// deny: the rows no answer may hold — ix->dead_bits, or, `masked`, the ~allow | dead of a masked search's dense route (DESIGN.md
// §15).  A masked search says nothing about the corpus: it neither feeds the filter watch nor uses up a cooldown.
int search_impl(codd_knn_index* ix, const float* dev_queries, int B, int k, uint32_t row_base, u64* out_keys,
                float* out_dist, int64_t* out_rows, hipStream_t st, const uint32_t* deny, bool masked = false) {
    if (!ix) return fail(CODD_KNN_EINVAL, "null index%s");
    if (!dev_queries) return fail(CODD_KNN_EINVAL, "null queries%s");
    if (B < 1 || B > CODD_KNN_MAX_BATCH) return fail(CODD_KNN_EINVAL, "B out of range [1,1024]%s");
    if (k < 1 || k > CODD_KNN_MAX_K) return fail(CODD_KNN_EINVAL, "k out of range [1,128]%s");
    DeviceGuard guard(ix->device);
    ix->stat_searches++;
    const int64_t n = ix->count;
    int rc;
    HIP_TRY(ix->qn.ensure((int64_t)B * ix->dpad));
    HIP_TRY(ix->keys_tmp.ensure((int64_t)B * k));
    if ((rc = wait_rows(ix, st)) != 0) return rc;
    if (n > 0 && space_filter_applies(ix, B, k)) return space_filter_search(ix, dev_queries, B, k, row_base, out_keys, out_dist, out_rows, st, deny);
    bool use_filter = n > 0 && filter_applies(ix, B, k);
    if (ix->eps_r_copied) {
        if (hipEventQuery(ix->eps_r_copied) == hipSuccess) {
            ix->eps_r_known = ix->eps_r_host[0];
            ix->wide_blocks_known = (int64_t)reinterpret_cast<const unsigned*>(ix->eps_r_host.get())[1];
        }
        else (void)hipGetLastError();  // "not ready" must not surface in a later error check
    }
    if (ix->watch_pending && ix->watch_copied) {
        if (hipEventQuery(ix->watch_copied) == hipSuccess) {
            ix->watch_pending = false;
            const unsigned long long surv = ix->watch_host[1], fb = ix->watch_host[2];
            if (ix->watch_q8_sent > 0 && ix->watch_q16_sent == 0) {  // only int8 passes in the window: the deltas are theirs
                const double per_q = (double)(surv - ix->watch_surv) / (double)ix->watch_q8_sent;
                if ((per_q > (double)ix->shadow8_max_surv || (fb - ix->watch_fb) * 20 > (unsigned long long)ix->watch_q8_sent) &&
                    ix->cooldown_useless_epoch != ix->epoch) {
                    ix->cooldown_left = ix->shadow8_cooldown;
                    ix->cooldown_surv8 = per_q;  // what the 2-byte filter has to beat
                    ix->stat_cooldowns++;
                }
            } else if (ix->watch_q16_sent > 0 && ix->watch_q8_sent == 0) {
                // only bf16 passes (a cooldown): when those leave the re-scoring just as crowded — rows closer to each other than
                // EITHER slack — the slower bf16 kernel buys nothing: stay on int8 until rows change
                // (relative, not absolute: the fp16 filter's passes cost about twice an int8 pass, so they pay as soon as they
                // leave well under half of the exact re-scoring — 7,000 survivors per query are a bargain against 62,000)
                const double per_q = (double)(surv - ix->watch_surv) / (double)ix->watch_q16_sent;
                if (per_q > (double)ix->shadow8_max_surv && per_q > 0.5 * ix->cooldown_surv8) {
                    ix->cooldown_useless_epoch = ix->epoch;
                    ix->cooldown_left = 0;
                }
            }
            ix->watch_surv = surv;
            ix->watch_fb = fb;
            ix->watch_q8 -= ix->watch_q8_sent;
            ix->watch_q16 -= ix->watch_q16_sent;
        } else {
            (void)hipGetLastError();
        }
    }
    const bool cooling = ix->cooldown_left > 0;
    if (cooling && use_filter && !masked) ix->cooldown_left--;
    // the int8 filter: every pass of <= 256 queries prepares its own block (a batch above 256 queries is several passes)
    const bool can8 = use_filter && ix->shadow8_enabled && (B <= ix->shadow8_max_batch || (B > kTileQ && ix->shadow8_max_batch >= kTileQ)) && CODD_MFMA16;
    // A corpus whose WORST block quantises badly keeps the int8 filter for the batches i8_tile_kernel takes as long as such blocks are
    // rare (under 1 %): that kernel and finalize evaluate the bound per 32-row block, so only the bad blocks' rows come through
    // as extra candidates.  The first-generation kernels (other batch sizes, rows under 384 elements) use the device-wide bound.
    const int nsteps8 = dpad8_of(ix) / 128;
    const bool per_block = ix->i8v2 != 0 && nsteps8 >= 3 && B > 64 && (B <= 128 ? ix->i8v2_half != 0 : B <= kTileQ) && (ix->i8v2 == 2 || nsteps8 > 4 || !ix->resident_q);
    const bool eps_ok = ix->eps_r_known <= ix->shadow8_max_eps || (per_block && ix->wide_blocks_known * 100 <= (ix->count + 31) / 32);
    bool use8 = can8 && !cooling && eps_ok;
    if (use_filter && !use8) {
        // the bf16 filter: its shadow is allocated by the first search that needs it.  When HBM cannot hold it the search is
        // still answered exactly — through the int8 filter where the index may use it (a cooldown or a wide eps_r only make
        // that one slower), else by the exact scan — and the failed allocation is not retried until rows change.
        if ((rc = ensure_filter_workspace(ix)) != 0) return rc;
        rc = ensure_shadow(ix, st);
        if (rc == CODD_KNN_ENOMEM) {
            if (can8) use8 = true;
            else use_filter = false;
        } else if (rc != 0) {
            return rc;
        }
    }
    const bool fused_prep = use_filter && B <= kTileQ;
    const int dpad8 = dpad8_of(ix);
    auto prep8 = [&](int q0, int nq) -> int {
        hipLaunchKernelGGL(prep_queries8_kernel, dim3(kTileQ / 4), dim3(256), 0, st, dev_queries + (int64_t)q0 * ix->dim, nq, ix->dim, ix->dpad, dpad8,
                           ix->qn + (int64_t)q0 * ix->dpad, reinterpret_cast<uint32_t*>(ix->qfrag8.get()), ix->qmeta, ix->eps_r_bits,
                           reinterpret_cast<unsigned*>(ix->ctl.get()), (int)(sizeof(FilterCtl) / 4), ix->exp_slack_scale);
        HIP_TRY(hipGetLastError());
        return CODD_KNN_OK;
    };
    if (use8) {
        if ((rc = ensure_filter_workspace(ix)) != 0) return rc;
        if ((rc = ensure_shadow8(ix, st)) != 0) return rc;
        // a handful of queries: ONE launch streams the int8 shadow, keeps the best approximate scores per wave and re-scores the
        // survivors exactly in its last workgroup (small_batch_kernel) instead of the six-launch filter chain
        if (small_batch_applies(ix, B, k)) {
            HIP_TRY(ix->qn.ensure((int64_t)B * ix->dpad));
            if ((rc = small_batch_search(ix, dev_queries, B, k, row_base, out_keys, out_dist, out_rows, st, deny)) != 0) return rc;
            return masked ? CODD_KNN_OK : after_filter_search(ix, B, true, st);
        }
        HIP_TRY(ix->qfrag8.ensure((int64_t)kTileQ * (dpad8 / 16)));
        if (!ix->qmeta) HIP_TRY(ix->qmeta.reset(1024));
    } else if (fused_prep) {
        hipLaunchKernelGGL(prep_queries_kernel, dim3(kTileQ / 4), dim3(256), 0, st, dev_queries, B, ix->dim, ix->dpad, ix->qn,
                           reinterpret_cast<uint2*>(ix->qfrag.get()), reinterpret_cast<unsigned*>(ix->ctl.get()), (int)(sizeof(FilterCtl) / 4));
        HIP_TRY(hipGetLastError());
    } else if ((rc = prep_exact_queries(ix, dev_queries, B, st)) != 0) {
        return rc;
    }

    // the filter passes write what the caller asked for — packed keys (the shard-local half of a sharded search) and / or
    // (distance, row) — straight from finalize: no unpack launch behind them
    if (n == 0) {
        // nothing stored: all-empty result (chromadb returns {"ids": [[]], ...})
        u64* keys_dst = out_keys ? out_keys : ix->keys_tmp;
        HIP_TRY(hipMemsetAsync(keys_dst, 0, (size_t)B * k * sizeof(u64), st));
        if (!out_dist && !out_rows) return CODD_KNN_OK;
        return launch_merge(keys_dst, B, k, k, k, nullptr, out_dist, out_rows, st);
    }
    if (!use_filter)  // small batches: the per-block partials merge straight into the caller's buffers
        return exact_scan(ix, ix->qn, B, k, row_base, out_keys, out_dist, out_rows, st, deny);
    if ((rc = ensure_filter_workspace(ix)) != 0) return rc;
    for (int q0 = 0; q0 < B; q0 += kTileQ) {
        const int nq = B - q0 < kTileQ ? B - q0 : kTileQ;
        if (use8 && (rc = prep8(q0, nq)) != 0) return rc;
        if ((rc = filter_pass(ix, ix->qn + (int64_t)q0 * ix->dpad, nq, k, row_base, out_keys ? out_keys + (int64_t)q0 * k : nullptr,
                              out_dist ? out_dist + (int64_t)q0 * k : nullptr, out_rows ? out_rows + (int64_t)q0 * k : nullptr, st, deny,
                              fused_prep || use8, use8)) != 0)
            return rc;
    }
    return masked ? CODD_KNN_OK : after_filter_search(ix, B, use8, st);
}

// ---- scopes ----------------------------------------------------------------------------------

// the label array, as long as the row store, zero (= no label) until codd_knn_set_scopes_host writes it.  Only ever called with
// scope_of == nullptr or from an exclusive call: a live array is regrown by grow_rows alone.
int ensure_scope_labels(codd_knn_index* ix, hipStream_t st) {
    if (ix->scope_of && ix->scope_of.cap() >= ix->count) return CODD_KNN_OK;
    if (ix->scope_of) return fail(CODD_KNN_EDEVICE, "scope labels shorter than the row store%s");
    const int64_t cap = ix->capacity > ix->count ? ix->capacity : ix->count;
    if (cap < 1) return CODD_KNN_OK;
    HIP_TRY(ix->scope_of.reset(cap));
    HIP_TRY(hipMemsetAsync(ix->scope_of, 0, (size_t)cap * sizeof(uint32_t), st));
    return CODD_KNN_OK;
}

// The scope lists are derived data like the shadows: (re)built from the labels on the searching stream by the first scoped search
// after the labels or the row count changed.  Searches on other streams wait for the build on the device; the build waits for
// what they have already enqueued (their scans may still read the lists it overwrites).
int ensure_scope_lists(codd_knn_index* ix, hipStream_t st) {
    const int64_t n = ix->count;
    if (ix->scope_perm && ix->scope_built_gen == ix->scope_gen && ix->scope_built_count == n) {
        if (ix->scope_stream != st) HIP_TRY(hipStreamWaitEvent(st, ix->scope_ready, 0));
        return CODD_KNN_OK;
    }
    int rc;
    if ((rc = ensure_scope_labels(ix, st)) != 0) return rc;
    const int64_t nlist = (int64_t)ix->max_scope + 1;
    if (n > ix->scope_perm.cap() || 2 * nlist + 1 > ix->scope_offsets.cap()) {
        if ((rc = wait_searching_streams(ix)) != 0) return rc;   // (growth is the one place where a search call blocks)
        if (n > ix->scope_perm.cap()) HIP_TRY(ix->scope_perm.reset(ix->capacity > n ? ix->capacity : n));
        if (2 * nlist + 1 > ix->scope_offsets.cap()) {
            int64_t cap = 2049;
            while (cap < 2 * nlist + 1) cap = 2 * cap - 1;
            HIP_TRY(ix->scope_offsets.reset(cap));
        }
    }
    for (WorkSlot& w : ix->slots) {
        if (!w.used || w.stream == st) continue;
        HIP_TRY(w.handover.ensure());
        if (hipEventRecord(w.handover, w.stream) == hipSuccess) HIP_TRY(hipStreamWaitEvent(st, w.handover, 0));
        else (void)hipGetLastError();  // (a stream that no longer exists has nothing in flight)
    }
    if (ix->scope_ready && ix->scope_stream != st && ix->scope_built_gen >= 0) HIP_TRY(hipStreamWaitEvent(st, ix->scope_ready, 0));
    unsigned* start = ix->scope_offsets;
    unsigned* fill = start + nlist + 1;
    HIP_TRY(hipMemsetAsync(fill, 0, (size_t)nlist * sizeof(unsigned), st));
    const unsigned rb = (unsigned)((n + 255) / 256);
    hipLaunchKernelGGL(scope_count_kernel, dim3(rb), dim3(256), 0, st, ix->scope_of, n, (int)nlist, fill, ix->dead_bits);
    hipLaunchKernelGGL(scope_offsets_kernel, dim3(1), dim3(1024), 0, st, fill, (int)nlist, start);
    hipLaunchKernelGGL(scope_scatter_kernel, dim3(rb), dim3(256), 0, st, ix->scope_of, n, (int)nlist, start, fill, ix->scope_perm, ix->dead_bits);
    HIP_TRY(hipGetLastError());
    HIP_TRY(ix->scope_ready.ensure());
    HIP_TRY(hipEventRecord(ix->scope_ready, st));
    ix->scope_stream = st;
    ix->scope_built_gen = ix->scope_gen;
    ix->scope_built_count = n;
    ix->stat_scope_builds++;
    return CODD_KNN_OK;
}

// the IVF layout and its coarse index go (a new install, a failed one)
void drop_ivf(codd_knn_index* ix) {
    (void)ix->rows_ivf.reset();
    (void)ix->ivf_ids.reset();
    (void)ix->ivf_offsets.reset();
    (void)codd_knn_destroy(ix->coarse);
    ix->coarse = nullptr;
    ix->ivf_epoch = -1;
}

}  // namespace

extern "C" {

const char* codd_knn_version(void) {
    return "codd_knn 0.7.0 gfx950"
#if CODD_SHADOW_F16
           " shadow=f16"
#else
           " shadow=bf16"
#endif
#if CODD_MFMA16
           " mfma=16x16x32 int8=16x16x64";
#else
           " mfma=32x32x16";
#endif
}
const char* codd_knn_last_error(void) { return g_err; }

int codd_knn_create(codd_knn_index** out, int device, int dim, int dtype, int metric) {
    if (!out) return fail(CODD_KNN_EINVAL, "null out pointer%s");
    *out = nullptr;
    if (dim < 1 || dim > 4096) return fail(CODD_KNN_EINVAL, "dim out of range [1,4096]%s");
    if (dtype != DT_F32 && dtype != DT_BF16 && dtype != DT_F16) return fail(CODD_KNN_EINVAL, "unknown dtype%s");
    if (metric != CODD_KNN_METRIC_COSINE && metric != CODD_KNN_METRIC_IP && metric != CODD_KNN_METRIC_L2)
        return fail(CODD_KNN_ENOTSUP, "unknown metric (cosine 0, ip 1, l2 2)%s");
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail(CODD_KNN_EINVAL, "no such device%s");
    const int dpad = (dim + 63) / 64 * 64;
    codd_knn_index* ix = new (std::nothrow) codd_knn_index();
    if (!ix) return fail(CODD_KNN_ENOMEM, "host allocation failed%s");
    ix->device = device;
    ix->dim = dim;
    ix->dpad = dpad;
    ix->dtype = dtype;
    ix->metric = metric;
    // ip and l2 rows are no unit vectors, which both MFMA filters assume: such an index takes no filter leg, every batch the exact scan
    if (metric != CODD_KNN_METRIC_COSINE) ix->all_normalized = false;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) ix->num_cus = prop.multiProcessorCount;
    *out = ix;
    return CODD_KNN_OK;
}

int codd_knn_destroy(codd_knn_index* ix) {
    if (!ix) return CODD_KNN_OK;
    DeviceGuard guard(ix->device);
    (void)hipDeviceSynchronize();
    // (every buffer and event is a member that frees itself; the device is current and idle, as their destructors need)
    delete ix;
    return CODD_KNN_OK;
}

int codd_knn_reserve(codd_knn_index* ix, int64_t rows) {
    if (!ix || rows < 0) return fail(CODD_KNN_EINVAL, "bad reserve arguments%s");
    if (rows >= 0xffffffffll) return fail(CODD_KNN_EINVAL, "row slots must fit 32 bits%s");
    DeviceGuard guard(ix->device);
    if (rows <= ix->capacity) return CODD_KNN_OK;
    HIP_TRY(hipDeviceSynchronize());
    return grow_rows(ix, rows, /*exact=*/true);  // the caller states the final size (288 GB of HBM is the only limit)
}

int codd_knn_upsert_host(codd_knn_index* ix, const int64_t* host_slots, const float* host_vecs, int64_t n, int normalize) {
    if (!ix || (n > 0 && (!host_slots || !host_vecs)) || n < 0) return fail(CODD_KNN_EINVAL, "bad upsert arguments%s");
    if (n == 0) return CODD_KNN_OK;
    int64_t max_slot = -1, min_slot = INT64_MAX;
    for (int64_t i = 0; i < n; ++i) {
        if (host_slots[i] < 0 || host_slots[i] >= 0xfffffffell) return fail(CODD_KNN_EINVAL, "row slot out of range%s");
        if (slot_dead(ix, host_slots[i])) return fail(CODD_KNN_EINVAL, "upsert into a deleted row slot (it stays dead until codd_knn_compact)%s");
        if (host_slots[i] > max_slot) max_slot = host_slots[i];
        if (host_slots[i] < min_slot) min_slot = host_slots[i];
    }
    DeviceGuard guard(ix->device);
    HIP_TRY(hipDeviceSynchronize());
    int rc = grow_rows(ix, max_slot + 1, /*exact=*/false);
    if (rc != 0) return rc;
    // stage in bounded pieces (<= 64 MiB of vectors per piece) through buffers the index keeps between calls (the indexer job
    // upserts one small batch at a time: an allocation and a release per call used to dominate them)
    const int64_t piece = (int64_t)(64ll << 20) / ((int64_t)ix->dim * 4) + 1;
    const int64_t pn = n < piece ? n : piece;
    if (pn * ix->dim > ix->stage_vec.cap()) HIP_TRY(ix->stage_vec.reset(pn * ix->dim < 65536 ? 65536 : pn * ix->dim));
    if (pn > ix->stage_slot.cap()) HIP_TRY(ix->stage_slot.reset(pn < 4096 ? 4096 : pn));
    float* dvec = ix->stage_vec;
    int64_t* dslot = ix->stage_slot;
    rc = CODD_KNN_OK;
    for (int64_t i0 = 0; i0 < n && rc == 0; i0 += pn) {
        const int64_t m = n - i0 < pn ? n - i0 : pn;
        hipError_t e = hipMemcpy(dvec, host_vecs + i0 * ix->dim, (size_t)m * ix->dim * sizeof(float), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(dslot, host_slots + i0, (size_t)m * sizeof(int64_t), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            rc = fail(CODD_KNN_EDEVICE, "staging copy failed: %s", hipGetErrorString(e));
            break;
        }
        rc = launch_ingest(ix, dvec, m, normalize, dslot, 0, nullptr);
        // (one synchronisation per piece: the staging buffers are reused by the next piece, and the call is synchronous by contract)
        if (rc == 0 && hipDeviceSynchronize() != hipSuccess) rc = fail(CODD_KNN_EDEVICE, "ingest kernel failed%s");
    }
    ix->rows_event_set = false;  // (everything is complete on the device)
    ix->reader_event_set = false;
    if (rc == 0) {
        slots_written(ix, min_slot, max_slot + 1);
        if (!normalize) ix->all_normalized = false;
    }
    return rc;
}

int codd_knn_upsert_device(codd_knn_index* ix, int64_t first_slot, const float* dev_vecs, int64_t n, int normalize, void* stream) {
    if (!ix || n < 0 || first_slot < 0 || (n > 0 && !dev_vecs)) return fail(CODD_KNN_EINVAL, "bad upsert arguments%s");
    if (n == 0) return CODD_KNN_OK;
    if (first_slot + n >= 0xffffffffll) return fail(CODD_KNN_EINVAL, "row slots must fit 32 bits%s");
    if (range_has_dead(ix, first_slot, first_slot + n)) return fail(CODD_KNN_EINVAL, "upsert into a deleted row slot (it stays dead until codd_knn_compact)%s");
    DeviceGuard guard(ix->device);
    if (first_slot + n > ix->capacity) {
        HIP_TRY(hipDeviceSynchronize());
        int rc = grow_rows(ix, first_slot + n, /*exact=*/false);
        if (rc != 0) return rc;
    }
    hipStream_t wst = (hipStream_t)stream;
    // device-side ordering against searches still in flight on OTHER streams (the call is exclusive on the host, but their
    // kernels may still be reading the rows this launch overwrites): the writing stream waits for every searching stream
    for (WorkSlot& w : ix->slots) {
        if (!w.used || w.stream == wst) continue;
        HIP_TRY(w.handover.ensure());
        if (hipEventRecord(w.handover, w.stream) == hipSuccess) HIP_TRY(hipStreamWaitEvent(wst, w.handover, 0));
        else (void)hipGetLastError();  // (a stream that no longer exists has nothing in flight)
    }
    // ... and for the previous writer, when that was another stream: rows_ready is ONE event, re-recorded by every write, so
    // chaining the writers makes the last record cover every earlier write (a reader only ever waits for the last one)
    if (ix->rows_event_set && ix->rows_stream != wst) HIP_TRY(hipStreamWaitEvent(wst, ix->rows_ready, 0));
    // ... and for streams that only READ rows outside a search (codd_knn_copy_rows_f32)
    if (ix->reader_event_set && ix->reader_stream != wst) HIP_TRY(hipStreamWaitEvent(wst, ix->reader_done, 0));
    int rc = launch_ingest(ix, dev_vecs, n, normalize, nullptr, first_slot, wst);
    if (rc != 0) return rc;
    // ... and searches on other streams wait for this write (wait_rows)
    HIP_TRY(ix->rows_ready.ensure());
    HIP_TRY(hipEventRecord(ix->rows_ready, wst));
    ix->rows_stream = wst;
    ix->rows_event_set = true;
    slots_written(ix, first_slot, first_slot + n);
    if (!normalize) ix->all_normalized = false;
    return CODD_KNN_OK;
}

int codd_knn_load_rows(codd_knn_index* ix, int64_t first_slot, const void* host_rows, int64_t n) {
    if (!ix || first_slot < 0 || n < 0 || (n > 0 && !host_rows)) return fail(CODD_KNN_EINVAL, "bad load_rows arguments%s");
    if (n == 0) return CODD_KNN_OK;
    if (first_slot + n >= 0xffffffffll) return fail(CODD_KNN_EINVAL, "row slots must fit 32 bits%s");
    if (range_has_dead(ix, first_slot, first_slot + n)) return fail(CODD_KNN_EINVAL, "load_rows into a deleted row slot (it stays dead until codd_knn_compact)%s");
    DeviceGuard guard(ix->device);
    HIP_TRY(hipDeviceSynchronize());
    int rc = grow_rows(ix, first_slot + n, /*exact=*/false);
    if (rc != 0) return rc;
    const size_t row_bytes = (size_t)ix->dpad * elem_size(ix->dtype);
    HIP_TRY(hipMemcpy(ix->rows + (size_t)first_slot * row_bytes, host_rows, (size_t)n * row_bytes, hipMemcpyHostToDevice));
    if (!metric_is_cosine(ix)) {   // (ip, l2: rows of any norm, and no filter to keep on)
        ix->rows_event_set = false;
        slots_written(ix, first_slot, first_slot + n);
        return CODD_KNN_OK;
    }
    // the loaded rows are taken as they are, so their norms are checked: the filters stay on only for unit rows
    // (tolerance = the storage type's rounding of a unit vector)
    DevBuf<unsigned> dev_bits;
    HIP_TRY(dev_bits.reset(1));
    hipError_t e = hipMemset(dev_bits, 0, sizeof(unsigned));
    const dim3 grid((unsigned)((n + 3) / 4)), block(256);
    if (e == hipSuccess) {
        (void)with_dtype(ix->dtype, [&](auto dt) {
            return launch_kernel<row_norm_check_kernel<dt>>(grid, block, 0, nullptr, ix->rows, first_slot, n, ix->dpad, dev_bits);
        });
        e = hipGetLastError();
    }
    float worst = 0.0f;
    if (e == hipSuccess) e = hipMemcpy(&worst, dev_bits, sizeof(float), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(CODD_KNN_EDEVICE, "norm check of the loaded rows failed: %s", hipGetErrorString(e));
    const float tol = ix->dtype == DT_F32 ? 1e-4f : (ix->dtype == DT_BF16 ? 4e-3f : 6e-4f);
    if (!(worst <= tol)) ix->all_normalized = false;
    ix->rows_event_set = false;
    slots_written(ix, first_slot, first_slot + n);
    return CODD_KNN_OK;
}

int codd_knn_count(const codd_knn_index* ix, int64_t* out) {
    if (!ix || !out) return fail(CODD_KNN_EINVAL, "bad count arguments%s");
    *out = ix->count;
    return CODD_KNN_OK;
}

int codd_knn_dim(const codd_knn_index* ix, int* dim, int* padded_dim, int* dtype) {
    if (!ix) return fail(CODD_KNN_EINVAL, "null index%s");
    if (dim) *dim = ix->dim;
    if (padded_dim) *padded_dim = ix->dpad;
    if (dtype) *dtype = ix->dtype;
    return CODD_KNN_OK;
}

int codd_knn_read_rows(const codd_knn_index* ix, int64_t first, int64_t n, void* host_out) {
    if (!ix || first < 0 || n < 0 || first + n > ix->count || (n > 0 && !host_out)) return fail(CODD_KNN_EINVAL, "bad read_rows range%s");
    if (n == 0) return CODD_KNN_OK;
    DeviceGuard guard(ix->device);
    const size_t row_bytes = (size_t)ix->dpad * elem_size(ix->dtype);
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(host_out, ix->rows + (size_t)first * row_bytes, (size_t)n * row_bytes, hipMemcpyDeviceToHost));
    return CODD_KNN_OK;
}

int codd_knn_search(codd_knn_index* ix, const float* dev_queries, int B, int k, float* dev_dist, int64_t* dev_rows, void* stream) {
    if (!dev_dist || !dev_rows) return fail(CODD_KNN_EINVAL, "null output%s");
    if (!ix) return fail(CODD_KNN_EINVAL, "null index%s");
    WorkScope work(ix, (hipStream_t)stream);
    return search_impl(ix, dev_queries, B, k, 0u, nullptr, dev_dist, dev_rows, (hipStream_t)stream, ix->dead_bits);
}

int codd_knn_search_keys(codd_knn_index* ix, const float* dev_queries, int B, int k, uint32_t row_base, uint64_t* dev_keys, void* stream) {
    if (!dev_keys) return fail(CODD_KNN_EINVAL, "null output%s");
    if (!ix) return fail(CODD_KNN_EINVAL, "null index%s");
    if ((int64_t)row_base + ix->count >= 0xffffffffll) return fail(CODD_KNN_EINVAL, "global row ids must fit 32 bits%s");
    WorkScope work(ix, (hipStream_t)stream);
    return search_impl(ix, dev_queries, B, k, row_base, (u64*)dev_keys, nullptr, nullptr, (hipStream_t)stream, ix->dead_bits);
}

int codd_knn_merge_keys(int device, const uint64_t* dev_keys_in, int B, int m, int k, uint64_t* dev_keys_out, float* dev_dist,
                        int64_t* dev_rows, void* stream) {
    if (!dev_keys_in || B < 1 || m < 1 || k < 1 || k > CODD_KNN_MAX_K) return fail(CODD_KNN_EINVAL, "bad merge arguments%s");
    DeviceGuard guard(device);
    return launch_merge((const u64*)dev_keys_in, B, m, m, k, (u64*)dev_keys_out, dev_dist, dev_rows, (hipStream_t)stream);
}

int codd_knn_merge_shards(int device, const uint64_t* dev_keys_in, int G, int B, int k_in, int k, uint64_t* dev_keys_out, float* dev_dist,
                          int64_t* dev_rows, void* stream) {
    if (!dev_keys_in || G < 1 || B < 1 || k_in < 1 || k < 1 || k > CODD_KNN_MAX_K) return fail(CODD_KNN_EINVAL, "bad merge arguments%s");
    DeviceGuard guard(device);
    return launch_merge((const u64*)dev_keys_in, B, (int64_t)G * k_in, k_in, k, (u64*)dev_keys_out, dev_dist, dev_rows, (hipStream_t)stream, nullptr,
                        nullptr, nullptr, k_in, (int64_t)B * k_in);
}

int codd_knn_merge_keys_metric(int device, const uint64_t* dev_keys_in, int B, int m, int k, int metric, uint64_t* dev_keys_out, float* dev_dist,
                               int64_t* dev_rows, void* stream) {
    if (!dev_keys_in || B < 1 || m < 1 || k < 1 || k > CODD_KNN_MAX_K) return fail(CODD_KNN_EINVAL, "bad merge arguments%s");
    if (metric != CODD_KNN_METRIC_COSINE && metric != CODD_KNN_METRIC_IP && metric != CODD_KNN_METRIC_L2) return fail(CODD_KNN_ENOTSUP, "unknown metric (cosine 0, ip 1, l2 2)%s");
    DeviceGuard guard(device);
    return launch_merge((const u64*)dev_keys_in, B, m, m, k, (u64*)dev_keys_out, dev_dist, dev_rows, (hipStream_t)stream, nullptr, nullptr, nullptr, 0, 0,
                        kernel_metric(metric));
}

int codd_knn_merge_shards_metric(int device, const uint64_t* dev_keys_in, int G, int B, int k_in, int k, int metric, uint64_t* dev_keys_out,
                                 float* dev_dist, int64_t* dev_rows, void* stream) {
    if (!dev_keys_in || G < 1 || B < 1 || k_in < 1 || k < 1 || k > CODD_KNN_MAX_K) return fail(CODD_KNN_EINVAL, "bad merge arguments%s");
    if (metric != CODD_KNN_METRIC_COSINE && metric != CODD_KNN_METRIC_IP && metric != CODD_KNN_METRIC_L2) return fail(CODD_KNN_ENOTSUP, "unknown metric (cosine 0, ip 1, l2 2)%s");
    DeviceGuard guard(device);
    return launch_merge((const u64*)dev_keys_in, B, (int64_t)G * k_in, k_in, k, (u64*)dev_keys_out, dev_dist, dev_rows, (hipStream_t)stream, nullptr,
                        nullptr, nullptr, k_in, (int64_t)B * k_in, kernel_metric(metric));
}

int codd_knn_approx_scores(codd_knn_index* ix, const float* dev_queries, int B, float* dev_scores, void* stream) {
    if (!ix || !dev_queries || !dev_scores || B < 1 || B > kTileQ) return fail(CODD_KNN_EINVAL, "bad debug arguments%s");
    // an ip or l2 index: the values of its int8 filter leg, where that leg exists
    const bool space = !metric_is_cosine(ix);
    const bool space_ok = space && ix->space_filter && ix->shadow8_enabled && CODD_MFMA16 && B <= 32 && !(ix->metric == CODD_KNN_METRIC_L2 && niter_of(ix) > 4);
    if (space && !space_ok)
        return fail(CODD_KNN_ENOTSUP, "approx_scores: the MFMA filters' scores exist for the cosine metric only (ip, l2: with \"space_filter\" on, B <= 32)%s");
    if (ix->count < 1) return fail(CODD_KNN_EINVAL, "empty index%s");
    DeviceGuard guard(ix->device);
    hipStream_t st = (hipStream_t)stream;
    WorkScope work(ix, st);
    int rc;
    if ((rc = wait_rows(ix, st)) != 0) return rc;
    HIP_TRY(ix->qn.ensure((int64_t)B * ix->dpad));
    if (space) {
        if ((rc = ensure_space_filter(ix, st)) != 0) return rc;
        if ((rc = launch_prep_raw(ix, dev_queries, B, ix->qn, st)) != 0) return rc;
        const int dpad8 = dpad8_of(ix);
        const int64_t ntiles8 = (ix->count + kTileRows - 1) / kTileRows;
        const dim3 g8((unsigned)(ntiles8 < ix->num_cus ? ntiles8 : ix->num_cus));
        if (ix->metric == CODD_KNN_METRIC_L2)
            rc = launch_kernel<sqd_filter_kernel<MODE_DUMP, 1>>(g8, dim3(kFilterThreads), filter_lds_bytes(MODE_DUMP), st, ix->shadow8, ix->qfrag8, ix->count, dpad8 / 128,
                                                                ntiles8, (int64_t)1, nullptr, nullptr, nullptr, nullptr, 0, nullptr, dev_scores, ix->rscale, ix->qmeta,
                                                                ix->rnorm2, ix->qmeta + 512);
        else
            rc = launch_kernel<gemm_filter_kernel<MODE_DUMP, 1, 1>>(g8, dim3(kFilterThreads), filter_lds_bytes(MODE_DUMP), st, ix->shadow8, ix->qfrag8, ix->count,
                                                                    dpad8 / 128, ntiles8, (int64_t)1, nullptr, nullptr, nullptr, nullptr, 0, nullptr, dev_scores, ix->rscale,
                                                                    ix->qmeta);
        if (rc != 0) return rc;
        HIP_TRY(hipGetLastError());
        return CODD_KNN_OK;
    }
    if ((rc = ensure_filter_workspace(ix)) != 0) return rc;
    if (ix->shadow8_enabled && B <= 32 && CODD_MFMA16) {
        // the int8 filter's scores (what a batch of <= 32 queries is filtered with when "shadow8" is on)
        if ((rc = ensure_shadow8(ix, st)) != 0) return rc;
        const int dpad8 = dpad8_of(ix);
        HIP_TRY(ix->qfrag8.ensure((int64_t)kTileQ * (dpad8 / 16)));
        if (!ix->qmeta) HIP_TRY(ix->qmeta.reset(1024));
        hipLaunchKernelGGL(prep_queries8_kernel, dim3(kTileQ / 4), dim3(256), 0, st, dev_queries, B, ix->dim, ix->dpad, dpad8, ix->qn,
                           reinterpret_cast<uint32_t*>(ix->qfrag8.get()), ix->qmeta, ix->eps_r_bits, reinterpret_cast<unsigned*>(ix->ctl.get()),
                           (int)(sizeof(FilterCtl) / 4), 1.0f);
        const int64_t ntiles8 = (ix->count + kTileRows - 1) / kTileRows;
        const int64_t g8 = ntiles8 < ix->num_cus ? ntiles8 : ix->num_cus;
        if ((rc = launch_kernel<gemm_filter_kernel<MODE_DUMP, 1, 1>>(dim3((unsigned)g8), dim3(kFilterThreads), filter_lds_bytes(MODE_DUMP), st,
                                                                     ix->shadow8, ix->qfrag8, ix->count, dpad8 / 128, ntiles8, (int64_t)1, nullptr, nullptr,
                                                                     nullptr, nullptr, 0, nullptr, dev_scores, ix->rscale, ix->qmeta)) != 0)
            return rc;
        HIP_TRY(hipGetLastError());
        return CODD_KNN_OK;
    }
    if ((rc = ensure_shadow(ix, st)) != 0) return rc;
    if ((rc = launch_normalize(DT_F32, dev_queries, B, ix->dim, ix->dpad, 1, nullptr, 0, ix->qn, nullptr, st)) != 0) return rc;
    hipLaunchKernelGGL(qfrag_kernel, dim3((kTileQ * (ix->dpad / 8) + 255) / 256), dim3(256), 0, st, ix->qn, B, ix->dpad, ix->qfrag,
                       (unsigned*)nullptr, 0);
    const int64_t ntiles = (ix->count + kTileRows - 1) / kTileRows;
    const int64_t g = ntiles < ix->num_cus ? ntiles : ix->num_cus;
    if ((rc = launch_kernel<gemm_filter_kernel<MODE_DUMP, 8>>(dim3((unsigned)g), dim3(kFilterThreads), filter_lds_bytes(MODE_DUMP), st, ix->shadow,
                                                              ix->qfrag, ix->count, ix->dpad / 64, ntiles, (int64_t)1, nullptr, nullptr, nullptr, nullptr, 0,
                                                              nullptr, dev_scores, nullptr, nullptr)) != 0)
        return rc;
    HIP_TRY(hipGetLastError());
    return CODD_KNN_OK;
}

int codd_knn_filter_slack(codd_knn_index* ix, const float* dev_queries, int B, float* dev_slack, void* stream) {
    if (!ix || !dev_queries || !dev_slack || B < 1 || B > kTileQ) return fail(CODD_KNN_EINVAL, "bad debug arguments%s");
    const bool space = !metric_is_cosine(ix);
    if (!ix->shadow8_enabled || !CODD_MFMA16 || (space && !ix->space_filter) || (space && ix->metric == CODD_KNN_METRIC_L2 && niter_of(ix) > 4))
        return fail(CODD_KNN_ENOTSUP, "filter_slack: this index has no int8 filter leg (\"shadow8\"; ip, l2: \"space_filter\")%s");
    if (ix->count < 1) return fail(CODD_KNN_EINVAL, "empty index%s");
    DeviceGuard guard(ix->device);
    hipStream_t st = (hipStream_t)stream;
    WorkScope work(ix, st);
    int rc;
    if ((rc = wait_rows(ix, st)) != 0) return rc;
    HIP_TRY(ix->qn.ensure((int64_t)B * ix->dpad));
    if ((rc = ensure_space_filter(ix, st)) != 0) return rc;
    if (space) {
        if ((rc = launch_prep_raw(ix, dev_queries, B, ix->qn, st)) != 0) return rc;
    } else {
        hipLaunchKernelGGL(prep_queries8_kernel, dim3(kTileQ / 4), dim3(256), 0, st, dev_queries, B, ix->dim, ix->dpad, dpad8_of(ix), ix->qn,
                           reinterpret_cast<uint32_t*>(ix->qfrag8.get()), ix->qmeta, ix->eps_r_bits, reinterpret_cast<unsigned*>(ix->ctl.get()),
                           (int)(sizeof(FilterCtl) / 4), ix->exp_slack_scale);
    }
    hipLaunchKernelGGL(filter_slack_kernel, dim3(1), dim3(kTileQ), 0, st, ix->qmeta + 256, B, dev_slack);
    HIP_TRY(hipGetLastError());
    return CODD_KNN_OK;
}

int codd_knn_copy_rows_f32(codd_knn_index* ix, int64_t first, int64_t n, float* dev_out, void* stream) {
    if (!ix || first < 0 || n < 0 || first + n > ix->count || (n > 0 && !dev_out)) return fail(CODD_KNN_EINVAL, "bad copy_rows range%s");
    if (n == 0) return CODD_KNN_OK;
    DeviceGuard guard(ix->device);
    const dim3 grid((unsigned)((n + 3) / 4)), block(256);
    hipStream_t st = (hipStream_t)stream;
    std::lock_guard<std::mutex> lock(ix->mu);
    // a read of the stored rows on the caller's stream: behind the last asynchronous write (as a search is), and the next
    // writer on another stream is ordered behind it (reader_done)
    int rc;
    if ((rc = wait_rows(ix, st)) != 0) return rc;
    rc = with_dtype(ix->dtype, [&](auto dt) {
        return launch_kernel<widen_rows_kernel<dt>>(grid, block, 0, st, ix->rows, first, n, ix->dim, ix->dpad, dev_out);
    });
    if (rc != 0) return rc;
    HIP_TRY(hipGetLastError());
    HIP_TRY(ix->reader_done.ensure());
    if (ix->reader_event_set && ix->reader_stream != st) HIP_TRY(hipStreamWaitEvent(st, ix->reader_done, 0));  // (one event: chain the readers too)
    HIP_TRY(hipEventRecord(ix->reader_done, st));
    ix->reader_stream = st;
    ix->reader_event_set = true;
    return CODD_KNN_OK;
}

int codd_knn_ivf_install(codd_knn_index* ix, const float* dev_centroids, int nlist, const int64_t* dev_perm,
                         const int64_t* dev_offsets, void* stream) {
    if (!ix || !dev_centroids || !dev_perm || !dev_offsets || nlist < 1 || nlist > (1 << 20)) return fail(CODD_KNN_EINVAL, "bad ivf_install arguments%s");
    if (!ivf_allowed(ix)) return fail(CODD_KNN_ENOTSUP, "ivf_install: IVF exists for the cosine metric only (spherical k-means, bf16 assignment)%s");
    if (ix->count < 1) return fail(CODD_KNN_EINVAL, "empty index%s");
    DeviceGuard guard(ix->device);
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipDeviceSynchronize());
    drop_ivf(ix);  // a previous layout

    const size_t row_bytes = (size_t)ix->dpad * elem_size(ix->dtype);
    const int64_t n = ix->count;
    // validate the caller's tables before anything indexes memory with them: offsets on the host (nlist + 1 values),
    // the permutation on the device
    {
        std::vector<int64_t> off((size_t)nlist + 1);
        HIP_TRY(hipMemcpyAsync(off.data(), dev_offsets, off.size() * sizeof(int64_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        bool ok = off[0] == 0 && off[(size_t)nlist] == n;
        for (int l = 0; ok && l < nlist; ++l) ok = off[(size_t)l] <= off[(size_t)l + 1];
        if (!ok) return fail(CODD_KNN_EINVAL, "ivf_install: offsets must start at 0, never decrease and end at the row count%s");
        DevBuf<unsigned> bad;
        HIP_TRY(bad.reset(1));
        hipError_t e = hipMemsetAsync(bad, 0, sizeof(unsigned), st);
        unsigned host_bad = 1;
        if (e == hipSuccess) {
            hipLaunchKernelGGL(perm_check_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, dev_perm, n, bad);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipMemcpyAsync(&host_bad, bad, sizeof(unsigned), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) return fail(CODD_KNN_EDEVICE, "ivf_install: permutation check failed: %s", hipGetErrorString(e));
        if (host_bad) return fail(CODD_KNN_EINVAL, "ivf_install: permutation entries must lie in [0, count)%s");
    }
    // (a failed install leaves no half-built layout behind: drop_ivf)
    int rc = CODD_KNN_OK;
    hipError_t he = ix->rows_ivf.reset(n * (int64_t)row_bytes);
    if (he == hipSuccess) he = ix->ivf_ids.reset(n);
    if (he == hipSuccess) he = ix->ivf_offsets.reset((int64_t)nlist + 1);
    if (he == hipSuccess) he = hipMemcpyAsync(ix->ivf_offsets, dev_offsets, (size_t)(nlist + 1) * sizeof(int64_t), hipMemcpyDeviceToDevice, st);
    if (he == hipSuccess) {
        hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, reinterpret_cast<const uint4*>(ix->rows.get()), dev_perm, n,
                           (int)(row_bytes / 16), reinterpret_cast<uint4*>(ix->rows_ivf.get()), ix->ivf_ids);
        he = hipGetLastError();
    }
    if (he != hipSuccess) {
        drop_ivf(ix);
        return fail(he == hipErrorOutOfMemory ? CODD_KNN_ENOMEM : CODD_KNN_EDEVICE, "ivf_install: building the list layout failed: %s", hipGetErrorString(he));
    }
    // the coarse index lives in the index's own space: unit centroids for cosine, the centroids as given for ip and l2 (§22)
    rc = codd_knn_create(&ix->coarse, ix->device, ix->dim, DT_F32, ix->metric);
    if (rc == 0) rc = codd_knn_upsert_device(ix->coarse, 0, dev_centroids, nlist, metric_is_cosine(ix) ? 1 : 0, stream);
    if (rc == 0 && hipStreamSynchronize(st) != hipSuccess) rc = fail(CODD_KNN_EDEVICE, "ivf_install: device work failed%s");
    if (rc != 0) {
        drop_ivf(ix);
        return rc;
    }
    ix->ivf_nlist = nlist;
    ix->ivf_count = n;
    ix->ivf_epoch = ix->epoch;
    return CODD_KNN_OK;
}

}  // extern "C"

namespace {

// what the scoped, the masked and the IVF entry points check before they take a workspace
int search_check_args(const codd_knn_index* ix, const float* dev_queries, int B, int k, uint32_t row_base) {
    if (!ix || !dev_queries) return fail(CODD_KNN_EINVAL, "null index or queries%s");
    if (B < 1 || B > CODD_KNN_MAX_BATCH) return fail(CODD_KNN_EINVAL, "B out of range [1,1024]%s");
    if (k < 1 || k > CODD_KNN_MAX_K) return fail(CODD_KNN_EINVAL, "k out of range [1,128]%s");
    if ((int64_t)row_base + ix->count >= 0xffffffffll) return fail(CODD_KNN_EINVAL, "global row ids must fit 32 bits%s");
    return CODD_KNN_OK;
}

// nothing visible (or nothing stored): all-empty result, no scan
int empty_result(codd_knn_index* ix, int B, int k, uint64_t* dev_keys, float* dev_dist, int64_t* dev_rows, hipStream_t st) {
    HIP_TRY(ix->keys_tmp.ensure((int64_t)B * k));
    u64* keys_dst = dev_keys ? (u64*)dev_keys : ix->keys_tmp.get();
    HIP_TRY(hipMemsetAsync(keys_dst, 0, (size_t)B * k * sizeof(u64), st));
    if (!dev_dist && !dev_rows) return CODD_KNN_OK;
    return launch_merge(keys_dst, B, k, k, k, nullptr, dev_dist, dev_rows, st);
}

// what every IVF entry point checks before it takes a workspace; clamps nprobe to the number of lists
int ivf_check_args(const codd_knn_index* ix, const float* dev_queries, int B, int k, uint32_t row_base, int* nprobe) {
    int rc;
    if ((rc = search_check_args(ix, dev_queries, B, k, row_base)) != 0) return rc;
    if (!ivf_allowed(ix)) return fail(CODD_KNN_ENOTSUP, "IVF search exists for the cosine metric only%s");
    if (!ix->coarse || ix->ivf_epoch != ix->epoch) return fail(CODD_KNN_EINVAL, "no IVF layout, or rows changed since codd_knn_ivf_install%s");
    if (*nprobe < 1) return fail(CODD_KNN_EINVAL, "nprobe must be >= 1%s");
    if (*nprobe > ix->ivf_nlist) *nprobe = ix->ivf_nlist;
    if (*nprobe > CODD_KNN_MAX_K) return fail(CODD_KNN_ENOTSUP, "nprobe above 128 is not supported (probe the whole index with codd_knn_search)%s");
    return CODD_KNN_OK;
}

// The body of every IVF search; the caller has checked the arguments, made the device current and holds the workspaces of the
// index and of its coarse index for `st`.  deny: the ORIGINAL row slots no answer may hold — ix->dead_bits, or the ~allow | dead
// of a masked search, which the list scans test where they test the tombstones.  Probe selection never sees it.
int ivf_search_body(codd_knn_index* ix, const float* dev_queries, int B, int k, int nprobe, uint32_t row_base, uint64_t* dev_keys, float* dev_dist,
                    int64_t* dev_rows, hipStream_t st, const uint32_t* deny) {
    int rc;
    if ((rc = wait_rows(ix, st)) != 0) return rc;
    HIP_TRY(ix->qn.ensure((int64_t)B * ix->dpad));
    HIP_TRY(ix->probe_keys.ensure((int64_t)B * nprobe));
    if ((rc = prep_exact_queries(ix, dev_queries, B, st)) != 0) return rc;
    const bool sq = ix->metric == CODD_KNN_METRIC_L2;  // the squared-distance list scans (§22); ip runs the dot-product ones on the raw query
    // 1. coarse: the nprobe best lists per query (exact scan of the centroids in the index's space, tiny)
    if ((rc = exact_scan(ix->coarse, ix->qn, B, nprobe, 0u, ix->probe_keys, nullptr, nullptr, st, ix->coarse->dead_bits)) != 0) return rc;
    const int niter = niter_of(ix);
    // 2a. a batch with enough (query, list) pairs to fill the chip without splitting lists: group the pairs by list on the
    //     device and scan every probed list once per kIvfNB of its queries (ivf_scan_shared_kernel)
    const int64_t npairs = (int64_t)B * nprobe;
    //     (worth it once a list is probed by two queries or more on average: below that every work item holds one pair and the
    //     grouping launches are pure overhead — 12.5M x 1024 fp16, 2,048 lists, B = 256: nprobe 8 5.98 ms per pair vs 7.22 shared)
    if (ix->ivf_share && npairs >= 1024 && npairs >= 2 * (int64_t)ix->ivf_nlist && !(ix->dtype != DT_F32 && niter == 4)) {
        const int nlist = ix->ivf_nlist;
        ix->stat_ivf_shared++;
        HIP_TRY(ix->ivf_group.ensure(3 * (int64_t)nlist + 2 + npairs));
        HIP_TRY(ix->ivf_partial.ensure(npairs * k));
        unsigned* cnt = ix->ivf_group;
        unsigned* pair_start = cnt + nlist;
        unsigned* item_start = pair_start + nlist + 1;
        unsigned* sorted_pairs = item_start + nlist + 1;
        {
        EvScope ev(ix, EV_SCAN, st);
        HIP_TRY(hipMemsetAsync(cnt, 0, (size_t)nlist * sizeof(unsigned), st));
        HIP_TRY(hipMemsetAsync(ix->ivf_partial, 0, (size_t)(npairs * k) * sizeof(u64), st));  // (an empty probe slot stays an empty list)
        const unsigned pb = (unsigned)((npairs + 255) / 256);
        hipLaunchKernelGGL(ivf_pair_count_kernel, dim3(pb), dim3(256), 0, st, ix->probe_keys, (int)npairs, cnt);
        hipLaunchKernelGGL(ivf_pair_offsets_kernel, dim3(1), dim3(1024), 0, st, cnt, nlist, pair_start, item_start);
        hipLaunchKernelGGL(ivf_pair_scatter_kernel, dim3(pb), dim3(256), 0, st, ix->probe_keys, (int)npairs, pair_start, cnt, sorted_pairs);
        // work items <= sum over lists of ceil(pairs / kIvfNB) <= min(pairs, lists + pairs / kIvfNB): the grid covers the bound, surplus workgroups leave at once
        const int64_t bound = std::min<int64_t>(npairs, (int64_t)nlist + npairs / kIvfNB);
        rc = with_row_form(ix, k, "row too wide for the IVF scan%s", [&](auto dt, auto ni, auto sl) {
            if (sq) {
                // (2-byte rows of 4 chunks per lane never come here, see the condition above: that form is not built)
                if constexpr (decltype(dt)::value != DT_F32 && decltype(ni)::value == 4) {
                    return fail(CODD_KNN_EINVAL, "the shared squared-distance scan takes no 2-byte rows of 4 chunks per lane%s");
                } else {
                    return launch_kernel<ivf_shared_sq<dt, ni, sl>>(dim3((unsigned)bound), dim3(256), 0, st, ix->rows_ivf, ix->ivf_ids, ix->ivf_offsets, pair_start,
                                                                    item_start, sorted_pairs, nlist, nprobe, ix->dpad, ix->qn, k, row_base, ix->ivf_partial, deny);
                }
            }
            return launch_kernel<ivf_scan_shared_kernel<dt, ni, sl>>(dim3((unsigned)bound), dim3(256), 0, st, ix->rows_ivf, ix->ivf_ids, ix->ivf_offsets,
                                                                     pair_start, item_start, sorted_pairs, nlist, nprobe, ix->dpad, ix->qn, k, row_base,
                                                                     ix->ivf_partial, deny);
        });
        if (rc != 0) return rc;
        HIP_TRY(hipGetLastError());
        }
        const int64_t ms = (int64_t)nprobe * k;
        return launch_merge_of(ix, ix->ivf_partial, B, ms, k, (u64*)dev_keys, dev_dist, dev_rows, st);
    }
    // 2. scan the probed lists; split each list over several blocks when the batch alone cannot fill the chip
    int split = (int)((4 * (int64_t)ix->num_cus + (int64_t)B * nprobe - 1) / ((int64_t)B * nprobe));
    split = split < 1 ? 1 : (split > 16 ? 16 : split);
    const int64_t m = (int64_t)nprobe * split * k;
    HIP_TRY(ix->ivf_partial.ensure((int64_t)B * m));
    const dim3 grid((unsigned)(nprobe * split), (unsigned)B), block(256);
    {
        EvScope ev(ix, EV_SCAN, st);
        rc = with_row_form(ix, k, "row too wide for the IVF scan%s", [&](auto dt, auto ni, auto sl) {
            if (sq)
                return launch_kernel<ivf_scan_sq<dt, ni, sl>>(grid, block, 0, st, ix->rows_ivf, ix->ivf_ids, ix->ivf_offsets, ix->probe_keys, nprobe, split, ix->dpad,
                                                              ix->qn, k, row_base, ix->ivf_partial, deny);
            return launch_kernel<ivf_scan_kernel<dt, ni, sl>>(grid, block, 0, st, ix->rows_ivf, ix->ivf_ids, ix->ivf_offsets, ix->probe_keys, nprobe, split,
                                                              ix->dpad, ix->qn, k, row_base, ix->ivf_partial, deny);
        });
    }
    if (rc != 0) return rc;
    HIP_TRY(hipGetLastError());
    // 3. top-k of the nprobe*split partial lists
    return launch_merge_of(ix, ix->ivf_partial, B, m, k, (u64*)dev_keys, dev_dist, dev_rows, st);
}

}  // namespace

extern "C" {

int codd_knn_ivf_search(codd_knn_index* ix, const float* dev_queries, int B, int k, int nprobe, uint32_t row_base,
                        uint64_t* dev_keys, float* dev_dist, int64_t* dev_rows, void* stream) {
    int rc;
    if ((rc = ivf_check_args(ix, dev_queries, B, k, row_base, &nprobe)) != 0) return rc;
    DeviceGuard guard(ix->device);
    hipStream_t st = (hipStream_t)stream;
    WorkScope work(ix, st), work_coarse(ix->coarse, st);
    return ivf_search_body(ix, dev_queries, B, k, nprobe, row_base, dev_keys, dev_dist, dev_rows, st, ix->dead_bits);
}

int codd_knn_set_scopes_host(codd_knn_index* ix, const int64_t* host_slots, const uint32_t* host_scopes, int64_t n) {
    if (!ix || n < 0 || (n > 0 && (!host_slots || !host_scopes))) return fail(CODD_KNN_EINVAL, "bad set_scopes arguments%s");
    if (n == 0) return CODD_KNN_OK;
    uint32_t top = 0;
    bool increasing = true;
    for (int64_t i = 0; i < n; ++i) {
        if (host_slots[i] < 0 || host_slots[i] >= ix->count) return fail(CODD_KNN_EINVAL, "set_scopes: row slot outside [0, count)%s");
        if (slot_dead(ix, host_slots[i])) return fail(CODD_KNN_EINVAL, "set_scopes: deleted row slot (it stays dead until codd_knn_compact)%s");
        if (host_scopes[i] > CODD_KNN_MAX_SCOPE) return fail(CODD_KNN_EINVAL, "set_scopes: scope above CODD_KNN_MAX_SCOPE%s");
        if (host_scopes[i] > top) top = host_scopes[i];
        if (i > 0 && host_slots[i] <= host_slots[i - 1]) increasing = false;
    }
    // (slot, scope) packed into one word each; a slot listed more than once keeps its LAST label (the device writes in no order)
    std::vector<int64_t> packed;
    try {
        packed.resize((size_t)n);
        for (int64_t i = 0; i < n; ++i) packed[(size_t)i] = (int64_t)(((u64)host_scopes[i] << 32) | (u64)host_slots[i]);
        if (!increasing) {
            std::vector<int64_t> order((size_t)n);
            for (int64_t i = 0; i < n; ++i) order[(size_t)i] = i;
            std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return host_slots[a] < host_slots[b]; });
            size_t m = 0;
            for (int64_t i = 0; i < n; ++i)
                if (i + 1 == n || host_slots[order[(size_t)i]] != host_slots[order[(size_t)i + 1]])
                    packed[m++] = (int64_t)(((u64)host_scopes[order[(size_t)i]] << 32) | (u64)host_slots[order[(size_t)i]]);
            packed.resize(m);
        }
    } catch (const std::bad_alloc&) {
        return fail(CODD_KNN_ENOMEM, "host allocation failed%s");
    }
    DeviceGuard guard(ix->device);
    HIP_TRY(hipDeviceSynchronize());
    int rc;
    if ((rc = ensure_scope_labels(ix, nullptr)) != 0) return rc;
    if (ix->stage_slot.cap() < 4096) HIP_TRY(ix->stage_slot.reset(4096));  // (the staging buffer codd_knn_upsert_host keeps between calls)
    const int64_t total = (int64_t)packed.size(), pn = ix->stage_slot.cap();
    for (int64_t i0 = 0; i0 < total; i0 += pn) {
        const int64_t m = total - i0 < pn ? total - i0 : pn;
        HIP_TRY(hipMemcpy(ix->stage_slot, packed.data() + i0, (size_t)m * sizeof(int64_t), hipMemcpyHostToDevice));
        hipLaunchKernelGGL(scope_set_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, nullptr, ix->stage_slot, m, ix->scope_of);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipDeviceSynchronize());  // (the staging buffer is reused by the next piece, and the call is synchronous by contract)
    }
    if (top > ix->max_scope) ix->max_scope = top;
    ix->scope_gen++;
    return CODD_KNN_OK;
}

int codd_knn_search_scoped(codd_knn_index* ix, const float* dev_queries, const uint32_t* dev_scopes, int B, int k, uint32_t row_base,
                           uint64_t* dev_keys, float* dev_dist, int64_t* dev_rows, void* stream) {
    if (!ix || !dev_queries) return fail(CODD_KNN_EINVAL, "null index or queries%s");
    if (!dev_scopes) return fail(CODD_KNN_EINVAL, "null scopes%s");
    int rc;
    if ((rc = search_check_args(ix, dev_queries, B, k, row_base)) != 0) return rc;
    DeviceGuard guard(ix->device);
    hipStream_t st = (hipStream_t)stream;
    WorkScope work(ix, st);
    ix->stat_scoped_searches++;
    const int64_t n = ix->count;
    if ((rc = wait_rows(ix, st)) != 0) return rc;
    if (n == 0) return empty_result(ix, B, k, dev_keys, dev_dist, dev_rows, st);  // nothing stored: all-empty result, as codd_knn_search gives
    // enough work items to fill the chip whatever the batch: a scope's list is cut into `split` parts.  The batch has between
    // ceil(B / 4) (one scope) and B (all different) groups of queries; the lower bound sizes the split, surplus workgroups are cheap.
    const int64_t groups = (B + 3) / 4;
    int split = (int)((4 * (int64_t)ix->num_cus + groups - 1) / groups);
    split = split < 1 ? 1 : (split > 256 ? 256 : split);
    const int64_t m = (int64_t)split * k;
    HIP_TRY(ix->qn.ensure((int64_t)B * ix->dpad));
    HIP_TRY(ix->partial.ensure((int64_t)B * m));
    HIP_TRY(ix->scope_group.ensure((int64_t)2 * CODD_KNN_MAX_BATCH));
    if ((rc = ensure_scope_lists(ix, st)) != 0) return rc;
    if ((rc = prep_exact_queries(ix, dev_queries, B, st)) != 0) return rc;
    unsigned* sorted_q = ix->scope_group;
    unsigned* rank = sorted_q + CODD_KNN_MAX_BATCH;
    hipLaunchKernelGGL(scope_group_kernel, dim3(1), dim3(1024), 0, st, dev_scopes, B, sorted_q, rank);
    HIP_TRY(hipGetLastError());
    {
        EvScope ev(ix, EV_SCAN, st);
        rc = with_row_form(ix, k, "row too wide for the scope scan%s", [&](auto dt, auto ni, auto sl) {
            if (ix->metric == CODD_KNN_METRIC_L2)
                return launch_kernel<scope_scan_l2<dt, ni, sl>>(dim3((unsigned)B, (unsigned)split), dim3(256), 0, st, ix->rows, ix->scope_perm, ix->scope_offsets,
                                                                n - ix->dead_count, ix->max_scope, dev_scopes, sorted_q, rank, B, split, ix->dpad, ix->qn, k, row_base,
                                                                ix->partial);
            return launch_kernel<scope_scan_kernel<dt, ni, sl>>(dim3((unsigned)B, (unsigned)split), dim3(256), 0, st, ix->rows, ix->scope_perm,
                                                                ix->scope_offsets, n - ix->dead_count, ix->max_scope, dev_scopes, sorted_q, rank, B, split, ix->dpad,
                                                                ix->qn, k, row_base, ix->partial);
        });
    }
    if (rc != 0) return rc;
    HIP_TRY(hipGetLastError());
    return launch_merge_of(ix, ix->partial, B, m, k, (u64*)dev_keys, dev_dist, dev_rows, st);
}

}  // extern "C"

namespace {

// Which way a masked search of m visible rows goes (time only, both routes give the same bits).  Dense — the
// ordinary dispatch under ~allow | dead — when the sample's anchors can be expected to hold 4k visible rows and the pass over the
// whole index costs less than ceil(B / NB) gathered walks of the list; "mask_list_pct" scales the dense side of that comparison.
bool mask_takes_dense(const codd_knn_index* ix, int B, int k, int64_t m) {
    if (ix->mask_route == 1) return false;
    if (ix->mask_route == 2) return true;
    const int64_t n = ix->count;
    const int64_t row_bytes = (int64_t)ix->dpad * (int64_t)elem_size(ix->dtype);
    const int nb = scope_nb(ix->dtype, niter_of(ix) > 4 ? kWideRows : niter_of(ix));
    const double list_bytes = 2.0 * (double)((B + nb - 1) / nb) * (double)m * (double)row_bytes;
    double dense_bytes;
    if (filter_applies(ix, B, k)) {
        const bool can8 = ix->shadow8_enabled && CODD_MFMA16 && (B <= ix->shadow8_max_batch || (B > kTileQ && ix->shadow8_max_batch >= kTileQ));
        const int nq = B < kTileQ ? B : kTileQ;
        const int nbq = nq <= 32 ? 1 : (nq <= 64 ? 2 : (nq <= 128 ? 4 : 8));
        const int64_t ts = sample_tile_count(ix, (n + kTileRows - 1) / kTileRows, k, can8, nbq);
        if ((double)m * (double)ts < 4.0 * (double)k * (double)n) return false;   // too few visible anchors: the pass would end in the fallback scan
        dense_bytes = (double)((B + kTileQ - 1) / kTileQ) * (double)n * (double)(can8 ? dpad8_of(ix) : 2 * ix->dpad);
    } else {
        // the exact scan reads the rows once per group of 8 queries, streaming: twice the rate of the gathered walk, as above
        dense_bytes = (double)((B + 7) / 8) * (double)n * (double)row_bytes;
    }
    return list_bytes * 100.0 > dense_bytes * (double)ix->mask_list_pct;
}

// The body both masked entry points run: the clipped allow words are in ix->mask_allow (written on `st`, or enqueued there) and m > 0,
// the number of allowed live rows, is known on the host.  Chooses the route and enqueues it.
int masked_search_body(codd_knn_index* ix, const float* dev_queries, int B, int k, int64_t nwords, int64_t m, uint32_t row_base,
                       uint64_t* dev_keys, float* dev_dist, int64_t* dev_rows, hipStream_t st) {
    const int64_t n = ix->count;
    int rc;
    if (mask_takes_dense(ix, B, k, m)) {
        ix->stat_mask_dense++;
        const int64_t total_words = (ix->capacity + 31) / 32;   // (as long as the tombstone bits: every kernel that reads those reads these)
        HIP_TRY(ix->mask_deny.ensure(total_words));
        hipLaunchKernelGGL(mask_deny_kernel, dim3((unsigned)((total_words + 255) / 256)), dim3(256), 0, st, ix->mask_allow, ix->dead_bits, n, nwords,
                           total_words, ix->mask_deny);
        HIP_TRY(hipGetLastError());
        std::swap(ix->dstats, ix->mask_dstats);   // (the passes below count into the masked searches' own counters)
        rc = search_impl(ix, dev_queries, B, k, row_base, (u64*)dev_keys, dev_dist, dev_rows, st, ix->mask_deny, true);
        std::swap(ix->dstats, ix->mask_dstats);
        return rc;
    }

    ix->stat_mask_list++;
    const int64_t nblocks = (nwords + 255) / 256;
    HIP_TRY(ix->mask_prefix.ensure(nwords + 2 * nblocks + 1));
    HIP_TRY(ix->mask_list.ensure(m));
    unsigned* prefix = ix->mask_prefix;
    unsigned* block_total = prefix + nwords;
    unsigned* block_base = block_total + nblocks;
    hipLaunchKernelGGL(mask_prefix_kernel, dim3((unsigned)nblocks), dim3(256), 0, st, ix->mask_allow, ix->dead_bits, n, nwords, prefix, block_total);
    hipLaunchKernelGGL(scope_offsets_kernel, dim3(1), dim3(1024), 0, st, block_total, (int)nblocks, block_base);
    hipLaunchKernelGGL(mask_scatter_kernel, dim3((unsigned)nblocks), dim3(256), 0, st, ix->mask_allow, ix->dead_bits, n, nwords, prefix, block_base, m,
                       ix->mask_list);
    HIP_TRY(hipGetLastError());
    // the split of codd_knn_search_scoped, and no more parts than the list has workgroup steps (16 rows)
    const int64_t groups = (B + 3) / 4;
    int split = (int)((4 * (int64_t)ix->num_cus + groups - 1) / groups);
    split = split < 1 ? 1 : (split > 256 ? 256 : split);
    if ((int64_t)split > (m + 15) / 16) split = (int)((m + 15) / 16);
    const int64_t pm = (int64_t)split * k;
    HIP_TRY(ix->qn.ensure((int64_t)B * ix->dpad));
    HIP_TRY(ix->partial.ensure((int64_t)B * pm));
    if ((rc = prep_exact_queries(ix, dev_queries, B, st)) != 0) return rc;
    {
        EvScope ev(ix, EV_SCAN, st);
        rc = with_row_form(ix, k, "row too wide for the mask scan%s", [&](auto dt, auto ni, auto sl) {
            constexpr int NB = scope_nb(decltype(dt)::value, decltype(ni)::value);
            if (ix->metric == CODD_KNN_METRIC_L2)
                return launch_kernel<mask_scan_l2<dt, ni, sl>>(dim3((unsigned)((B + NB - 1) / NB), (unsigned)split), dim3(256), 0, st, ix->rows, ix->mask_list, m, B,
                                                               split, ix->dpad, ix->qn, k, row_base, ix->partial);
            return launch_kernel<mask_scan_kernel<dt, ni, sl>>(dim3((unsigned)((B + NB - 1) / NB), (unsigned)split), dim3(256), 0, st, ix->rows, ix->mask_list, m,
                                                               B, split, ix->dpad, ix->qn, k, row_base, ix->partial);
        });
    }
    if (rc != 0) return rc;
    HIP_TRY(hipGetLastError());
    return launch_merge_of(ix, ix->partial, B, pm, k, (u64*)dev_keys, dev_dist, dev_rows, st);
}

// The host words of a masked search (nwords > 0 of them): clipped to [0, n) into the workspace's pinned staging buffer and counted
// against the tombstone mirror on the way (*m: the rows the call may see, exact, nothing read back).  The caller's words are not
// touched again; the staging buffer's previous copy (the stream's last masked search) is waited for first.
int stage_host_mask(codd_knn_index* ix, const uint32_t* host_allow_bits, int64_t nwords, int64_t n, int64_t* m) {
    if (ix->mask_upload_pending) HIP_TRY(hipEventSynchronize(ix->mask_uploaded));
    ix->mask_upload_pending = false;
    if (nwords > ix->mask_host.cap()) HIP_TRY(ix->mask_host.reset(nwords + nwords / 2 + 64));
    HIP_TRY(ix->mask_uploaded.ensure());
    const bool any_dead = ix->dead_count > 0;
    int64_t seen = 0;
    for (int64_t w = 0; w < nwords; ++w) {
        const int64_t left = n - w * 32;
        const uint32_t a = host_allow_bits[w] & (left >= 32 ? 0xffffffffu : (1u << (uint32_t)left) - 1u);
        ix->mask_host[w] = a;
        seen += __builtin_popcount(any_dead && (size_t)w < ix->dead_host.size() ? a & ~ix->dead_host[(size_t)w] : a);
    }
    *m = seen;
    return CODD_KNN_OK;
}

// ... and one asynchronous copy on `st` takes the staged words to the workspace's allow buffer
int upload_staged_mask(codd_knn_index* ix, int64_t nwords, hipStream_t st) {
    HIP_TRY(ix->mask_allow.ensure(nwords));
    HIP_TRY(hipMemcpyAsync(ix->mask_allow, ix->mask_host, (size_t)nwords * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipEventRecord(ix->mask_uploaded, st));
    ix->mask_upload_pending = true;
    return CODD_KNN_OK;
}

// A masked IVF search behind its mask: `allow` are nwords device words, valid on `st` (the workspace's copy of the
// host words, or the caller's own); deny = ~allow | dead over the nwords words that cover every row slot of the layout goes into the
// workspace's deny buffer and takes the tombstones' place in the list scans.  Nothing depends on how many rows the mask leaves.
int ivf_masked_body(codd_knn_index* ix, const float* dev_queries, int B, int k, int nprobe, const uint32_t* allow, int64_t nwords, uint32_t row_base,
                    uint64_t* dev_keys, float* dev_dist, int64_t* dev_rows, hipStream_t st) {
    HIP_TRY(ix->mask_deny.ensure(nwords));
    hipLaunchKernelGGL(mask_deny_kernel, dim3((unsigned)((nwords + 255) / 256)), dim3(256), 0, st, allow, ix->dead_bits, ix->count, nwords, nwords,
                       ix->mask_deny);
    HIP_TRY(hipGetLastError());
    return ivf_search_body(ix, dev_queries, B, k, nprobe, row_base, dev_keys, dev_dist, dev_rows, st, ix->mask_deny);
}

bool docs_valid(const codd_knn_index* ix) { return ix->doc_arena && ix->doc_epoch == ix->epoch && ix->doc_count == ix->count; }

}  // namespace

extern "C" {

int codd_knn_search_masked(codd_knn_index* ix, const float* dev_queries, int B, int k, const uint32_t* host_allow_bits, int64_t nwords,
                           uint32_t row_base, uint64_t* dev_keys, float* dev_dist, int64_t* dev_rows, void* stream) {
    int rc;
    if ((rc = search_check_args(ix, dev_queries, B, k, row_base)) != 0) return rc;
    DeviceGuard guard(ix->device);
    hipStream_t st = (hipStream_t)stream;
    WorkScope work(ix, st);
    const int64_t n = ix->count;
    if (nwords != (n + 31) / 32) return fail(CODD_KNN_EINVAL, "search_masked: nwords must be ceil(count / 32)%s");
    if (nwords > 0 && !host_allow_bits) return fail(CODD_KNN_EINVAL, "null allow bits%s");
    ix->stat_masked_searches++;
    if ((rc = wait_rows(ix, st)) != 0) return rc;
    // The host words: clipped to [0, count) into the workspace's pinned staging buffer, counted against the tombstone mirror on
    // the way (m: the rows this call may see, exact, nothing read back), then one asynchronous copy from the staging buffer.  The
    // caller's words are not touched again; the staging buffer's previous copy (the stream's last masked search) is waited for first.
    int64_t m = 0;
    if (nwords > 0 && (rc = stage_host_mask(ix, host_allow_bits, nwords, n, &m)) != 0) return rc;
    ix->stat_last_mask_rows = m;
    if (m == 0) return empty_result(ix, B, k, dev_keys, dev_dist, dev_rows, st);
    if ((rc = upload_staged_mask(ix, nwords, st)) != 0) return rc;
    return masked_search_body(ix, dev_queries, B, k, nwords, m, row_base, dev_keys, dev_dist, dev_rows, st);
}

int codd_knn_search_masked_dev(codd_knn_index* ix, const float* dev_queries, int B, int k, const uint32_t* dev_allow_bits, int64_t nwords,
                               uint32_t row_base, uint64_t* dev_keys, float* dev_dist, int64_t* dev_rows, void* stream) {
    int rc;
    if ((rc = search_check_args(ix, dev_queries, B, k, row_base)) != 0) return rc;
    DeviceGuard guard(ix->device);
    hipStream_t st = (hipStream_t)stream;
    WorkScope work(ix, st);
    const int64_t n = ix->count;
    if (nwords != (n + 31) / 32) return fail(CODD_KNN_EINVAL, "search_masked_dev: nwords must be ceil(count / 32)%s");
    if (nwords > 0 && !dev_allow_bits) return fail(CODD_KNN_EINVAL, "null allow bits%s");
    ix->stat_masked_searches++;
    ix->stat_masked_dev++;
    if ((rc = wait_rows(ix, st)) != 0) return rc;
    // The device words: clipped to [0, count) into the workspace's allow buffer and counted against the tombstone bits by one small
    // kernel behind whatever wrote them on `st`; the count comes back through pinned memory — the one host synchronisation of the call
    // (m chooses the route and sizes the list).
    int64_t m = 0;
    if (nwords > 0) {
        if (!ix->mask_m_dev) HIP_TRY(ix->mask_m_dev.reset(1));
        if (!ix->mask_m_host) HIP_TRY(ix->mask_m_host.reset(1));
        HIP_TRY(ix->mask_allow.ensure(nwords));
        HIP_TRY(hipMemsetAsync(ix->mask_m_dev, 0, sizeof(unsigned long long), st));
        hipLaunchKernelGGL(mask_clip_count_kernel, dim3((unsigned)((nwords + 255) / 256)), dim3(256), 0, st, dev_allow_bits, ix->dead_bits, n, nwords,
                           ix->mask_allow, ix->mask_m_dev);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(ix->mask_m_host, ix->mask_m_dev, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        m = (int64_t)*ix->mask_m_host;
    }
    ix->stat_last_mask_rows = m;
    if (m == 0) return empty_result(ix, B, k, dev_keys, dev_dist, dev_rows, st);
    return masked_search_body(ix, dev_queries, B, k, nwords, m, row_base, dev_keys, dev_dist, dev_rows, st);
}

int codd_knn_ivf_search_masked(codd_knn_index* ix, const float* dev_queries, int B, int k, int nprobe, const uint32_t* host_allow_bits, int64_t nwords,
                               uint32_t row_base, uint64_t* dev_keys, float* dev_dist, int64_t* dev_rows, void* stream) {
    int rc;
    if ((rc = ivf_check_args(ix, dev_queries, B, k, row_base, &nprobe)) != 0) return rc;
    DeviceGuard guard(ix->device);
    hipStream_t st = (hipStream_t)stream;
    WorkScope work(ix, st), work_coarse(ix->coarse, st);
    const int64_t n = ix->count;   // (>= 1: a layout exists)
    if (nwords != (n + 31) / 32) return fail(CODD_KNN_EINVAL, "ivf_search_masked: nwords must be ceil(count / 32)%s");
    if (!host_allow_bits) return fail(CODD_KNN_EINVAL, "null allow bits%s");
    ix->stat_ivf_masked++;
    int64_t m = 0;   // (counted by the staging pass, not needed: nothing here depends on it)
    if ((rc = stage_host_mask(ix, host_allow_bits, nwords, n, &m)) != 0) return rc;
    if ((rc = upload_staged_mask(ix, nwords, st)) != 0) return rc;
    return ivf_masked_body(ix, dev_queries, B, k, nprobe, ix->mask_allow, nwords, row_base, dev_keys, dev_dist, dev_rows, st);
}

int codd_knn_ivf_search_masked_dev(codd_knn_index* ix, const float* dev_queries, int B, int k, int nprobe, const uint32_t* dev_allow_bits, int64_t nwords,
                                   uint32_t row_base, uint64_t* dev_keys, float* dev_dist, int64_t* dev_rows, void* stream) {
    int rc;
    if ((rc = ivf_check_args(ix, dev_queries, B, k, row_base, &nprobe)) != 0) return rc;
    DeviceGuard guard(ix->device);
    hipStream_t st = (hipStream_t)stream;
    WorkScope work(ix, st), work_coarse(ix->coarse, st);
    if (nwords != (ix->count + 31) / 32) return fail(CODD_KNN_EINVAL, "ivf_search_masked_dev: nwords must be ceil(count / 32)%s");
    if (!dev_allow_bits) return fail(CODD_KNN_EINVAL, "null allow bits%s");
    ix->stat_ivf_masked++;
    // the caller's words are read once, by mask_deny_kernel on `st` (which clips them to [0, count) itself): no count, no read-back
    return ivf_masked_body(ix, dev_queries, B, k, nprobe, dev_allow_bits, nwords, row_base, dev_keys, dev_dist, dev_rows, st);
}

int codd_knn_slice_mask(int device, const uint32_t* dev_global_bits, int64_t global_rows, int64_t row_base, int64_t count, uint32_t* dev_out,
                        int64_t nwords, void* stream) {
    if (global_rows < 0 || row_base < 0 || count < 0) return fail(CODD_KNN_EINVAL, "slice_mask: negative global_rows, row_base or count%s");
    if (nwords != (count + 31) / 32) return fail(CODD_KNN_EINVAL, "slice_mask: nwords must be ceil(count / 32)%s");
    if (nwords == 0) return CODD_KNN_OK;
    if (!dev_out || (global_rows > 0 && !dev_global_bits)) return fail(CODD_KNN_EINVAL, "slice_mask: null words%s");
    DeviceGuard guard(device);
    const int rc = launch_kernel<mask_slice_kernel>(dim3((unsigned)((nwords + 255) / 256)), dim3(256), 0, (hipStream_t)stream, dev_global_bits, global_rows,
                                                    row_base, count, dev_out, nwords);
    if (rc != 0) return rc;
    HIP_TRY(hipGetLastError());
    return CODD_KNN_OK;
}

int codd_knn_set_documents_host(codd_knn_index* ix, const uint8_t* host_bytes, const int64_t* host_offsets, int64_t n) {
    if (!ix || !host_offsets || n < 0) return fail(CODD_KNN_EINVAL, "set_documents: null index or offsets%s");
    if (n != ix->count) return fail(CODD_KNN_EINVAL, "set_documents: n must equal the count (one document per row slot)%s");
    if (host_offsets[0] != 0) return fail(CODD_KNN_EINVAL, "set_documents: offsets must start at 0%s");
    for (int64_t r = 0; r < n; ++r)
        if (host_offsets[r + 1] < host_offsets[r]) return fail(CODD_KNN_EINVAL, "set_documents: offsets must be non-decreasing%s");
    const int64_t total = host_offsets[n];
    if (total > 0 && !host_bytes) return fail(CODD_KNN_EINVAL, "set_documents: null bytes%s");
    if (total > 0 && memchr(host_bytes, 0, (size_t)total)) return fail(CODD_KNN_EINVAL, "set_documents: a document holds a 0x00 byte%s");
    DeviceGuard guard(ix->device);
    HIP_TRY(hipDeviceSynchronize());
    // the arena on the host first: document r at host_offsets[r] + r, its separator behind it, zeros to the end of the allocation
    const int64_t bytes = total + n, alloc = doc_arena_alloc_bytes(bytes);
    std::vector<uint8_t> arena;
    std::vector<int64_t> offsets;
    try {
        arena.assign((size_t)alloc, (uint8_t)0);
        offsets.resize((size_t)n + 1);
    } catch (const std::bad_alloc&) {
        return fail(CODD_KNN_ENOMEM, "host allocation failed%s");
    }
    for (int64_t r = 0; r < n; ++r) {
        offsets[(size_t)r] = host_offsets[r] + r;
        const int64_t len = host_offsets[r + 1] - host_offsets[r];
        if (len > 0) memcpy(arena.data() + offsets[(size_t)r], host_bytes + host_offsets[r], (size_t)len);
    }
    offsets[(size_t)n] = bytes;
    DevBuf<uint8_t> dev_arena;
    DevBuf<int64_t> dev_offsets;
    hipError_t e = dev_arena.reset(alloc);
    if (e == hipSuccess) e = dev_offsets.reset(n + 1);
    if (e == hipSuccess) e = hipMemcpy(dev_arena, arena.data(), (size_t)alloc, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dev_offsets, offsets.data(), ((size_t)n + 1) * sizeof(int64_t), hipMemcpyHostToDevice);
    // (on failure the previous snapshot stays as it was)
    if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? CODD_KNN_ENOMEM : CODD_KNN_EDEVICE, "set_documents: upload failed: %s", hipGetErrorString(e));
    ix->doc_arena = std::move(dev_arena);
    ix->doc_offsets = std::move(dev_offsets);
    ix->doc_bytes = bytes;
    ix->doc_count = n;
    ix->doc_epoch = ix->epoch;
    return CODD_KNN_OK;
}

int codd_knn_match_documents(codd_knn_index* ix, const uint8_t* host_needle, int needle_len, uint32_t* dev_bits, int64_t nwords, void* stream) {
    if (!ix || !host_needle) return fail(CODD_KNN_EINVAL, "match_documents: null index or needle%s");
    if (needle_len < 1 || needle_len > CODD_KNN_MAX_NEEDLE) return fail(CODD_KNN_EINVAL, "match_documents: needle_len out of range [1,256]%s");
    if (memchr(host_needle, 0, (size_t)needle_len)) return fail(CODD_KNN_EINVAL, "match_documents: the needle holds a 0x00 byte%s");
    static_assert(kDocMaxNeedle == CODD_KNN_MAX_NEEDLE, "doc_match.h and codd_knn.h disagree");
    DeviceGuard guard(ix->device);
    hipStream_t st = (hipStream_t)stream;
    std::lock_guard<std::mutex> lock(ix->mu);   // (no workspace: the kernel reads the snapshot and writes the caller's words)
    if (!docs_valid(ix)) return fail(CODD_KNN_EINVAL, "match_documents: no document snapshot, or a stale one (rows changed since codd_knn_set_documents_host)%s");
    if (nwords != (ix->count + 31) / 32) return fail(CODD_KNN_EINVAL, "match_documents: nwords must be ceil(count / 32)%s");
    if (nwords == 0) return CODD_KNN_OK;
    if (!dev_bits) return fail(CODD_KNN_EINVAL, "match_documents: null bits%s");
    DocNeedle needle;
    memset(&needle, 0, sizeof(needle));
    memcpy(needle.w, host_needle, (size_t)needle_len);
    HIP_TRY(hipMemsetAsync(dev_bits, 0, (size_t)nwords * sizeof(uint32_t), st));
    const int64_t tiles = (ix->doc_bytes + kDocTile - 1) / kDocTile;
    const int64_t most = (int64_t)ix->num_cus * 8;   // (grid-stride beyond eight workgroups per compute unit)
    const int rc = launch_kernel<doc_match_kernel>(dim3((unsigned)(tiles < most ? tiles : most)), dim3(kDocThreads), 0, st,
                                                   reinterpret_cast<const uint4*>(ix->doc_arena.get()), ix->doc_bytes, tiles, ix->doc_offsets, ix->count, needle,
                                                   needle_len, dev_bits);
    if (rc != 0) return rc;
    HIP_TRY(hipGetLastError());
    ix->stat_doc_matches++;
    return CODD_KNN_OK;
}

int codd_knn_embedder_create(codd_knn_embedder** out, int device, int dim, float trigram_weight) {
    if (!out) return fail(CODD_KNN_EINVAL, "embedder_create: null out pointer%s");
    *out = nullptr;
    static_assert(kEmbedMaxDim == 4096 && kEmbedMinDim == 8, "text_embed.h and codd_knn.h disagree");
    if (dim < kEmbedMinDim || dim > kEmbedMaxDim) return fail(CODD_KNN_EINVAL, "embedder_create: dim out of range [8,4096]%s");
    if (!(trigram_weight - trigram_weight == 0.0f)) return fail(CODD_KNN_EINVAL, "embedder_create: trigram_weight must be finite%s");
    if (device < 0) return fail(CODD_KNN_EINVAL, "embedder_create: no such device%s");
    codd_knn_embedder* e = new (std::nothrow) codd_knn_embedder();
    if (!e) return fail(CODD_KNN_ENOMEM, "host allocation failed%s");
    e->device = device;
    e->dim = dim;
    e->trigram_weight = trigram_weight;
    *out = e;
    return CODD_KNN_OK;
}

int codd_knn_embedder_destroy(codd_knn_embedder* e) {
    if (!e) return CODD_KNN_OK;
    if (e->device_seen) {   // (its buffers and events free themselves: the device is current and idle, as their destructors need)
        DeviceGuard guard(e->device);
        (void)hipDeviceSynchronize();
        delete e;
    } else {
        delete e;
    }
    return CODD_KNN_OK;
}

int codd_knn_embed_texts_host(codd_knn_embedder* e, const uint8_t* host_bytes, const int64_t* host_offsets, int64_t n, float* dev_out, void* stream) {
    if (!e || !host_offsets || n < 0) return fail(CODD_KNN_EINVAL, "embed_texts: null embedder or offsets, or negative n%s");
    if (n > CODD_KNN_MAX_EMBED_TEXTS) return fail(CODD_KNN_EINVAL, "embed_texts: more than CODD_KNN_MAX_EMBED_TEXTS texts%s");
    if (host_offsets[0] != 0) return fail(CODD_KNN_EINVAL, "embed_texts: offsets must start at 0%s");
    for (int64_t r = 0; r < n; ++r)
        if (host_offsets[r + 1] < host_offsets[r]) return fail(CODD_KNN_EINVAL, "embed_texts: offsets must be non-decreasing%s");
    const int64_t total = host_offsets[n];
    if (total > CODD_KNN_MAX_EMBED_BYTES) return fail(CODD_KNN_EINVAL, "embed_texts: more than CODD_KNN_MAX_EMBED_BYTES bytes of text%s");
    if (total > 0 && !host_bytes) return fail(CODD_KNN_EINVAL, "embed_texts: null bytes%s");
    unsigned char seen = 0;
    for (int64_t i = 0; i < total; ++i) seen |= host_bytes[i];
    if (seen & 0x80) return fail(CODD_KNN_EINVAL, "embed_texts: a byte at or above 0x80 (ASCII only: other texts are embedded on the host)%s");
    if (n == 0) return CODD_KNN_OK;
    if (!dev_out) return fail(CODD_KNN_EINVAL, "embed_texts: null output%s");
    std::lock_guard<std::mutex> lock(e->mu);
    if (!e->device_seen) {
        int ndev = 0;
        HIP_TRY(hipGetDeviceCount(&ndev));
        if (e->device >= ndev) return fail(CODD_KNN_EINVAL, "embed_texts: no such device%s");
        e->device_seen = true;
    }
    DeviceGuard guard(e->device);
    hipStream_t st = (hipStream_t)stream;
    // the staging buffer: the previous call's copy has to have left it — the only wait on the host; its kernel is not waited for
    if (e->upload_pending) HIP_TRY(hipEventSynchronize(e->uploaded));
    e->upload_pending = false;
    const int64_t off_bytes = (n + 1) * (int64_t)sizeof(int64_t), need = off_bytes + total;
    if (need > e->stage_host.cap()) HIP_TRY(e->stage_host.reset(need + need / 2 + 4096));
    HIP_TRY(e->stage_dev.ensure(e->stage_host.cap()));
    HIP_TRY(e->uploaded.ensure());
    HIP_TRY(e->embedded.ensure());
    memcpy(e->stage_host.get(), host_offsets, (size_t)off_bytes);
    if (total > 0) memcpy(e->stage_host.get() + off_bytes, host_bytes, (size_t)total);
    // the device copy may still be read by the previous call's kernel on another stream: this stream waits for it on the device
    if (e->embedded_set && e->last_stream != st) HIP_TRY(hipStreamWaitEvent(st, e->embedded, 0));
    HIP_TRY(hipMemcpyAsync(e->stage_dev, e->stage_host, (size_t)need, hipMemcpyHostToDevice, st));
    HIP_TRY(hipEventRecord(e->uploaded, st));
    e->upload_pending = true;
    const int64_t most = (int64_t)1 << 20;   // (grid-stride beyond that many texts)
    const int rc = launch_kernel<text_embed_kernel>(dim3((unsigned)(n < most ? n : most)), dim3(kEmbedThreads), (size_t)e->dim * sizeof(float), st,
                                                    (const uint8_t*)(e->stage_dev.get() + off_bytes), reinterpret_cast<const int64_t*>(e->stage_dev.get()), n,
                                                    e->dim, e->trigram_weight, dev_out);
    if (rc != 0) return rc;
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(e->embedded, st));
    e->embedded_set = true;
    e->last_stream = st;
    return CODD_KNN_OK;
}

int codd_knn_delete_host(codd_knn_index* ix, const int64_t* host_slots, int64_t n) {
    if (!ix || n < 0 || (n > 0 && !host_slots)) return fail(CODD_KNN_EINVAL, "bad delete arguments%s");
    for (int64_t i = 0; i < n; ++i)
        if (host_slots[i] < 0 || host_slots[i] >= ix->count) return fail(CODD_KNN_EINVAL, "delete: row slot outside [0, count)%s");
    if (n == 0) return CODD_KNN_OK;
    DeviceGuard guard(ix->device);
    HIP_TRY(hipDeviceSynchronize());
    int rc;
    if ((rc = grow_dead_bits(ix, ix->capacity)) != 0) return rc;
    // the slots that are not dead yet, each once (an already-dead or repeated slot is a no-op): marked in the host mirror first,
    // taken back if the device cannot follow
    std::vector<int64_t> fresh;
    try {
        for (int64_t i = 0; i < n; ++i) {
            uint32_t& word = ix->dead_host[(size_t)(host_slots[i] >> 5)];
            const uint32_t bit = 1u << (uint32_t)(host_slots[i] & 31);
            if (word & bit) continue;
            fresh.push_back(host_slots[i]);
            word |= bit;
        }
    } catch (const std::bad_alloc&) {
        for (int64_t slot : fresh) ix->dead_host[(size_t)(slot >> 5)] &= ~(1u << (uint32_t)(slot & 31));
        return fail(CODD_KNN_ENOMEM, "host allocation failed%s");
    }
    auto undo = [&]() {
        for (int64_t slot : fresh) ix->dead_host[(size_t)(slot >> 5)] &= ~(1u << (uint32_t)(slot & 31));
        if (ix->dead_bits) (void)hipMemcpy(ix->dead_bits, ix->dead_host.data(), (size_t)ix->dead_bits.bytes(), hipMemcpyHostToDevice);
    };
    // the staging buffer codd_knn_upsert_host keeps between calls, grown once to hold the call's slots (at most 1M of them, 8 MiB:
    // a piece costs a copy, a launch and a synchronisation — 5M slots through 4,096-slot pieces were 1,221 such round trips)
    const int64_t total = (int64_t)fresh.size();
    const int64_t want = total < 4096 ? 4096 : (total < (1ll << 20) ? total : (1ll << 20));
    if (ix->stage_slot.cap() < want && ix->stage_slot.reset(want) != hipSuccess) {
        (void)hipGetLastError();
        undo();
        return fail(CODD_KNN_ENOMEM, "delete: staging buffer%s");
    }
    const int64_t pn = ix->stage_slot.cap();
    for (int64_t i0 = 0; i0 < total; i0 += pn) {
        const int64_t m = total - i0 < pn ? total - i0 : pn;
        hipError_t e = hipMemcpy(ix->stage_slot, fresh.data() + i0, (size_t)m * sizeof(int64_t), hipMemcpyHostToDevice);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(dead_set_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, nullptr, ix->stage_slot, m, ix->dead_bits);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipDeviceSynchronize();  // (the staging buffer is reused by the next piece, and the call is synchronous by contract)
        if (e != hipSuccess) {
            undo();
            return fail(CODD_KNN_EDEVICE, "delete: setting the tombstone bits failed: %s", hipGetErrorString(e));
        }
    }
    ix->stat_delete_calls++;
    if (total == 0) return CODD_KNN_OK;
    ix->dead_count += total;
    for (int64_t slot : fresh)
        if (slot < ix->first_dead) ix->first_dead = slot;
    ix->scope_gen++;  // the scope lists leave dead rows out: rebuilt by the next scoped search, like after a label change
    // (no epoch bump: the stored rows and both shadows are what they were, and an installed IVF layout stays valid — its scans
    //  mask by the original row slot)
    return CODD_KNN_OK;
}

int codd_knn_live_count(const codd_knn_index* ix, int64_t* out) {
    if (!ix || !out) return fail(CODD_KNN_EINVAL, "bad live_count arguments%s");
    *out = ix->count - ix->dead_count;
    return CODD_KNN_OK;
}

int codd_knn_compact(codd_knn_index* ix, int64_t* new_count) {
    if (!ix) return fail(CODD_KNN_EINVAL, "null index%s");
    if (ix->dead_count == 0) {
        if (new_count) *new_count = ix->count;
        return CODD_KNN_OK;
    }
    DeviceGuard guard(ix->device);
    HIP_TRY(hipDeviceSynchronize());
    const int64_t n = ix->count, live = n - ix->dead_count, first = ix->first_dead;
    const size_t row_bytes = (size_t)ix->dpad * elem_size(ix->dtype);
    const int cpr = (int)(row_bytes / 16);
    // source rows per chunk: what the bounce buffer (the staging buffer of codd_knn_upsert_host, at most 64 MiB) holds
    int64_t chunk = ix->compact_chunk_rows > 0 ? ix->compact_chunk_rows : (int64_t)((64ull << 20) / row_bytes);
    if (chunk > n - first) chunk = n - first;
    if (chunk < 1) chunk = 1;
    const int64_t bounce_floats = (chunk * (int64_t)row_bytes + 3) / 4;
    if (bounce_floats > ix->stage_vec.cap()) HIP_TRY(ix->stage_vec.reset(bounce_floats < 65536 ? 65536 : bounce_floats));
    if ((chunk + 1) / 2 > ix->stage_slot.cap())  // the chunk's scope labels, 4 bytes each
        HIP_TRY(ix->stage_slot.reset((chunk + 1) / 2 < 4096 ? 4096 : (chunk + 1) / 2));
    // new slot of a live row = its rank among the live rows: prefix sums over the bitmap, on the device
    const int64_t nwords = (n + 31) / 32, nblocks = (nwords + 255) / 256;
    DevBuf<unsigned> sums;   // [nwords] per-word prefix, [nblocks] block totals, [nblocks + 1] block bases
    HIP_TRY(sums.reset(nwords + 2 * nblocks + 1));
    unsigned* prefix = sums;
    unsigned* block_total = prefix + nwords;
    unsigned* block_base = block_total + nblocks;
    hipLaunchKernelGGL(live_prefix_kernel, dim3((unsigned)nblocks), dim3(256), 0, nullptr, ix->dead_bits, n, nwords, prefix, block_total);
    hipLaunchKernelGGL(scope_offsets_kernel, dim3(1), dim3(1024), 0, nullptr, block_total, (int)nblocks, block_base);
    hipError_t e = hipGetLastError();
    // ascending chunks of source rows from the first dead slot on (the rows below it stay where they are), ordered on one stream
    uint4* rows4 = reinterpret_cast<uint4*>(ix->rows.get());
    uint4* bounce = reinterpret_cast<uint4*>(ix->stage_vec.get());
    uint32_t* bounce_scope = reinterpret_cast<uint32_t*>(ix->stage_slot.get());
    int64_t dbase = first;  // every slot below the first dead one is live
    for (int64_t s0 = first; s0 < n && e == hipSuccess; s0 += chunk) {
        const int64_t s1 = s0 + chunk < n ? s0 + chunk : n;
        const int64_t moved = live_in_range(ix, s0, s1);
        if (moved == 0) continue;
        hipLaunchKernelGGL(compact_gather_kernel, dim3((unsigned)((s1 - s0 + 3) / 4)), dim3(256), 0, nullptr, rows4, ix->dead_bits, n, prefix, block_base,
                           ix->scope_of, s0, s1, dbase, chunk, cpr, bounce, bounce_scope);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(ix->rows + (size_t)dbase * row_bytes, bounce, (size_t)moved * row_bytes, hipMemcpyDeviceToDevice, nullptr);
        if (e == hipSuccess && ix->scope_of)
            e = hipMemcpyAsync(ix->scope_of + dbase, bounce_scope, (size_t)moved * sizeof(uint32_t), hipMemcpyDeviceToDevice, nullptr);
        dbase += moved;
    }
    // the slots past the live rows are new slots again: no label, no tombstone; the int8 shadow's scales there read "no such row"
    // ... and zero rows: a later write past the new count that does not regrow the store brings them back below the count
    if (e == hipSuccess) e = hipMemsetAsync(ix->rows + (size_t)live * row_bytes, 0, (size_t)(n - live) * row_bytes, nullptr);
    if (e == hipSuccess && ix->scope_of) e = hipMemsetAsync(ix->scope_of + live, 0, (size_t)(n - live) * sizeof(uint32_t), nullptr);
    if (e == hipSuccess) e = hipMemsetAsync(ix->dead_bits, 0, (size_t)ix->dead_bits.bytes(), nullptr);
    if (e == hipSuccess && ix->rscale) {
        const int64_t hi = n < ix->shadow8_rows ? n : ix->shadow8_rows;
        if (hi > live) e = hipMemsetD32Async((hipDeviceptr_t)(ix->rscale + live), (int)0x7fc00000, (size_t)(hi - live), nullptr);
        const int64_t b0 = (live + 31) / 32, b1 = (hi + 31) / 32;
        if (e == hipSuccess && b1 > b0) e = hipMemsetD32Async((hipDeviceptr_t)(ix->bmeta + b0), (int)0x7fc00000, (size_t)(b1 - b0) * 2, nullptr);
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    // A device failure in the middle leaves rows partly moved under an unchanged bitmap and count: the index is unusable from
    // then on (destroy it and rebuild the collection), as the header says.  Nothing short of a device error gets here.
    if (e != hipSuccess) return fail(CODD_KNN_EDEVICE, "compaction failed, the index is unusable: %s", hipGetErrorString(e));
    if (dbase != live) return fail(CODD_KNN_EDEVICE, "compaction: the host's row mapping disagrees with its dead count%s");
    std::fill(ix->dead_host.begin(), ix->dead_host.end(), 0u);
    ix->count = live;
    ix->dead_count = 0;
    ix->first_dead = INT64_MAX;
    ix->rows_event_set = false;  // (everything is complete on the device)
    ix->reader_event_set = false;
    // both shadows are dirty from the first dead slot on (and the last live row's 32-row block is quantised again: its scale
    // spanned rows that are gone); the epoch bump makes an installed IVF layout stale, as after an upsert
    // A dirty range still pending from earlier upserts may reach past the new count (the count never shrank before compaction
    // existed): cut it back first — a shadow build over rows past the count would write past a shadow sized for the count.
    // Every pending dirty row at or behind `first` has moved to a slot in [first, live): the widened range below covers it.
    auto cut = [&](int64_t& dlo, int64_t& dhi) {
        if (dhi > live) dhi = live;
        if (dlo > dhi) dlo = dhi;
    };
    cut(ix->dirty_lo, ix->dirty_hi);
    cut(ix->dirty16_lo, ix->dirty16_hi);
    const int64_t lo = live > 0 ? (first < live - 1 ? first : live - 1) : 0;
    rows_written(ix, lo, live);
    ix->scope_gen++;
    ix->stat_compactions++;
    if (new_count) *new_count = live;
    return CODD_KNN_OK;
}

#ifdef CODD_I8_EXP_STAMPS
// diagnostic builds only (not in include/codd_knn.h): the per-wave phase stamps of the last i8_tile_kernel<FILTER> launch on `stream`'s
// workspace — [workgroup][wave][8] u64: issue, corpus wait, MFMA phase, end-of-interval sync, epilogue, intervals, total, tiles
int codd_knn_exp_read_stamps(codd_knn_index* ix, unsigned long long* host_out, int n_u64, void* stream) {
    if (!ix || !host_out) return CODD_KNN_EINVAL;
    WorkScope work(ix, (hipStream_t)stream);
    if (!ix->bucket_max || (int64_t)n_u64 > ix->bucket_max.cap()) return CODD_KNN_EINVAL;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(host_out, ix->bucket_max, (size_t)n_u64 * 8, hipMemcpyDeviceToHost));
    return CODD_KNN_OK;
}
#endif

int codd_knn_set_option(codd_knn_index* ix, const char* key, int64_t value) {
    if (!ix || !key) return fail(CODD_KNN_EINVAL, "bad option arguments%s");
    if (strcmp(key, "scan_blocks_per_cu") == 0) {
        if (value < 1 || value > 8) return fail(CODD_KNN_EINVAL, "scan_blocks_per_cu must be in [1,8]%s");
        ix->scan_blocks_per_cu = (int)value;
        return CODD_KNN_OK;
    }
    if (strcmp(key, "filter") == 0) { ix->filter_enabled = value != 0; return CODD_KNN_OK; }
    if (strcmp(key, "filter_min_rows") == 0) { ix->filter_min_rows = value < 1 ? 1 : value; return CODD_KNN_OK; }
    if (strcmp(key, "filter_min_rows_small") == 0) { ix->filter_min_rows_small = value < 1 ? 1 : value; return CODD_KNN_OK; }
    if (strcmp(key, "filter_min_batch") == 0) { ix->filter_min_batch = value < 1 ? 1 : (int)value; return CODD_KNN_OK; }
    if (strcmp(key, "shadow8") == 0) {
        if (value != 0 && value != 1) return fail(CODD_KNN_EINVAL, "shadow8 must be 0 or 1%s");
        ix->shadow8_enabled = (int)value;
        return CODD_KNN_OK;
    }
    if (strcmp(key, "space_filter") == 0) {  // the int8 filter leg of an ip or l2 index; no effect on a cosine index
        if (value != 0 && value != 1) return fail(CODD_KNN_EINVAL, "space_filter must be 0 or 1%s");
        ix->space_filter = (int)value;
        return CODD_KNN_OK;
    }
    if (strcmp(key, "space_ivf") == 0) {  // IVF on an ip or l2 index; no effect on a cosine index
        if (value != 0 && value != 1) return fail(CODD_KNN_EINVAL, "space_ivf must be 0 or 1%s");
        ix->space_ivf = (int)value;
        return CODD_KNN_OK;
    }
    if (strcmp(key, "shadow8_max_batch") == 0) {
        if (value < 1 || value > 256) return fail(CODD_KNN_EINVAL, "shadow8_max_batch must be in [1,256]%s");
        ix->shadow8_max_batch = (int)value;
        return CODD_KNN_OK;
    }
    if (strcmp(key, "shadow8_max_surv") == 0) {
        if (value < 1 || value > 1000000) return fail(CODD_KNN_EINVAL, "shadow8_max_surv must be in [1,1000000]%s");
        ix->shadow8_max_surv = (int)value;
        return CODD_KNN_OK;
    }
    if (strcmp(key, "shadow8_cooldown") == 0) {
        if (value < 0 || value > 1000000) return fail(CODD_KNN_EINVAL, "shadow8_cooldown must be in [0,1000000]%s");
        ix->shadow8_cooldown = (int)value;
        ix->cooldown_left = 0;
        return CODD_KNN_OK;
    }
#if CODD_EXPERIMENTS
    if (strcmp(key, "exp_slack_pct") == 0) {  // what-if timing only, experiment builds only: < 100 makes the int8 filter UNSOUND
        if (value < 1 || value > 100) return fail(CODD_KNN_EINVAL, "exp_slack_pct must be in [1,100]%s");
        ix->exp_slack_scale = (float)value / 100.0f;
        return CODD_KNN_OK;
    }
#endif
    if (strcmp(key, "debug_fail_shadow_alloc") == 0) {  // test hook: the bf16 shadow's allocation fails as if HBM were full
        ix->debug_fail_shadow_alloc = value != 0;
        if (!value) ix->shadow_nomem_epoch = -1;
        return CODD_KNN_OK;
    }
    if (strcmp(key, "all_normalized") == 0) {
        // 0: the caller knows of rows that are not unit vectors (a persisted index written with normalize = 0): both filters
        // off, every search takes the exact scan.  The flag cannot be switched back on from outside.
        if (value != 0) return fail(CODD_KNN_EINVAL, "all_normalized can only be cleared (0)%s");
        ix->all_normalized = false;
        return CODD_KNN_OK;
    }
    if (strcmp(key, "i8v2") == 0) {
        if (value < 0 || value > 2) return fail(CODD_KNN_EINVAL, "i8v2 must be 0, 1 or 2%s");
        ix->i8v2 = (int)value;
        return CODD_KNN_OK;
    }
    if (strcmp(key, "f16_tile") == 0) {
        if (value != 0 && value != 1) return fail(CODD_KNN_EINVAL, "f16_tile must be 0 or 1%s");
        ix->f16_tile = (int)value;
        return CODD_KNN_OK;
    }
    if (strcmp(key, "ivf_share") == 0) {
        if (value != 0 && value != 1) return fail(CODD_KNN_EINVAL, "ivf_share must be 0 or 1%s");
        ix->ivf_share = (int)value;
        return CODD_KNN_OK;
    }
    if (strcmp(key, "fuse_fallback") == 0) {
        if (value != 0 && value != 1) return fail(CODD_KNN_EINVAL, "fuse_fallback must be 0 or 1%s");
        ix->fuse_fallback = (int)value;
        return CODD_KNN_OK;
    }
    if (strcmp(key, "small_batch_max") == 0) {
        if (value < 0 || value > 1) return fail(CODD_KNN_EINVAL, "small_batch_max must be 0 or 1%s");
        ix->small_batch_max = (int)value;
        return CODD_KNN_OK;
    }
    if (strcmp(key, "per_block") == 0) {
        if (value < 0 || value > 7) return fail(CODD_KNN_EINVAL, "per_block must be in [0,7]%s");
        ix->per_block = (int)value;
        return CODD_KNN_OK;
    }
    if (strcmp(key, "i8_pair") == 0) {
        if (value < 0 || value > 2) return fail(CODD_KNN_EINVAL, "i8_pair must be 0, 1 or 2%s");
        ix->i8_pair = (int)value;
        return CODD_KNN_OK;
    }
    if (strcmp(key, "i8v2_half") == 0) {
        if (value != 0 && value != 1) return fail(CODD_KNN_EINVAL, "i8v2_half must be 0 or 1%s");
        ix->i8v2_half = (int)value;
        return CODD_KNN_OK;
    }
    if (strcmp(key, "resident_q") == 0) {
        if (value != 0 && value != 1) return fail(CODD_KNN_EINVAL, "resident_q must be 0 or 1%s");
        ix->resident_q = (int)value;
        return CODD_KNN_OK;
    }
    if (strcmp(key, "sample_rounds8") == 0) {
        if (value < 1 || value > 16) return fail(CODD_KNN_EINVAL, "sample_rounds8 must be in [1,16]%s");
        ix->sample_rounds8 = (int)value;
        return CODD_KNN_OK;
    }
    if (strcmp(key, "sample_div8") == 0) {
        if (value < 1 || value > 1000) return fail(CODD_KNN_EINVAL, "sample_div8 must be in [1,1000]%s");
        ix->sample_div8 = (int)value;
        return CODD_KNN_OK;
    }
    if (strcmp(key, "sample_tiles") == 0) {
        if (value < 1 || value > 65536) return fail(CODD_KNN_EINVAL, "sample_tiles must be in [1,65536]%s");
        ix->sample_tiles = (int)value;
        return CODD_KNN_OK;
    }
    if (strcmp(key, "sample_div") == 0) {
        if (value < 1 || value > 4096) return fail(CODD_KNN_EINVAL, "sample_div must be in [1,4096]%s");
        ix->sample_div = (int)value;
        return CODD_KNN_OK;
    }
    if (strcmp(key, "compact_chunk_rows") == 0) {
        if (value < 0 || value > (1ll << 32)) return fail(CODD_KNN_EINVAL, "compact_chunk_rows must be in [0,2^32]%s");
        ix->compact_chunk_rows = value;
        return CODD_KNN_OK;
    }
    if (strcmp(key, "mask_route") == 0) {
        if (value < 0 || value > 2) return fail(CODD_KNN_EINVAL, "mask_route must be 0 (auto), 1 (list) or 2 (dense)%s");
        ix->mask_route = (int)value;
        return CODD_KNN_OK;
    }
    if (strcmp(key, "mask_list_pct") == 0) {
        if (value < 0 || value > 100000) return fail(CODD_KNN_EINVAL, "mask_list_pct must be in [0,100000]%s");
        ix->mask_list_pct = (int)value;
        return CODD_KNN_OK;
    }
    if (strcmp(key, "hit_cap") == 0) {
        if (value < 16 || value > (1 << 20)) return fail(CODD_KNN_EINVAL, "hit_cap must be in [16,2^20]%s");
        ix->hit_cap_q = (int)value;
        return CODD_KNN_OK;
    }
    if (strcmp(key, "profile") == 0) {
        // value = number of (start, stop) event pairs to keep (0 switches timing off); resets the log
        if (value < 0 || value > 65536) return fail(CODD_KNN_EINVAL, "profile pairs must be in [0,65536]%s");
        DeviceGuard guard(ix->device);
        while ((int64_t)ix->ev.size() < 2 * value) {
            Event e;
            HIP_TRY(e.ensure(hipEventDefault));
            ix->ev.push_back(std::move(e));
        }
        ix->ev_kind.assign(ix->ev.size() / 2, 0);
        ix->profile = value > 0;
        ix->ev_used = 0;
        return CODD_KNN_OK;
    }
    return fail(CODD_KNN_EINVAL, "unknown option: %s", key);
}

int codd_knn_debug_live_allocations(int64_t* buffers, int64_t* bytes, int64_t* events) {
    if (!buffers || !bytes || !events) return fail(CODD_KNN_EINVAL, "debug_live_allocations: null output%s");
    *buffers = g_live_buffers.load();
    *bytes = g_live_bytes.load();
    *events = g_live_events.load();
    return CODD_KNN_OK;
}

int codd_knn_get_stat(const codd_knn_index* ix, const char* key, int64_t* out) {
    if (!ix || !key || !out) return fail(CODD_KNN_EINVAL, "bad stat arguments%s");
    // "time_ns:<kernel>" / "events:<kernel>" with kernel in {scan, filter, sample, finalize}
    const bool want_time = strncmp(key, "time_ns:", 8) == 0, want_events = strncmp(key, "events:", 7) == 0;
    if (want_time || want_events) {
        const char* name = key + (want_time ? 8 : 7);
        int kind = -1;
        for (int i = 0; i < EV_KINDS; ++i)
            if (strcmp(name, kEvNames[i]) == 0) kind = i;
        if (kind < 0) return fail(CODD_KNN_EINVAL, "unknown kernel name in stat: %s", key);
        double total_ms = 0.0;
        int64_t events = 0;
        if (ix->ev_used > 0) {
            DeviceGuard guard(ix->device);
            HIP_TRY(hipEventSynchronize(ix->ev[2 * ix->ev_used - 1]));
            for (int i = 0; i < ix->ev_used; ++i) {
                if (ix->ev_kind[i] != kind) continue;
                float ms = 0.0f;
                HIP_TRY(hipEventElapsedTime(&ms, ix->ev[2 * i], ix->ev[2 * i + 1]));
                total_ms += ms;
                events++;
            }
        }
        *out = want_time ? (int64_t)(total_ms * 1e6) : events;
        return CODD_KNN_OK;
    }
    if (strcmp(key, "searches") == 0) *out = ix->stat_searches;
    else if (strcmp(key, "scan_launches") == 0) *out = ix->stat_scan_launches;
    else if (strcmp(key, "last_scan_blocks") == 0) *out = ix->stat_last_scan_blocks;
    else if (strcmp(key, "last_scan_group") == 0) *out = ix->stat_last_scan_group;
    else if (strcmp(key, "last_finalize_parts") == 0) *out = ix->stat_last_finalize_parts;
    else if (strcmp(key, "ivf_shared_searches") == 0) *out = ix->stat_ivf_shared;
    else if (strcmp(key, "ivf_masked_searches") == 0) *out = ix->stat_ivf_masked;
    else if (strcmp(key, "scoped_searches") == 0) *out = ix->stat_scoped_searches;
    else if (strcmp(key, "scope_builds") == 0) *out = ix->stat_scope_builds;
    else if (strcmp(key, "scopes") == 0) *out = (int64_t)ix->max_scope;
    else if (strcmp(key, "masked_searches") == 0) *out = ix->stat_masked_searches;
    else if (strcmp(key, "mask_list_searches") == 0) *out = ix->stat_mask_list;
    else if (strcmp(key, "mask_dense_searches") == 0) *out = ix->stat_mask_dense;
    else if (strcmp(key, "last_mask_rows") == 0) *out = ix->stat_last_mask_rows;
    else if (strcmp(key, "masked_dev_searches") == 0) *out = ix->stat_masked_dev;
    else if (strcmp(key, "docs_valid") == 0) *out = docs_valid(ix) ? 1 : 0;
    else if (strcmp(key, "doc_bytes") == 0) *out = ix->doc_arena ? ix->doc_bytes : 0;
    else if (strcmp(key, "doc_tile_bytes") == 0) *out = kDocTile;
    else if (strcmp(key, "doc_matches") == 0) *out = ix->stat_doc_matches;
    else if (strcmp(key, "dead_rows") == 0) *out = ix->dead_count;
    else if (strcmp(key, "delete_calls") == 0) *out = ix->stat_delete_calls;
    else if (strcmp(key, "compactions") == 0) *out = ix->stat_compactions;
    else if (strcmp(key, "filter_passes") == 0) *out = ix->stat_filter_passes;
    else if (strcmp(key, "shadow8_builds") == 0) *out = ix->stat_shadow8_builds;
    else if (strcmp(key, "shadow16_builds") == 0) *out = ix->stat_shadow_builds;
    else if (strcmp(key, "shadow16_alloc_failures") == 0) *out = ix->stat_shadow_nomem;
    else if (strcmp(key, "all_normalized") == 0) *out = ix->all_normalized ? 1 : 0;
    else if (strcmp(key, "metric") == 0) *out = ix->metric;
    else if (strcmp(key, "space_filter") == 0) *out = ix->space_filter;
    else if (strcmp(key, "space_ivf") == 0) *out = ix->space_ivf;
    else if (strcmp(key, "shadow8_passes") == 0) *out = ix->stat_shadow8_passes;
    else if (strcmp(key, "i8v2_passes") == 0) *out = ix->stat_i8v2_passes;
    else if (strcmp(key, "f16_tile_passes") == 0) *out = ix->stat_f16_tile_passes;
    else if (strcmp(key, "small_batch_passes") == 0) *out = ix->stat_small_batch;
    else if (strcmp(key, "shadow8_cooldowns") == 0) *out = ix->stat_cooldowns;
    else if (strcmp(key, "shadow8_wide_blocks") == 0) {  // blocks whose error norm exceeds shadow8_max_eps, as last read back
        if (ix->eps_r_copied && hipEventQuery(ix->eps_r_copied) == hipSuccess) *out = (int64_t)reinterpret_cast<const unsigned*>(ix->eps_r_host.get())[1];
        else {
            (void)hipGetLastError();
            *out = ix->wide_blocks_known;
        }
    }
    else if (strcmp(key, "shadow8_eps_r_micro") == 0) {  // worst row's quantisation error norm x 1e6, as last read back
        if (ix->eps_r_copied && hipEventQuery(ix->eps_r_copied) == hipSuccess) *out = (int64_t)(ix->eps_r_host[0] * 1e6f);
        else {
            (void)hipGetLastError();
            *out = (int64_t)(ix->eps_r_known * 1e6f);
        }
    }
    else if (strcmp(key, "fallback_queries") == 0 || strcmp(key, "filter_hits") == 0 || strcmp(key, "filter_survivors") == 0) {
        // device-side counters (the search itself never reads them back): synchronises
        unsigned long long h[4] = {0, 0, 0, 0};
        if (ix->dstats) {
            DeviceGuard guard(ix->device);
            HIP_TRY(hipDeviceSynchronize());
            HIP_TRY(hipMemcpy(h, ix->dstats, sizeof(h), hipMemcpyDeviceToHost));
        }
        *out = (int64_t)(key[0] == 'f' && key[1] == 'a' ? h[2] : (strcmp(key, "filter_hits") == 0 ? h[0] : h[1]));
    }
    else if (strcmp(key, "mask_filter_hits") == 0 || strcmp(key, "mask_filter_survivors") == 0 || strcmp(key, "mask_fallback_queries") == 0) {
        // the same device counters, of the dense masked passes alone: synchronises
        unsigned long long h[4] = {0, 0, 0, 0};
        if (ix->mask_dstats) {
            DeviceGuard guard(ix->device);
            HIP_TRY(hipDeviceSynchronize());
            HIP_TRY(hipMemcpy(h, ix->mask_dstats, sizeof(h), hipMemcpyDeviceToHost));
        }
        *out = (int64_t)(key[12] == 'h' ? h[0] : (key[12] == 's' ? h[1] : h[2]));
    }
    else if (strcmp(key, "capacity_rows") == 0) *out = ix->capacity;
    else if (strcmp(key, "num_cus") == 0) *out = ix->num_cus;
    else if (strcmp(key, "device_bytes") == 0) {
        int64_t b = ix->capacity * (int64_t)ix->dpad * (int64_t)elem_size(ix->dtype) + ix->shadow_rows * (int64_t)ix->dpad * 2 +
                    ix->shadow8_rows * ((int64_t)dpad8_of(ix) + 4) + ix->scope_of.bytes() + ix->scope_perm.bytes() + ix->scope_offsets.bytes() + ix->dead_bits.bytes() +
                    ix->doc_arena.bytes() + ix->doc_offsets.bytes();
        for (const WorkSlot& w : ix->slots)
            b += w.bufs.qn.bytes() + w.bufs.partial.bytes() + w.bufs.keys_tmp.bytes() + w.bufs.hits.bytes() + w.bufs.bucket_max.bytes() +
                 w.bufs.qfrag.bytes() + w.bufs.fb_partial.bytes() + w.bufs.probe_keys.bytes() + w.bufs.ivf_partial.bytes();
        *out = b;  // (the terms it has always had: DESIGN.md §18 lists what it leaves out)
    } else if (strcmp(key, "workspaces") == 0) {
        int64_t c = 0;
        for (const WorkSlot& w : ix->slots) c += w.used ? 1 : 0;
        *out = c;
    }
    else return fail(CODD_KNN_EINVAL, "unknown stat: %s", key);
    return CODD_KNN_OK;
}

}  // extern "C"
