// exact_score.h — the canonical exact score and the block top-k merge, written once.
//
// score(q, row) = chunk j of the row belongs to lane j % 64; one fmaf chain per lane over its chunks in increasing j (elements in
// order inside a chunk); the 32 .. 1 butterfly over the lanes; + 0.0f.  Every kernel that scores a stored row calls the functions of
// this file, so every search path returns the same bits by construction:
//   narrow rows (NITER = 1 .. 4 chunks per lane): load_query_frags -> fetch4 -> score4 (fetch4_widened -> score4_one: the whole-store scan)
//   wide rows   (NITER = kWideRows)             : wide_stage_query -> wide_scores
//   per-wave lists -> one list per workgroup    : store_list, merge_lists, write_keys / write_ranks
//
// Scalars of the load and score functions are passed by reference on purpose: by value, hipcc's schedule of the inlined body comes out
// differently (finalize_kernel<0, 1, 1> 64 -> 68 VGPRs and 8 -> 7 waves per SIMD, scan_topk_kernel<0, 4, 2, 1> 124 -> 178 and 4 -> 2).
// tests/test_delete_kernel_resources.py (BEFORE_OCC) and tests/test_scoped_kernel_resources.py (PARENT_OCC) hold the outcome: change
// a signature here only with both passing.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "geometry.h"
#include "row_traits.h"
#include "wave_topk.h"

namespace codd {

// The metric of an exact-score function or body, a compile-time switch that defaults to the code as it always was:
//   kMetricDot  the canonical dot product — cosine on normalised operands, ip (CODD_KNN_METRIC_IP) on raw ones
//   kMetricL2   (== CODD_KNN_METRIC_L2) the squared distance by the direct difference: the chain step is t = q_e - c_e (one fp32
//               subtraction), a = fmaf(t, t, a); the butterfly sum is the distance and the score is 0.0f - distance, so that
//               larger is still better, an exact match scores +0, and the integer merges need no change
constexpr int kMetricDot = 0;
constexpr int kMetricL2 = 2;

// the tail of the expression for four rows at once: a[r] = this lane's chain of row r.  packed4: the 16 lanes of group r hold the
// score of row r; packed_score(y, r) hands it to every lane; reduce4 = both, sc[r] = the score of row r in every lane
template <int METRIC = kMetricDot>
__device__ __forceinline__ float packed4(const float (&a)[4], const int& lane) {
    if constexpr (METRIC == kMetricL2) return 0.0f - butterfly_sum4(a[0], a[1], a[2], a[3], lane);
    else return butterfly_sum4(a[0], a[1], a[2], a[3], lane);
}
__device__ __forceinline__ float packed_score(float y, const int& r) { return __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(y), 16 * r)); }
template <int METRIC = kMetricDot>
__device__ __forceinline__ void reduce4(const float (&a)[4], const int& lane, float (&sc)[4]) {
    const float y = packed4<METRIC>(a, lane);
#pragma unroll
    for (int r = 0; r < 4; ++r) sc[r] = packed_score(y, r);
}

// ---- narrow rows: the query's chunks and the rows' chunks both live in registers ----
// qf[it][e] = element e of chunk lane + 64 it of the query row q (zeros past the row, and everywhere for an absent query: q == nullptr)
template <int NITER, int E>
__device__ __forceinline__ void load_query_frags(const float* __restrict__ q, const int& nchunks, const int& lane, float (&qf)[NITER][E]) {
#pragma unroll
    for (int it = 0; it < NITER; ++it) {
        const int j = lane + kWave * it;
#pragma unroll
        for (int e = 0; e < E; ++e) qf[it][e] = (q && j < nchunks) ? q[(int64_t)j * E + e] : 0.0f;
    }
}

// c[r][it] = the raw 16-byte chunk lane + 64 it of row r (p[r]: the row's chunk `lane`), zero past the row: 4 NITER loads in flight
template <int NITER>
__device__ __forceinline__ void fetch4(const uint4* const (&p)[4], const int& nchunks, const int& lane, uint4 (&c)[4][NITER]) {
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int it = 0; it < NITER; ++it) {
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (lane + kWave * it < nchunks) v = p[r][kWave * it];
            c[r][it] = v;
        }
}

// sc[b][r] = the score of row r against query b < nq (0 for b >= nq), in every lane.  Chunk-major: a chunk is widened when its
// step comes (a widened bf16 / fp16 chunk is twice the registers) and serves every query.
template <int DT, int NB, int NITER, int METRIC = kMetricDot>
__device__ __forceinline__ void score4(const uint4 (&c)[4][NITER], const float (&qf)[NB][NITER][RowTraits<DT>::E], const int& nq, const int& lane, float (&sc)[NB][4]) {
    typedef RowTraits<DT> RT;
    constexpr int E = RT::E;
    float a[NB][4];
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int r = 0; r < 4; ++r) a[b][r] = 0.0f;
#pragma unroll
    for (int it = 0; it < NITER; ++it)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float w[E];
            RT::widen(c[r][it], w);
#pragma unroll
            for (int b = 0; b < NB; ++b)
                if (b < nq) {
#pragma unroll
                    for (int e = 0; e < E; ++e) {
                        if constexpr (METRIC == kMetricL2) {
                            const float t = qf[b][it][e] - w[e];
                            a[b][r] = __builtin_fmaf(t, t, a[b][r]);
                        } else {
                            a[b][r] = __builtin_fmaf(qf[b][it][e], w[e], a[b][r]);
                        }
                    }
                }
        }
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        if (b < nq) {
            reduce4<METRIC>(a[b], lane, sc[b]);
        } else {
#pragma unroll
            for (int r = 0; r < 4; ++r) sc[b][r] = 0.0f;
        }
    }
}

// scan_topk_body's order (widened at load, one query at a time, scores left packed): with score4, scan_topk_kernel<0, 4, 2, 1> 124 -> 178 VGPRs, 4 -> 2 waves
template <int DT, int NITER>
__device__ __forceinline__ void fetch4_widened(const uint4* const (&p)[4], const int& nchunks, const int& lane, float (&w)[4][NITER][RowTraits<DT>::E]) {
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int it = 0; it < NITER; ++it) {
            uint4 c = make_uint4(0u, 0u, 0u, 0u);
            if (lane + kWave * it < nchunks) c = p[r][kWave * it];
            RowTraits<DT>::widen(c, w[r][it]);
        }
}
template <int NITER, int E, int METRIC = kMetricDot>
__device__ __forceinline__ float score4_one(const float (&w)[4][NITER][E], const float (&qf)[NITER][E], const int& lane) {
    float a[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int it = 0; it < NITER; ++it)
#pragma unroll
            for (int e = 0; e < E; ++e) {
                if constexpr (METRIC == kMetricL2) {
                    const float t = qf[it][e] - w[r][it][e];
                    a[r] = __builtin_fmaf(t, t, a[r]);
                } else {
                    a[r] = __builtin_fmaf(qf[it][e], w[r][it][e], a[r]);
                }
            }
    return packed4<METRIC>(a, lane);
}

// ---- wide rows: more than 4 chunks per lane (f32 rows above 1,024 elements, 2-byte rows above 2,048) ----
// NITER = kWideRows selects the wide form of an exact-score body.  The full-width query no longer fits the registers (8 queries x 16
// chunks x 4 f32 = 512 VGPRs), so it is staged ONCE per workgroup in LDS, fp32 and chunk-major: qs[j * E + e] for chunk j, zeros past
// the row up to a whole segment.  The row is walked in segments of kSegIt chunks per lane (what NITER 4 holds in registers), the
// segment's row loads all in flight before its first fmaf, and each lane's accumulators are carried from one segment to the next:
// chunk j is still lane j % 64's and is visited in increasing j, so the per-lane chains, the butterfly behind them and the scores are
// exactly the narrow form's.  (kWideRows itself: geometry.h)
constexpr int kSegIt = 4;
constexpr int kWideMaxFloats = 4096;  // LDS floats of one staged query: dpad <= 4096 rounds up to at most 4,096 (f32: 1,024 chunks; 2-byte: 512)
__host__ __device__ constexpr int wide_nseg(int nchunks) { return (nchunks + kSegIt * kWave - 1) / (kSegIt * kWave); }
__host__ __device__ constexpr int wide_qfloats(int nchunks, int E) { return wide_nseg(nchunks) * kSegIt * kWave * E; }

// dst[0, nfloats) <- the query row src[0, dpad) followed by zeros (src == nullptr: all zeros); the workgroup's threads share it out
__device__ __forceinline__ void wide_stage_query(float* __restrict__ dst, const float* __restrict__ src, const int& dpad, const int& nfloats, const int& tid, const int& nthreads) {
    float4* d4 = reinterpret_cast<float4*>(dst);
    const float4* s4 = reinterpret_cast<const float4*>(src);
    const int have = src ? dpad >> 2 : 0;
    for (int i = tid; i < (nfloats >> 2); i += nthreads) d4[i] = i < have ? s4[i] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

// segment s of NR rows (p[r]: the row's chunk `lane`) against NQ staged queries (query b at qs + b * qstride): acc[b][r] continues
// each lane's canonical fmaf chain over chunks lane + 64 (kSegIt s + it), it = 0 .. kSegIt-1.  f32: the segment widened as it lands,
// one query's LDS values at a time; 2-byte rows: the 16-byte chunks stay raw until their step and chunk it's query values are read
// once for all rows.  Either way the same fmaf sequence per (query, row).
// USER only names the instantiation (the code is the same): a kernel added later asks for a copy of its own where sharing one would
// move hipcc's register allocation of the kernels that already use it (ivf_scan_sq beside scan_topk_wide_l2<DT, 1, SLOTS>: DESIGN.md §22).
template <int DT, int NQ, int NR, int METRIC = kMetricDot, int USER = 0>
__device__ __forceinline__ void wide_segment(const uint4* const (&p)[NR], const int& s, const int& nchunks, const int& lane, const float* qs, const int& qstride, float (&acc)[NQ][NR]) {
    typedef RowTraits<DT> RT;
    constexpr int E = RT::E;
    if constexpr (E == 4) {
        float w[NR][kSegIt][E];
#pragma unroll
        for (int r = 0; r < NR; ++r)
#pragma unroll
            for (int it = 0; it < kSegIt; ++it) {
                const int o = kWave * (kSegIt * s + it);
                uint4 c = make_uint4(0u, 0u, 0u, 0u);
                if (lane + o < nchunks) c = p[r][o];
                RT::widen(c, w[r][it]);
            }
#pragma unroll
        for (int b = 0; b < NQ; ++b) {
            float q[kSegIt][E];
#pragma unroll
            for (int it = 0; it < kSegIt; ++it) {
                const float4 v = *reinterpret_cast<const float4*>(qs + (int64_t)b * qstride + (int64_t)(lane + kWave * (kSegIt * s + it)) * E);
                q[it][0] = v.x; q[it][1] = v.y; q[it][2] = v.z; q[it][3] = v.w;
            }
#pragma unroll
            for (int r = 0; r < NR; ++r)
#pragma unroll
                for (int it = 0; it < kSegIt; ++it)
#pragma unroll
                    for (int e = 0; e < E; ++e) {
                        if constexpr (METRIC == kMetricL2) {
                            const float t = q[it][e] - w[r][it][e];
                            acc[b][r] = __builtin_fmaf(t, t, acc[b][r]);
                        } else {
                            acc[b][r] = __builtin_fmaf(q[it][e], w[r][it][e], acc[b][r]);
                        }
                    }
        }
        return;
    }
    uint4 c[NR][kSegIt];
#pragma unroll
    for (int r = 0; r < NR; ++r)
#pragma unroll
        for (int it = 0; it < kSegIt; ++it) {
            const int o = kWave * (kSegIt * s + it);
            c[r][it] = make_uint4(0u, 0u, 0u, 0u);
            if (lane + o < nchunks) c[r][it] = p[r][o];
        }
#pragma unroll
    for (int it = 0; it < kSegIt; ++it) {
        float q[NQ][E];
#pragma unroll
        for (int b = 0; b < NQ; ++b) {
            const float4* src = reinterpret_cast<const float4*>(qs + (int64_t)b * qstride + (int64_t)(lane + kWave * (kSegIt * s + it)) * E);
#pragma unroll
            for (int e4 = 0; e4 < E / 4; ++e4) {
                const float4 v = src[e4];
                q[b][4 * e4] = v.x; q[b][4 * e4 + 1] = v.y; q[b][4 * e4 + 2] = v.z; q[b][4 * e4 + 3] = v.w;
            }
        }
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            float w[E];
            RT::widen(c[r][it], w);
#pragma unroll
            for (int b = 0; b < NQ; ++b)
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    if constexpr (METRIC == kMetricL2) {
                        const float t = q[b][e] - w[e];
                        acc[b][r] = __builtin_fmaf(t, t, acc[b][r]);
                    } else {
                        acc[b][r] = __builtin_fmaf(q[b][e], w[e], acc[b][r]);
                    }
                }
        }
    }
}

// score4's wide twin for 4 G rows (G groups of four, every group's loads of a segment in flight together) against NQ staged queries:
// sc[b][4 g + r] = the score of row r of group g against query b < nq (0 for b >= nq), in every lane
template <int DT, int NQ, int G, int METRIC = kMetricDot, int USER = 0>
__device__ __forceinline__ void wide_scores(const uint4* const (&p)[4 * G], const int& nchunks, const int& lane, const float* qs, const int& qstride, const int& nq, float (&sc)[NQ][4 * G]) {
    float acc[NQ][4 * G];
#pragma unroll
    for (int b = 0; b < NQ; ++b)
#pragma unroll
        for (int r = 0; r < 4 * G; ++r) acc[b][r] = 0.0f;
    const int nseg = wide_nseg(nchunks);
    for (int s = 0; s < nseg; ++s) wide_segment<DT, NQ, 4 * G, METRIC, USER>(p, s, nchunks, lane, qs, qstride, acc);
#pragma unroll
    for (int b = 0; b < NQ; ++b)
#pragma unroll
        for (int g = 0; g < G; ++g) {
            float sg[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            if (b < nq) {
                const float a[4] = {acc[b][4 * g], acc[b][4 * g + 1], acc[b][4 * g + 2], acc[b][4 * g + 3]};
                reduce4<METRIC>(a, lane, sg);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) sc[b][4 * g + r] = sg[r];
        }
}

// ---- block merge: the waves' top-k lists meet in LDS, list i of wave w at lds[((w * nlists + i) * SLOTS + slot) * 64 + lane] ----
template <int SLOTS>
__device__ __forceinline__ void store_list(u64* __restrict__ lds, int wave, int nlists, int i, int lane, const WaveTopK<SLOTS>& L) {
#pragma unroll
    for (int s = 0; s < SLOTS; ++s) lds[((wave * nlists + i) * SLOTS + s) * kWave + lane] = L.v[s];
}
// folds list i of waves [w0, w1) into M (ranks >= k of a stored list are stale: dropped).  M = the wave's own list and w0 = 1: wave 0
// collects the workgroup's one list; M fresh and w0 = 0: wave i collects query i's list.  After a barrier behind store_list.
template <int SLOTS>
__device__ __forceinline__ void merge_lists(WaveTopK<SLOTS>& M, const u64* __restrict__ lds, int w0, int w1, int nlists, int i, int k, int lane) {
    for (int wv = w0; wv < w1; ++wv)
#pragma unroll
        for (int s = 0; s < SLOTS; ++s) {
            u64 cand = lds[((wv * nlists + i) * SLOTS + s) * kWave + lane];
            if (s * kWave + lane >= k) cand = 0ull;
            M.offer_lanes(cand, k, lane);
        }
}
// ranks < k of a list as packed keys
template <int SLOTS>
__device__ __forceinline__ void write_keys(const WaveTopK<SLOTS>& M, int k, int lane, u64* __restrict__ keys) {
#pragma unroll
    for (int s = 0; s < SLOTS; ++s) {
        const int rank = s * kWave + lane;
        if (rank < k) keys[rank] = M.v[s];
    }
}
// ... to any of: packed keys, (distance, row); distance = 1 - score, under kMetricL2 0 - score; an empty rank reads (inf, -1)
template <int SLOTS, int METRIC = kMetricDot>
__device__ __forceinline__ void write_ranks(const WaveTopK<SLOTS>& M, int k, int lane, u64* __restrict__ keys, float* __restrict__ dist, int64_t* __restrict__ rows) {
#pragma unroll
    for (int s = 0; s < SLOTS; ++s) {
        const int rank = s * kWave + lane;
        if (rank < k) {
            const u64 key = M.v[s];
            if (keys) keys[rank] = key;
            if (dist) dist[rank] = key ? (METRIC == kMetricL2 ? 0.0f : 1.0f) - key_score(key) : INFINITY;
            if (rows) rows[rank] = key ? (int64_t)key_row(key) : (int64_t)-1;
        }
    }
}

}  // namespace codd
