// scan_kernels.h — an implementation part of codd_knn.hip, included there exactly once; not a stand-alone interface.
// Device side, the exact scan of the whole row store: scan_topk_body and its kernels (dot product and squared L2, narrow and
// wide rows, the listed fallback), finalize_fb_kernel, and the integer top-k merge of packed keys.
#pragma once

namespace {

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

}  // namespace
