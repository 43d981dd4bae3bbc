// list_scan_kernels.h — an implementation part of codd_knn.hip, included there exactly once; not a stand-alone interface.
// Device side, everything that scans a row list or builds one: the IVF layout helpers, pair grouping and scans,
// list_scan_body, the scope kernels, tombstones and compaction, and the mask kernels.
#pragma once

namespace {

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
// (kIvfNB, the queries per work item: geometry.h)
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

// (queries per work item: scope_nb(), geometry.h)
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
