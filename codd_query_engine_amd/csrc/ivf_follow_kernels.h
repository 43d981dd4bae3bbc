// ivf_follow_kernels.h — an implementation part of codd_knn.hip, included there exactly once; not a stand-alone interface.
// Device side of an IVF layout that follows writes (host bookkeeping: ivf_follow.h):
//   pend_set_kernel           sets the bits of the slots a write made pending (the slots are the tail of the device list)
//   pend_or_kernel            deny | pending: the bitmap the list scans of a search with rows pending run under
//   ivf_delta_kernel, _sq     the delta scan (_sq: an l2 index, named like ivf_scan_sq): every pending slot scored from the MAIN row store with the canonical exact score
//                             (list_scan_body's gathering form under the call's deny bits), one partial list per (query, part)
//   widen_listed_rows_kernel  the stored rows of listed slots as fp32 queries (the fold assigns a row by searching the coarse index)
//   list_of_build_kernel      list_of[slot] from ivf_ids / ivf_offsets (first fold after an install)
//   list_assign_kernel        list_of[slot] = the coarse index's top-1 for the chunk's pending slots
//   ivf_list_count_kernel, ivf_list_offsets_kernel, ivf_list_scatter_kernel
//                             rows per list, their 64-bit exclusive prefix sums (up to 2^20 lists), slots to list positions; the
//                             order inside a list is whatever the atomics give (keys carry the row: a top-k does not depend on it)
#pragma once

namespace {

__global__ __launch_bounds__(256) void pend_set_kernel(const uint32_t* __restrict__ slots, int64_t n, uint32_t* __restrict__ bits) {
    const int64_t i = (int64_t)blockIdx.x * 256 + (int64_t)threadIdx.x;
    if (i < n) atomicOr(&bits[slots[i] >> 5], 1u << (slots[i] & 31u));
}

// deny: the call's own bitmap (tombstones, or ~allow | dead), null = none
__global__ __launch_bounds__(256) void pend_or_kernel(const uint32_t* __restrict__ deny, const uint32_t* __restrict__ pend, int64_t nwords,
                                                      uint32_t* __restrict__ out) {
    const int64_t w = (int64_t)blockIdx.x * 256 + (int64_t)threadIdx.x;
    if (w < nwords) out[w] = (deny ? deny[w] : 0u) | pend[w];
}

// grid (ceil(B / NB), split): workgroup (g, part) serves queries g * NB .. g * NB + NB-1 over part `part` of list[0, m), as
// mask_scan_body does, but under `deny` (a pending row may be deleted, or lie outside the call's mask) and with the caller's stride
// between the queries' partial lists: [query][stride_q], part `part` at part * k
template <int DT, int NITER, int SLOTS, int METRIC>
__device__ __forceinline__ void delta_scan_body(const void* __restrict__ rows_, const uint32_t* __restrict__ list, int64_t m, int B, int split,
                                                int dpad, const float* __restrict__ qn, int k, uint32_t row_base, const uint32_t* __restrict__ deny,
                                                u64* __restrict__ partial, int64_t stride_q) {
    constexpr int NB = scope_nb(DT, NITER);
    const int q0 = (int)blockIdx.x * NB, part = (int)blockIdx.y;
    const int nq = B - q0 < NB ? B - q0 : NB;
    const float* q[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) q[b] = b < nq ? qn + (int64_t)(q0 + b) * dpad : nullptr;
    const int64_t per = scope_part_rows(m, split);
    const int64_t begin = part * per < m ? part * per : m;
    const int64_t end = begin + per < m ? begin + per : m;
    list_scan_body<DT, NB, NITER, SLOTS, true, METRIC>(rows_, list, begin, end, dpad, q, nq, k, row_base, deny,
                                                       [&](int b) { return partial + (int64_t)(q0 + b) * stride_q + (int64_t)part * k; });
}
template <int DT, int NITER, int SLOTS>
__global__ __launch_bounds__(256) void ivf_delta_kernel(const void* __restrict__ rows_, const uint32_t* __restrict__ list, int64_t m, int B, int split,
                                                        int dpad, const float* __restrict__ qn, int k, uint32_t row_base,
                                                        const uint32_t* __restrict__ deny, u64* __restrict__ partial, int64_t stride_q) {
    delta_scan_body<DT, NITER, SLOTS, kMetricDot>(rows_, list, m, B, split, dpad, qn, k, row_base, deny, partial, stride_q);
}
template <int DT, int NITER, int SLOTS>
__global__ __launch_bounds__(256) void ivf_delta_sq(const void* __restrict__ rows_, const uint32_t* __restrict__ list, int64_t m, int B, int split,
                                                    int dpad, const float* __restrict__ qn, int k, uint32_t row_base,
                                                    const uint32_t* __restrict__ deny, u64* __restrict__ partial, int64_t stride_q) {
    delta_scan_body<DT, NITER, SLOTS, kMetricL2>(rows_, list, m, B, split, dpad, qn, k, row_base, deny, partial, stride_q);
}

// widen_rows_kernel by slot: out[r] = the stored row of slots[r], fp32 [n][dim], one wave per row
template <int DT>
__global__ __launch_bounds__(256) void widen_listed_rows_kernel(const void* __restrict__ rows_, const uint32_t* __restrict__ slots, int64_t n, int dim,
                                                                int dpad, float* __restrict__ out) {
    typedef RowTraits<DT> RT;
    constexpr int E = RT::E;
    const int lane = lane_id();
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= n) return;
    const int nchunks = dpad / E;
    const uint4* p = reinterpret_cast<const uint4*>(rows_) + (int64_t)slots[r] * (int64_t)nchunks;
    for (int j = lane; j < nchunks; j += kWave) {
        float w[E];
        RT::widen(p[j], w);
#pragma unroll
        for (int e = 0; e < E; ++e)
            if (j * E + e < dim) out[r * (int64_t)dim + j * E + e] = w[e];
    }
}

// position i of the layout holds row ids[i] of the list l with offsets[l] <= i < offsets[l + 1]: the last l whose start is <= i
__global__ __launch_bounds__(256) void list_of_build_kernel(const uint32_t* __restrict__ ids, const int64_t* __restrict__ offsets, int nlist, int64_t n,
                                                            uint32_t* __restrict__ list_of) {
    const int64_t i = (int64_t)blockIdx.x * 256 + (int64_t)threadIdx.x;
    if (i >= n) return;
    int lo = 0, hi = nlist;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (offsets[mid] <= i) lo = mid; else hi = mid;
    }
    list_of[ids[i]] = (uint32_t)lo;
}

// keys[i]: the coarse index's best key for the stored row of slots[i] (k = 1).  An empty key (no centroid scored: cannot happen
// with nlist >= 1) and a list out of range fall to list 0
__global__ __launch_bounds__(256) void list_assign_kernel(const u64* __restrict__ keys, const uint32_t* __restrict__ slots, int64_t n, int nlist,
                                                          uint32_t* __restrict__ list_of) {
    const int64_t i = (int64_t)blockIdx.x * 256 + (int64_t)threadIdx.x;
    if (i >= n) return;
    const u64 key = keys[i];
    uint32_t l = key != 0ull ? key_row(key) : 0u;
    if (l >= (uint32_t)nlist) l = 0u;
    list_of[slots[i]] = l;
}

__global__ __launch_bounds__(256) void ivf_list_count_kernel(const uint32_t* __restrict__ list_of, int64_t n, int nlist, unsigned* __restrict__ cnt) {
    const int64_t r = (int64_t)blockIdx.x * 256 + (int64_t)threadIdx.x;
    if (r >= n) return;
    uint32_t l = list_of[r];
    if (l >= (uint32_t)nlist) l = 0u;   // (cannot happen: every slot below the count was assigned)
    atomicAdd(&cnt[l], 1u);
}
// one workgroup: offsets[l] = exclusive prefix sum of cnt[] in 64 bits, the total at offsets[nlist]; cnt[] is cleared on the way (the
// scatter's fill counters).  1,024 threads x up to 1,024 lists each: 2^20 lists
__global__ __launch_bounds__(1024) void ivf_list_offsets_kernel(unsigned* __restrict__ cnt, int nlist, int64_t* __restrict__ offsets) {
    __shared__ unsigned long long s_p[1024];
    const int tid = (int)threadIdx.x;
    const int per = (nlist + 1023) / 1024;
    unsigned long long sp = 0;
    for (int j = 0; j < per; ++j) {
        const int l = tid * per + j;
        sp += l < nlist ? cnt[l] : 0u;
    }
    s_p[tid] = sp;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {   // Hillis-Steele inclusive scan
        const unsigned long long a = tid >= off ? s_p[tid - off] : 0ull;
        __syncthreads();
        s_p[tid] += a;
        __syncthreads();
    }
    unsigned long long bp = s_p[tid] - sp;
    for (int j = 0; j < per; ++j) {
        const int l = tid * per + j;
        if (l < nlist) {
            const unsigned c = cnt[l];
            offsets[l] = (int64_t)bp;
            bp += c;
            cnt[l] = 0u;
        }
    }
    if (tid == 1023) offsets[nlist] = (int64_t)s_p[1023];
}
__global__ __launch_bounds__(256) void ivf_list_scatter_kernel(const uint32_t* __restrict__ list_of, int64_t n, int nlist, const int64_t* __restrict__ offsets,
                                                               unsigned* __restrict__ fill, int64_t* __restrict__ perm) {
    const int64_t r = (int64_t)blockIdx.x * 256 + (int64_t)threadIdx.x;
    if (r >= n) return;
    uint32_t l = list_of[r];
    if (l >= (uint32_t)nlist) l = 0u;
    const int64_t at = offsets[l] + (int64_t)atomicAdd(&fill[l], 1u);
    if (at < n) perm[at] = r;   // (at < n always: the counts came from the same labels)
}

}  // namespace
