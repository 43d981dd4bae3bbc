// ingest_kernels.h — an implementation part of codd_knn.hip, included there exactly once; not a stand-alone interface.
// Device side, ingest: what turns caller vectors into stored rows and their bf16 shadow, and what reads stored rows back
// (normalise or store raw, query preparation of a filter pass, the norm check and the fp32 read-back of codd_knn_load_rows
// and the index build).
#pragma once

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

}  // namespace
