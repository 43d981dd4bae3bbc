// shadow8_kernels.h — an implementation part of codd_knn.hip, included there exactly once; not a stand-alone interface.
// Device side, the int8 shadow: building it from the stored rows, the query preparation and error bounds of the int8 filter
// leg (cosine and raw), and small_batch_kernel, which answers few queries from the shadow in one launch.
#pragma once

namespace {

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

}  // namespace
