// filter_gemm.h — the large-batch leg of the search: a bf16 MFMA GEMM that never materialises the
// B x N score matrix.  It FILTERS: for every query it emits the rows whose approximate score
// clears a per-query threshold that provably keeps every true top-k row; the
// survivors are re-scored exactly (canonical fp32) by finalize_kernel.
//
// Data layout (both operands are stored in MFMA-fragment order, so every wave-level load is one
// contiguous 1 KiB piece and LDS reads are conflict-free without a swizzle); shown for the shipped
// v_mfma_f32_16x16x32_bf16 shape (shadow_piece_index / qfrag_piece_index are the definition; the
// 32x32x16 order is kept behind -DCODD_MFMA16=0):
//
//   shadow (bf16 copy of the corpus, written at ingest), in 16-byte pieces of 8 elements:
//       piece[((block*nsteps + s)*4 + (rs*2 + ks))*64 + (kq*16 + r)]
//                                   = C[row = 32*block + 16*rs + r][k = 64s + 32ks + 8kq + 0..7]
//   qfrag (bf16 query block, written by qfrag_kernel per search):
//       piece[(s*32 + qb*2 + ks)*64 + (kq*16 + c)] = Q[query = 16*qb + c][k = 64s + 32ks + 8kq + 0..7]
//
// One MFMA consumes, per lane (r|c = lane&15, kq = lane>>4), exactly one such piece of each operand;
// the k order inside an instruction is permuted identically on both sides, which a dot product does
// not notice.
//
// Workgroup = 8 waves = one tile of 256 corpus rows x 256 queries, K-step 64:
//   * wave w owns corpus rows [32w, 32w+32) of the tile and ALL 256 queries: 2 x 16 accumulator blocks
//     of 16x16 (128 VGPRs).  Its corpus fragments go HBM -> registers directly (each corpus byte
//     enters the CU once, is used by one wave: no LDS round trip), three K-steps deep in a
//     register ring so ~12 KiB per wave stays in flight;
//   * the query K-slice (32 KiB, L2-resident, shared by the 8 waves) is double-buffered in LDS in
//     stages of two slices, staged through registers (issue early, write late) so that every load in
//     the kernel is an ordinary counted load and __syncthreads() stays a bare s_barrier;
//   * one barrier per stage; 64 MFMAs + 32 ds_read_b128 per wave per K-step.
#pragma once
#include <type_traits>

#include "exact_score.h"
#include "geometry.h"
#include "row_traits.h"
#include "wave_topk.h"

namespace codd {

// (CODD_SHADOW_F16, CODD_MFMA16, kTileRows, kTileQ: geometry.h)
#if CODD_SHADOW_F16
typedef __attribute__((ext_vector_type(8))) _Float16 bf16x8;  // "shadow element x8" (name kept for the bf16 default)
#else
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
#endif
typedef __attribute__((ext_vector_type(16))) float f32x16;

constexpr int kStagePieces = 2048;  // 16-byte pieces of one query K-slice (256 q x 64 k bf16 = 32 KiB)
#ifndef CODD_RB
#define CODD_RB 1            // 32-row corpus blocks per wave: 1 -> 8 waves x 256 regs, 2 -> 4 waves x 512 regs
#endif
#ifndef CODD_QSPLIT
#define CODD_QSPLIT 1        // 2: two waves share each row group and take half of the query blocks each
#endif
constexpr int kRB = CODD_RB;
constexpr int kQSplit = CODD_QSPLIT;
constexpr int kRowGroups = 8 / kRB;                   // row groups of a 256-row tile
constexpr int kFilterWaves = kRowGroups * kQSplit;
constexpr int kFilterThreads = 64 * kFilterWaves;
constexpr int kQP = kStagePieces / kFilterThreads;  // query-slice pieces each thread stages per K-step
// MFMA block geometry.  32x32x16: a wave's 32 rows are ONE row block, a 64-wide K-step is 4 sub-steps, a
// 32-query block per accumulator (16 regs).  16x16x32: TWO row blocks of 16, 2 sub-steps, 16-query blocks
// (4 regs).  Either way a wave-level operand piece is 64 lanes x 16 B = 1 KiB and an accumulator set is 128 regs.
constexpr int kMB = CODD_MFMA16 ? 16 : 32;         // rows (and queries) per MFMA block
constexpr int kAccRegs = CODD_MFMA16 ? 4 : 16;
constexpr int kKS = CODD_MFMA16 ? 2 : 4;           // MFMA K sub-steps per 64-wide K-step
constexpr int kRS = (32 / kMB) * kRB;              // row blocks per wave
constexpr int kQBper32 = 32 / kMB;                 // query blocks per 32 queries
static_assert(kFilterWaves <= 8, "at most 8 waves per workgroup");
#if CODD_MFMA16
typedef __attribute__((ext_vector_type(4))) float acc_t;
#else
typedef __attribute__((ext_vector_type(16))) float acc_t;
#endif
// which of the 4 corpus pieces of a (32-row block, K-step) feeds row block rs at sub-step ks
__host__ __device__ constexpr int a_piece(int rs_in_block, int ks) { return CODD_MFMA16 ? rs_in_block * 2 + ks : ks; }
// which piece of a query K-slice feeds query block qb at sub-step ks
__host__ __device__ constexpr int b_piece(int qb, int ks) { return CODD_MFMA16 ? qb * 2 + ks : qb * 4 + ks; }
// accumulator register r of a lane -> row offset inside the MFMA row block
__device__ __forceinline__ int acc_row(int r, int lane) {
    return CODD_MFMA16 ? 4 * (lane >> 4) + r : 4 * (lane >> 5) + (r & 3) + 8 * (r >> 2);
}
// build-time experiment switches (defaults = the shipped configuration)
#ifndef CODD_EXPERIMENTS
#define CODD_EXPERIMENTS 0
#endif
#if !CODD_EXPERIMENTS && (defined(CODD_NO_EPILOGUE) || defined(CODD_EXP_SAME_TILE) || defined(CODD_EXP_NO_QSTAGE) || defined(CODD_EXP_NB) || \
                          defined(CODD_EXP_NO_HITS) || defined(CODD_EXP_NO_LDSREAD) || defined(CODD_EXP_NO_FLUSH) || defined(CODD_EXP_NO_BARRIER))
#error "the CODD_EXP_* / CODD_NO_EPILOGUE switches return wrong results or race: they exist only in -DCODD_EXPERIMENTS=1 builds (build_variant)"
#endif
#ifndef CODD_QS
#define CODD_QS 2            // 64-wide query K-slices per LDS stage = K-steps per workgroup barrier
#endif
#ifndef CODD_PIN_SCHEDULE
#define CODD_PIN_SCHEDULE 1  // sched_group_barrier shape of a K-step
#endif
#ifndef CODD_MFMA_PRIO
#define CODD_MFMA_PRIO 0     // s_setprio(1) around the MFMA cluster
#endif
#ifndef CODD_STATIC_PRIO
#define CODD_STATIC_PRIO 0   // waves 4..7 (the second wave of every SIMD) run at s_setprio 1 for the whole kernel
#endif
#ifndef CODD_NT_LOADS
#define CODD_NT_LOADS 1      // corpus fragments with the non-temporal cache policy (read-once stream)
#endif
#ifndef CODD_BLOCKED_TILES
#define CODD_BLOCKED_TILES 0 // 1: workgroup b walks a contiguous range of tiles instead of b, b+G, b+2G, ...
#endif
#ifndef CODD_NO_EPILOGUE
#define CODD_NO_EPILOGUE 0   // diagnostic only: skip the threshold test (results are wrong)
#endif
#ifndef CODD_EXP_SAME_TILE
#define CODD_EXP_SAME_TILE 0 // diagnostic only: every step re-reads tile 0 (L2-resident corpus)
#endif
#ifndef CODD_EXP_NO_QSTAGE
#define CODD_EXP_NO_QSTAGE 0 // diagnostic only: no query staging loads / LDS writes
#endif
#ifndef CODD_EXP_NB
#define CODD_EXP_NB 8        // diagnostic only: query blocks actually multiplied (8 = all)
#endif
#ifndef CODD_EXP_NO_HITS
#define CODD_EXP_NO_HITS 0   // diagnostic only: thresholds forced to +inf
#endif
#ifndef CODD_EXP_NO_LDSREAD
#define CODD_EXP_NO_LDSREAD 0 // diagnostic only: the query fragment is taken from a register, not from LDS
#endif
#ifndef CODD_EXP_NO_FLUSH
#define CODD_EXP_NO_FLUSH 0  // diagnostic only: the final hit list is dropped (results are wrong)
#endif
#ifndef CODD_EXP_NO_BARRIER
#define CODD_EXP_NO_BARRIER 0 // diagnostic only: no stage barriers (racy)
#endif
constexpr int kQS = CODD_QS;
constexpr int kLdsQBytes = 2 * kQS * kStagePieces * 16;
constexpr int kHitCap = kQS == 1 ? 4096 : 2048;  // per-workgroup LDS hit list (entries of 3 dwords)
#ifndef CODD_HITCNT_STRIDE
#define CODD_HITCNT_STRIDE 1  // dwords between two queries' global hit counters (32 = one 128-byte line each)
#endif
#ifndef CODD_FLUSH_AT
#define CODD_FLUSH_AT (kHitCap / 2)  // a workgroup empties its LDS hit list at the first tile end with more entries
#endif
constexpr int kHitCntStride = CODD_HITCNT_STRIDE;
#ifndef CODD_RING
#define CODD_RING 3
#endif
#ifndef CODD_STAGGER
#define CODD_STAGGER 0  // 1: waves 4..7 run their MFMA halves half a K-step behind waves 0..3 (one barrier per K-step)
#endif
#ifndef CODD_QDEPTH
#define CODD_QDEPTH 1   // 2: the query slice of step t+3 is requested during step t (one step more for the L2 round trip), 16 more VGPRs
#endif
constexpr int kQD = CODD_QDEPTH;
constexpr int kUnroll = CODD_RING * CODD_QDEPTH;  // steps per unrolled loop body: every register buffer index is static
constexpr int kRing = CODD_RING;        // corpus-fragment register ring (K-steps)
constexpr int kPrefetch = CODD_RING - 1;  // K-steps the corpus loads run ahead

enum { MODE_FILTER = 0, MODE_SAMPLE = 1, MODE_DUMP = 2 };
constexpr int kLdsWords = 576;  // dwords of per-workgroup bookkeeping behind the query slices (256 thresholds + counter, or 256 u64 keys)

// flags[] words shared with the host
enum { FLAG_WG_OVERFLOW = 0 /* statistics: a workgroup hit list filled up */, FLAG_NEED_FALLBACK = 1 /* any query queued */, FLAG_WORDS = 4 };

// 16-byte piece (8 consecutive elements, c8 = element/8) of `row` in the shadow / of query q in qfrag.
// 32x32x16: lane (h = lane>>5, r = lane&31) of sub-step kk holds k = 64s + 32h + 8kk + 0..7
// 16x16x32: lane (kq = lane>>4, r = lane&15) of sub-step ks holds k = 64s + 32ks + 8kq + 0..7
__host__ __device__ inline int64_t shadow_piece_index(int64_t row, int c8, int nsteps) {
    const int64_t block = row >> 5;
    const int s = c8 >> 3;
#if CODD_MFMA16
    const int rs = (int)(row >> 4) & 1, r = (int)(row & 15), ks = (c8 >> 2) & 1, kq = c8 & 3;
    return ((block * nsteps + s) * 4 + a_piece(rs, ks)) * 64 + (kq * 16 + r);
#else
    const int r = (int)(row & 31), h = (c8 >> 2) & 1, kk = c8 & 3;
    return ((block * nsteps + s) * 4 + kk) * 64 + (h * 32 + r);
#endif
}
__host__ __device__ inline int64_t qfrag_piece_index(int q, int c8) {
    const int s = c8 >> 3;
#if CODD_MFMA16
    const int qb = q >> 4, c = q & 15, ks = (c8 >> 2) & 1, kq = c8 & 3;
    return ((int64_t)s * 32 + b_piece(qb, ks)) * 64 + (kq * 16 + c);
#else
    const int nb = q >> 5, c = q & 31, h = (c8 >> 2) & 1, kk = c8 & 3;
    return (((int64_t)s * 8 + nb) * 4 + kk) * 64 + (h * 32 + c);
#endif
}

// two fp32 values -> two shadow elements (bf16, or fp16 under CODD_SHADOW_F16), round to nearest even
__device__ __forceinline__ uint32_t pack_bf16x2(float lo, float hi) {
#if CODD_SHADOW_F16
    typedef _Float16 h2 __attribute__((ext_vector_type(2)));
    const h2 v = {(_Float16)lo, (_Float16)hi};  // v_cvt_f16_f32, RNE; |x| <= 1 here, no overflow
    return __builtin_bit_cast(uint32_t, v);
#endif
    uint32_t a = __float_as_uint(lo), b = __float_as_uint(hi);
    a = ((a & 0x7fffffffu) > 0x7f800000u) ? ((a >> 16) | 0x0040u) : ((a + 0x7fffu + ((a >> 16) & 1u)) >> 16);
    b = ((b & 0x7fffffffu) > 0x7f800000u) ? ((b >> 16) | 0x0040u) : ((b + 0x7fffu + ((b >> 16) & 1u)) >> 16);
    return (a & 0xffffu) | (b << 16);
}

// qn: [B][dpad] fp32 normalised queries -> qfrag pieces (queries >= B are zero).  One thread per piece.
// Also zeroes the pass's control block (ctl_words dwords) so that no separate memset launch is needed.
__global__ __launch_bounds__(256) void qfrag_kernel(const float* __restrict__ qn, int B, int dpad, uint4* __restrict__ qfrag,
                                                    unsigned* __restrict__ ctl, int ctl_words) {
    const int npieces = kTileQ * (dpad >> 3);
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx < ctl_words) ctl[idx] = 0u;
    if (idx >= npieces) return;
    const int q = idx / (dpad >> 3), c8 = idx % (dpad >> 3);
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (q < B) {
        const float4* p = reinterpret_cast<const float4*>(qn + (int64_t)q * dpad + c8 * 8);
        const float4 a = p[0], b = p[1];
        v = make_uint4(pack_bf16x2(a.x, a.y), pack_bf16x2(a.z, a.w), pack_bf16x2(b.x, b.y), pack_bf16x2(b.z, b.w));
    }
    qfrag[qfrag_piece_index(q, c8)] = v;
}

// f(integral_constant<int, 0>{}) ... f(integral_constant<int, N-1>{}), in order
template <int N, int I = 0, typename F>
__device__ __forceinline__ void static_for(F f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        static_for<N, I + 1>(f);
    }
}

// append a workgroup's LDS hit list (entries: score bits, row, query) to the per-query global lists
// qs (optional, LDS): per-query factor still to be applied to the stored scores (filter_i8.h stores acc * rscale and leaves
// the query's scale to the flush)
__device__ __forceinline__ void flush_hits(const unsigned* lds_hits, unsigned m, int tid, u64* __restrict__ hits,
                                           unsigned* __restrict__ hit_cnt, int cap_q, const float* qs = nullptr) {
    for (unsigned e = tid; e < m; e += kFilterThreads) {
        const unsigned row = lds_hits[e * 3 + 1], q = lds_hits[e * 3 + 2];
        float v = __uint_as_float(lds_hits[e * 3 + 0]);
        if (qs) v *= qs[q];
        const unsigned slot = atomicAdd(&hit_cnt[q * kHitCntStride], 1u);
        if (slot < (unsigned)cap_q) hits[(int64_t)q * cap_q + slot] = make_key(v, row);
    }
}

// The same append for the list a workgroup is left with when it has run out of tiles (the common case: ~1000 hits,
// all 256 workgroups at once).  One device-scope atomic per hit made that moment ~0.12 ms of every launch, whatever
// the row count (profiles/r1/v5_hit_flush_ablation.txt); here the entries are first counted per query in LDS and every
// query reserves its whole range with ONE atomic.  cnt256 is a scratch of 256 words (the thresholds, dead by now).
#ifndef CODD_BALLOT_HITS
#define CODD_BALLOT_HITS 0   // 1: the epilogue reserves LDS hit slots per accumulator block (ballots) instead of per register; measured 2 % slower
#endif
#ifndef CODD_BINNED_INLOOP
#define CODD_BINNED_INLOOP 0  // 1: the flushes inside the loop reserve per-query ranges too (int8 kernel -1 %, bf16 kernel +10 % time: register allocation; off)
#endif
#ifndef CODD_BINNED_FLUSH
#define CODD_BINNED_FLUSH 1
#endif
__device__ __forceinline__ void flush_hits_binned(const unsigned* lds_hits, unsigned m, int tid, unsigned* cnt256,
                                                  u64* __restrict__ hits, unsigned* __restrict__ hit_cnt, int cap_q, const float* qs = nullptr) {
    constexpr int kPer = kHitCap / kFilterThreads;
    static_assert(kHitCap % kFilterThreads == 0, "hit list is a whole number of entries per thread");
    if (tid < 256) cnt256[tid] = 0u;
    __syncthreads();
    unsigned rank[kPer];
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
        const unsigned e = (unsigned)tid + (unsigned)i * kFilterThreads;
        rank[i] = e < m ? atomicAdd(&cnt256[lds_hits[e * 3 + 2]], 1u) : 0u;
    }
    __syncthreads();
    if (tid < 256) {
        const unsigned c = cnt256[tid];
        cnt256[tid] = c ? atomicAdd(&hit_cnt[tid * kHitCntStride], c) : 0u;  // a poisoned counter stays poisoned
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
        const unsigned e = (unsigned)tid + (unsigned)i * kFilterThreads;
        if (e < m) {
            const unsigned q = lds_hits[e * 3 + 2];
            const unsigned slot = cnt256[q] + rank[i];
            float v = __uint_as_float(lds_hits[e * 3 + 0]);
            if (qs) v *= qs[q];
            if (slot < (unsigned)cap_q) hits[(int64_t)q * cap_q + slot] = make_key(v, lds_hits[e * 3 + 1]);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// gemm_filter_kernel<MODE, NBQ>   (NBQ = 32-query blocks actually multiplied: 1, 2, 4 or 8; a small
//   batch pays only for its own MFMAs and LDS traffic and the kernel turns into a pure HBM stream)
//   MODE_FILTER: every (query, row) with approx score >= thr[query] is appended to hits[query][]
//   MODE_SAMPLE: per (tile, query) the best (approx score, row) key is written to bucket_key[query][tile]
//   MODE_DUMP  : all scores to dump[query][row] (diagnostics / layout tests, small n only)
// Run-tile u (0 <= u < ntiles_run) is corpus tile u*tile_stride; workgroup b takes u = b, b+G, ...
// ---------------------------------------------------------------------------------------------
// EL = 1: the operands are int8 with one fp32 scale per corpus row (rscale) and per query (qscale): 128 elements per
// K-step instead of 64, v_mfma_i32_16x16x64_i8 (twice the bf16 rate, half the bytes), exact integer accumulation; a
// score is acc * rscale[row] * qscale[query].  The piece / ring / LDS geometry is byte-identical to the bf16 mode.
// RES = 1 (only launched when the row has at most 4 K-steps, i.e. the whole query block fits the 4 LDS slices): the
// query block is loaded into LDS once per workgroup and never re-staged — no staging loads, LDS writes or stage barriers
// in the loop (re-staging costs 15-19 % of the kernel, profiles/r1/v5_hit_flush_ablation.txt).
// The kernel body lives in filter_gemm_body.inc and is included into both kernels below, so that each __global__ function holds
// the statements themselves (hipcc compiles a body reached through a forwarding call differently, and gemm_filter_kernel must stay
// the code it was: tests/test_spaces_kernel_resources.py).  The body sees MODE, NBQ, EL, RES, the kernel's parameters, and
//   SQD = 0: the code as it always was;
//   SQD = 1 (EL = 1, RES = 0): the squared-distance form of the int8 mode.  The value of a (query, row) is
//            v = fma(acc * rscale[row], 2 * qscale[query], -rnorm2[row]) - qn2[query] ~ -|q - c|^2 (rnorm2: the row's canonical sum of
//            squares, qn2: the query's); the test runs on the fma against thr + qn2, written !(w < t) so that a value that is not a
//            number is a hit, never a silent miss; a hit carries v.
template <int MODE, int NBQ, int EL = 0, int RES = 0>
__global__ __launch_bounds__(kFilterThreads, kFilterWaves == 8 ? 2 : 1) void gemm_filter_kernel(
    const uint4* __restrict__ shadow, const uint4* __restrict__ qfrag, int64_t n, int nsteps, int64_t ntiles_run,
    int64_t tile_stride, const float* __restrict__ thr, u64* __restrict__ bucket_key, u64* __restrict__ hits,
    unsigned* __restrict__ hit_cnt, int cap_q, unsigned* __restrict__ flags, float* __restrict__ dump,
    const float* __restrict__ rscale = nullptr, const float* __restrict__ qscale = nullptr) {
    constexpr int SQD = 0;
    constexpr const float* rnorm2 = nullptr;
    constexpr const float* qn2 = nullptr;
#include "filter_gemm_body.inc"
}

// The filter of an l2 index: the staged int8 GEMM with the squared-distance epilogue.  rnorm2[row] and qn2[query]
// are the canonical sums of squares of the stored row and of the cleaned query.
template <int MODE, int NBQ>
__global__ __launch_bounds__(kFilterThreads, kFilterWaves == 8 ? 2 : 1) void sqd_filter_kernel(
    const uint4* __restrict__ shadow, const uint4* __restrict__ qfrag, int64_t n, int nsteps, int64_t ntiles_run,
    int64_t tile_stride, const float* __restrict__ thr, u64* __restrict__ bucket_key, u64* __restrict__ hits,
    unsigned* __restrict__ hit_cnt, int cap_q, unsigned* __restrict__ flags, float* __restrict__ dump,
    const float* __restrict__ rscale, const float* __restrict__ qscale, const float* __restrict__ rnorm2,
    const float* __restrict__ qn2) {
    constexpr int SQD = 1, EL = 1, RES = 0;
#include "filter_gemm_body.inc"
}

constexpr int kSurvChunk = 2048;  // hits examined per round; their survivors always fit the LDS list
#ifndef CODD_FIN_WAVES
#define CODD_FIN_WAVES 8
#endif
constexpr int kFinWaves = CODD_FIN_WAVES;      // waves of a finalize workgroup (one query, or one share of its hits): the kernel is a chain of
constexpr int kFinThreads = kFinWaves * kWave; // round trips (hit list, k anchor rows, survivor rows), so a query gets as many waves as pay

// finalize_body: what one workgroup of kFinThreads threads does for ONE query (or one share of its candidates): `my[0, total)`
// are the query's candidate keys (approximate score, local row; 0 = empty slot), qn_q its normalised fp32 vector.
//   eps1 : the slack between an approximate and an exact score — the whole of it, or (bmeta != nullptr, the int8 filter) its
//          block-independent part A(q), with bq = B(q): eps(q, block) = A + B e_block, e_block = bmeta[row / 32].y
//   out_*_q / part_keys_q : where this query's k results go (any may be null)
//   dead : the tombstone bits (null: no row was ever deleted).  A dead hit is dropped BEFORE the k best approximate hits are
//          chosen — L' must be the smallest exact score of k LIVE rows, or rows between a dead anchor's score and the live
//          k-th best would be cut off — and it is never re-scored into the answer.
// Shared by finalize_kernel and by the last workgroup of small_batch_kernel (shadow8_kernels.h).
template <int DT, int NITER, int SLOTS, int METRIC = kMetricDot>
__device__ __forceinline__ void finalize_body(const void* __restrict__ rows_, int dpad, const float* __restrict__ qn_q, const u64* __restrict__ my,
                                              unsigned total, unsigned part, unsigned nparts, int k, float eps1, float bq,
                                              const float2* __restrict__ bmeta, uint32_t row_base, u64* __restrict__ out_keys_q,
                                              float* __restrict__ out_dist_q, int64_t* __restrict__ out_rows_q, u64* __restrict__ part_keys_q,
                                              unsigned long long* __restrict__ stats, const uint32_t* __restrict__ dead,
                                              float* lo_out = nullptr) {
    typedef RowTraits<DT> RT;
    constexpr int E = RT::E;
    __shared__ u64 lds_list[kFinWaves * SLOTS * kWave];
    __shared__ unsigned lds_surv[kSurvChunk];
    __shared__ unsigned lds_n;
    __shared__ float lds_lo;
    __shared__ float lds_anchor[kFinWaves];

    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;

    // the query's fragments for the exact re-scoring: requested first, so the round trip overlaps step 1
    const int nchunks = dpad / E;
    float qf[1][NITER > 0 ? NITER : 1][E];
    float* lds_q = nullptr;
    if constexpr (NITER == kWideRows) {  // wide rows: the query in LDS (the first barrier below publishes it)
        __shared__ __attribute__((aligned(16))) float lds_qw[kWideMaxFloats];
        lds_q = lds_qw;
        wide_stage_query(lds_q, qn_q, dpad, wide_qfloats(nchunks, E), tid, kFinThreads);
    } else {
        load_query_frags(qn_q, nchunks, lane, qf[0]);
    }

    // 1. k-th largest approximate key
    WaveTopK<SLOTS> L;
    L.init();
    for (unsigned i0 = wave * kWave; i0 < total; i0 += kFinThreads) {
        const unsigned i = i0 + lane;
        u64 key = i < total ? my[i] : 0ull;
        if (dead && key && row_dead(dead, key_row(key))) key = 0ull;
        L.offer_lanes(key, k, lane);
    }
    store_list(lds_list, wave, 1, 0, lane, L);
    __syncthreads();
    if (wave == 0) {
        merge_lists(L, lds_list, 1, kFinWaves, 1, 0, k, lane);
        // rows of the k best approximate hits (or none when the list is not full: then every hit survives)
        if (lane == 0) lds_n = L.thr ? (unsigned)k : 0u;
        if (L.thr) {
#pragma unroll
            for (int s = 0; s < SLOTS; ++s)
                if (s * kWave + lane < k) lds_surv[s * kWave + lane] = key_row(L.v[s]);
        }
    }
    __syncthreads();
    const uint4* base = reinterpret_cast<const uint4*>(rows_);
    // canonical exact scores of up to four rows per wave step (the expression of the exact scan)
    auto rescore4 = [&](const unsigned (&rowid)[4], float (&sc)[1][4]) __attribute__((always_inline)) {
        const uint4* p[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) p[r] = base + (int64_t)rowid[r] * nchunks + lane;
        if constexpr (NITER == kWideRows) {
            wide_scores<DT, 1, 1, METRIC>(p, nchunks, lane, lds_q, 0, 1, sc);
        } else {
            uint4 c[4][NITER];
            fetch4(p, nchunks, lane, c);
            score4<DT, 1, NITER, METRIC>(c, qf, 1, lane, sc);
        }
    };
    // 1b. anchor: those k rows are k distinct rows with EXACT scores >= L' := their smallest exact score, so the true
    // k-th best score is >= L' and every true top-k row has an approximate score >= L' - eps (one eps, not two: the
    // bound compares an approximation with an exact score, not two approximations)
    {
        const unsigned nk = lds_n;
        float worst = INFINITY;
        for (unsigned j = wave * 4; j < nk; j += 4 * kFinWaves) {
            unsigned rowid[4];
            float sc[1][4];
#pragma unroll
            for (int r = 0; r < 4; ++r) rowid[r] = lds_surv[j + r < nk ? j + r : nk - 1];
            rescore4(rowid, sc);
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (j + r < nk) worst = fminf(worst, sc[0][r]);
        }
        if (lane == 0) lds_anchor[wave] = worst;
        __syncthreads();
        if (tid == 0) {
            float l4 = lds_anchor[0];
#pragma unroll
            for (int wv = 1; wv < kFinWaves; ++wv) l4 = fminf(l4, lds_anchor[wv]);
            lds_lo = nk ? l4 - eps1 : -INFINITY;
            if (lo_out) *lo_out = lds_lo;
        }
        __syncthreads();
    }
    const float lo = lds_lo;

    WaveTopK<SLOTS> X;
    X.init();
    unsigned survivors = 0;

    // 2 + 3. round by round: survivors of the next kSurvChunk hits (approx >= a_k - 2 eps: no other row can reach
    // the exact top-k) are compacted into LDS and re-scored exactly, four rows per wave step, with the same
    // canonical expression as the scan.  No cap on the number of survivors: a dense cluster costs time, not exactness.
    const unsigned my_lo = (unsigned)((u64)total * part / nparts), my_hi = (unsigned)((u64)total * (part + 1) / nparts);  // this workgroup's share
    for (unsigned b0 = my_lo; b0 < my_hi; b0 += kSurvChunk) {
        if (tid == 0) lds_n = 0u;
        __syncthreads();
        const unsigned b1 = b0 + kSurvChunk < my_hi ? b0 + kSurvChunk : my_hi;
        for (unsigned i = b0 + tid; i < b1; i += kFinThreads) {
            const u64 key = my[i];
            const float slack_b = bmeta ? bq * bmeta[key_row(key) >> 5].y : 0.0f;
            if (key_score(key) + slack_b >= lo && !(dead && row_dead(dead, key_row(key)))) lds_surv[atomicAdd(&lds_n, 1u)] = key_row(key);
        }
        __syncthreads();
        const unsigned ns = lds_n;
        survivors += ns;
        // eight rows per wave step: two independent groups of four, so that both groups' row reads are in flight
        // before the first is consumed (the loop is a chain of HBM round trips otherwise)
        for (unsigned j0 = wave * 8; j0 < ns; j0 += 8 * kFinWaves) {
            unsigned rowid8[2][4];
            float sc8[1][8];
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int r = 0; r < 4; ++r) rowid8[h][r] = lds_surv[j0 + 4 * h + r < ns ? j0 + 4 * h + r : ns - 1];
            if constexpr (NITER == kWideRows && E == 4) {  // (f32: one segment of all eight rows at a time, 32 loads in flight)
                const uint4* p[8];
#pragma unroll
                for (int hr = 0; hr < 8; ++hr) p[hr] = base + (int64_t)rowid8[hr >> 2][hr & 3] * nchunks + lane;
                wide_scores<DT, 1, 2, METRIC>(p, nchunks, lane, lds_q, 0, 1, sc8);
            } else {
                float s0[1][4], s1[1][4];
                rescore4(rowid8[0], s0);
                rescore4(rowid8[1], s1);
#pragma unroll
                for (int r = 0; r < 4; ++r) { sc8[0][r] = s0[0][r]; sc8[0][4 + r] = s1[0][r]; }
            }
#pragma unroll
            for (int hr = 0; hr < 8; ++hr)
                if (j0 + hr < ns) X.offer(make_key(sc8[0][hr], row_base + rowid8[hr >> 2][hr & 3]), k, lane);
        }
        __syncthreads();  // lds_surv is refilled by the next round
    }
    if (tid == 0 && stats) {
        if (part == 0) atomicAdd(&stats[0], (unsigned long long)total);
        atomicAdd(&stats[1], (unsigned long long)survivors);
    }

    // 4. merge the waves' lists
    store_list(lds_list, wave, 1, 0, lane, X);
    __syncthreads();
    if (wave == 0) {
        merge_lists(X, lds_list, 1, kFinWaves, 1, 0, k, lane);
        // one share of several: its keys for the merge launch; else the caller's (distance, row) outputs straight from here
        if (nparts > 1) write_keys(X, k, lane, part_keys_q);
        else write_ranks<SLOTS, METRIC>(X, k, lane, out_keys_q, out_dist_q, out_rows_q);
    }
    __syncthreads();  // (a caller that loops over queries reuses the shared lists)
}

template <int DT, int NITER, int SLOTS>
__global__ __launch_bounds__(kFinThreads) void finalize_kernel(const void* __restrict__ rows_, int dpad, const float* __restrict__ qn,
                                                       const u64* __restrict__ hits, const unsigned* __restrict__ hit_cnt,
                                                       int cap_q, unsigned* __restrict__ flags, int k, float two_eps,
                                                       uint32_t row_base, u64* __restrict__ out_keys,
                                                       unsigned* __restrict__ fb_count, unsigned* __restrict__ fb_list,
                                                       unsigned long long* __restrict__ stats, const float* __restrict__ two_eps_q = nullptr,
                                                       u64* __restrict__ part_keys = nullptr, float* __restrict__ out_dist = nullptr,
                                                       int64_t* __restrict__ out_rows = nullptr, const float2* __restrict__ bmeta = nullptr,
                                                       const uint32_t* __restrict__ dead = nullptr) {
    // bmeta (int8 filter; two_eps_q = qmeta + 256): the slack is evaluated per 32-row block, eps(q, block) = A(q) + B(q) e_block
    // (A at two_eps_q[256 + q], B at two_eps_q[512 + q], e_block = bmeta[row / 32].y): a hit survives iff
    // approx + B e_block >= L' - A.  Valid whichever kernel wrote the hit list (every kernel's list holds these rows).
    // gridDim.y > 1: the query's hit list is shared out between gridDim.y workgroups (contiguous shares), each
    // writes its own top-k to part_keys[(q * P + p) * k ..] and a merge launch follows.  With one or a few queries
    // and thousands of survivors (the int8 filter) one workgroup per query would do all the re-scoring on one CU.
    const int q = blockIdx.x;
    const unsigned total = hit_cnt[q * kHitCntStride];
    const unsigned part = blockIdx.y, nparts = gridDim.y;
    if (total > (unsigned)cap_q) {  // the candidate list was truncated: only the exact scan can answer this query
        if (threadIdx.x == 0 && part == 0) {
            fb_list[atomicAdd(fb_count, 1u)] = (unsigned)q;
            atomicOr(&flags[FLAG_NEED_FALLBACK], 1u);
        }
        return;
    }
    const float eps1 = bmeta ? two_eps_q[256 + q] : 0.5f * (two_eps_q ? two_eps_q[q] : two_eps);
    const float bq = bmeta ? two_eps_q[512 + q] : 0.0f;
    finalize_body<DT, NITER, SLOTS>(rows_, dpad, qn + (int64_t)q * dpad, hits + (int64_t)q * cap_q, total, part, nparts, k, eps1, bq, bmeta, row_base,
                                    out_keys ? out_keys + (int64_t)q * k : nullptr, out_dist ? out_dist + (int64_t)q * k : nullptr,
                                    out_rows ? out_rows + (int64_t)q * k : nullptr, part_keys ? part_keys + ((int64_t)q * nparts + part) * k : nullptr, stats, dead);
}

// finalize_kernel for an l2 index: the hits' keys are approximate -|q - c|^2, the survivors are re-scored with the
// canonical squared distance of DESIGN.md §20 and the distance written is 0 - score.  The device-wide bound only (no bmeta); rows of
// 1 .. 4 chunks per lane.
template <int DT, int NITER, int SLOTS>
__global__ __launch_bounds__(kFinThreads) void sqd_fin_kernel(const void* __restrict__ rows_, int dpad, const float* __restrict__ qn,
                                                           const u64* __restrict__ hits, const unsigned* __restrict__ hit_cnt, int cap_q,
                                                           unsigned* __restrict__ flags, int k, uint32_t row_base, u64* __restrict__ out_keys,
                                                           unsigned* __restrict__ fb_count, unsigned* __restrict__ fb_list,
                                                           unsigned long long* __restrict__ stats, const float* __restrict__ two_eps_q,
                                                           u64* __restrict__ part_keys, float* __restrict__ out_dist, int64_t* __restrict__ out_rows,
                                                           const uint32_t* __restrict__ dead) {
    static_assert(NITER != kWideRows, "the squared-distance filter leg serves rows of 1 .. 4 chunks per lane");
    const int q = blockIdx.x;
    const unsigned total = hit_cnt[q * kHitCntStride];
    const unsigned part = blockIdx.y, nparts = gridDim.y;
    if (total > (unsigned)cap_q) {  // the candidate list was truncated: only the exact scan can answer this query
        if (threadIdx.x == 0 && part == 0) {
            fb_list[atomicAdd(fb_count, 1u)] = (unsigned)q;
            atomicOr(&flags[FLAG_NEED_FALLBACK], 1u);
        }
        return;
    }
    finalize_body<DT, NITER, SLOTS, kMetricL2>(rows_, dpad, qn + (int64_t)q * dpad, hits + (int64_t)q * cap_q, total, part, nparts, k, 0.5f * two_eps_q[q], 0.0f,
                                               nullptr, row_base, out_keys ? out_keys + (int64_t)q * k : nullptr, out_dist ? out_dist + (int64_t)q * k : nullptr,
                                               out_rows ? out_rows + (int64_t)q * k : nullptr, part_keys ? part_keys + ((int64_t)q * nparts + part) * k : nullptr,
                                               stats, dead);
}

// ---------------------------------------------------------------------------------------------
// anchor_thr_kernel: one wave per query.  The sample pass left, per bucket (sampled tile), the (approximate score, row)
// key of its best row.  The k best buckets name k DISTINCT rows; their EXACT scores (canonical expression) are all
// >= L := the smallest of them, hence the true k-th best score is >= L and every true top-k row has an approximate
// score >= L - eps.  thr[q] = L - eps(q); -inf when fewer than k buckets hold a row; +inf for padding queries.
// (Anchoring on exact scores costs k row reads per query and saves one eps of slack against the k-th largest
// *approximate* bucket maximum: a third fewer hits for the bf16 filter, 6x fewer for the int8 one.)
// dead (tombstone bits, null: none): a bucket whose best row is deleted is no anchor — its score bounds nothing a live row
// reaches.  Fewer than k live anchors: thr = -inf as above, every row becomes a hit and the query is answered by finalize over
// all of them or, past the candidate capacity, by the exact-scan fallback queue; never a threshold from fewer than k rows.
// ---------------------------------------------------------------------------------------------
constexpr int kAnchorWaves = 4;  // waves per query: the bucket scan and the k row reads are shared out (one wave: 19 us of a 430 us shard step)
template <int DT, int NITER, int SLOTS, int METRIC, bool RE = false>
__device__ __forceinline__ void anchor_thr_body(const u64* __restrict__ bucket_key, int64_t nbuckets, int B, int k,
                                                const void* __restrict__ rows_, int dpad, const float* __restrict__ qn, float eps,
                                                const float* __restrict__ two_eps_q, float* __restrict__ thr,
                                                float* __restrict__ thr0, const uint32_t* __restrict__ dead,
                                                const u64* __restrict__ more = nullptr, unsigned nmore = 0u, unsigned bucket_row0 = 0u) {
    // RE (with more, nmore, bucket_row0): the re-anchor of the sample cascade (reanchor_thr_kernel below); every statement it adds is
    // compiled for RE alone, so anchor_thr_kernel and sqd_thr_kernel stay the kernels they were
    // thr0 (int8 filter, with two_eps_q = qmeta + 256): L - A(q), the block-independent part of the per-block threshold
    // L - A(q) - B(q) e_block that i8_tile_kernel evaluates (A at two_eps_q[256 + q])
    typedef RowTraits<DT> RT;
    constexpr int E = RT::E;
    __shared__ u64 lds_list[kAnchorWaves * SLOTS * kWave];  // the waves' lists; then [rank] of the merged one
    __shared__ float lds_worst[kAnchorWaves];
    __shared__ int lds_full;
    const int q = blockIdx.x, tid = (int)threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
    if (q >= B) {
        if (tid == 0) {
            thr[q] = INFINITY;
            if (thr0) thr0[q] = INFINITY;
        }
        return;
    }
    const int nchunks = dpad / E;
    float qf[1][NITER > 0 ? NITER : 1][E];
    float* lds_q = nullptr;
    if constexpr (NITER == kWideRows) {  // wide rows: the query in LDS (the barrier behind the bucket scan publishes it)
        __shared__ __attribute__((aligned(16))) float lds_qw[kWideMaxFloats];
        lds_q = lds_qw;
        wide_stage_query(lds_q, qn + (int64_t)q * dpad, dpad, wide_qfloats(nchunks, E), tid, kAnchorWaves * kWave);
    } else {
        load_query_frags(qn + (int64_t)q * dpad, nchunks, lane, qf[0]);
    }
    WaveTopK<SLOTS> L;
    L.init();
    for (int64_t i0 = (int64_t)wave * kWave; i0 < nbuckets; i0 += kAnchorWaves * kWave) {
        const int64_t i = i0 + lane;
        u64 key = i < nbuckets ? bucket_key[(int64_t)q * nbuckets + i] : 0ull;
        if constexpr (RE) {
            if (key) key = make_key(key_score(key), key_row(key) + bucket_row0);
        }
        if (dead && key && row_dead(dead, key_row(key))) key = 0ull;
        L.offer_lanes(key, k, lane);
    }
    if constexpr (RE) {
        for (unsigned i0 = (unsigned)wave * kWave; i0 < nmore; i0 += kAnchorWaves * kWave) {
            const unsigned i = i0 + lane;
            u64 key = i < nmore ? more[i] : 0ull;
            if (dead && key && row_dead(dead, key_row(key))) key = 0ull;
            L.offer_lanes(key, k, lane);
        }
    }
    store_list(lds_list, wave, 1, 0, lane, L);
    __syncthreads();
    if (wave == 0) {
        merge_lists(L, lds_list, 1, kAnchorWaves, 1, 0, k, lane);
        store_list(lds_list, 0, 1, 0, lane, L);  // rank s * 64 + lane
        if (lane == 0) lds_full = L.thr ? 1 : 0;
    }
    __syncthreads();
    if (!lds_full) {  // fewer than k buckets with a row: no threshold can be justified
        if constexpr (RE) return;   // (the query keeps the thresholds it had)
        if (tid == 0) {
            thr[q] = -INFINITY;
            if (thr0) thr0[q] = -INFINITY;
        }
        return;
    }
    const uint4* base = reinterpret_cast<const uint4*>(rows_);
    // exact scores of the rows ranked [j, j+4) (ranks past k-1 repeat the last one)
    auto group = [&](int j, float (&sc)[1][4]) __attribute__((always_inline)) {
        const uint4* p[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) p[r] = base + (int64_t)key_row(lds_list[j + r < k ? j + r : k - 1]) * nchunks + lane;  // (the rank is uniform)
        if constexpr (NITER == kWideRows) {
            wide_scores<DT, 1, 1, METRIC>(p, nchunks, lane, lds_q, 0, 1, sc);
        } else {
            uint4 c[4][NITER];
            fetch4(p, nchunks, lane, c);
            score4<DT, 1, NITER, METRIC>(c, qf, 1, lane, sc);
        }
    };
    float worst = INFINITY;
    if (k <= 4 * kAnchorWaves) {  // the usual case (k = 10): one group of four rows per wave, one round trip
        if (4 * wave < k) {
            float s0[1][4];
            group(4 * wave, s0);
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (4 * wave + r < k) worst = fminf(worst, s0[0][r]);
        }
    } else {
        for (int j = 8 * wave; j < k; j += 8 * kAnchorWaves) {  // two independent groups per step: both groups' row reads fly together
            float s0[1][4], s1[1][4];
            group(j, s0);
            group(j + 4, s1);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (j + r < k) worst = fminf(worst, s0[0][r]);
                if (j + 4 + r < k) worst = fminf(worst, s1[0][r]);
            }
        }
    }
    if (lane == 0) lds_worst[wave] = worst;
    __syncthreads();
    if (tid == 0) {
        float wmin = lds_worst[0];
#pragma unroll
        for (int wv = 1; wv < kAnchorWaves; ++wv) wmin = fminf(wmin, lds_worst[wv]);
        if constexpr (RE) {
            thr[q] = fmaxf(thr[q], wmin - (two_eps_q ? 0.5f * two_eps_q[q] : eps));
            if (thr0) thr0[q] = fmaxf(thr0[q], wmin - two_eps_q[256 + q]);
        } else {
            thr[q] = wmin - (two_eps_q ? 0.5f * two_eps_q[q] : eps);
            if (thr0) thr0[q] = wmin - two_eps_q[256 + q];
        }
    }
}

template <int DT, int NITER, int SLOTS>
__global__ __launch_bounds__(kAnchorWaves * kWave) void anchor_thr_kernel(const u64* __restrict__ bucket_key, int64_t nbuckets, int B, int k,
                                                                          const void* __restrict__ rows_, int dpad, const float* __restrict__ qn, float eps,
                                                                          const float* __restrict__ two_eps_q, float* __restrict__ thr,
                                                                          float* __restrict__ thr0 = nullptr, const uint32_t* __restrict__ dead = nullptr) {
    anchor_thr_body<DT, NITER, SLOTS, kMetricDot>(bucket_key, nbuckets, B, k, rows_, dpad, qn, eps, two_eps_q, thr, thr0, dead);
}

// reanchor_thr_kernel: the second anchoring of the sample cascade, one workgroup per query.  The first sample (A0)
// left its bucket keys — rows numbered from row slot bucket_row0 — and anchor_thr_kernel sound thresholds; the filter program has
// since listed every row of the tiles 0, d + 1, 2 (d + 1), ... that those thresholds admit (hits, hit_cnt).  The k best approximate
// keys of (that list U the bucket keys), dead rows dropped first, name k distinct live rows (A0's tiles are none of A1's); L is their
// smallest canonical score and thr, thr0 follow by anchor_thr_kernel's formulas.  The old threshold and the new one are each a lower
// bound on the approximate score of every top-k row, so the larger of the two is written: the thresholds only ever tighten, and
// a query with fewer than k live candidates keeps what it had.  A list that overflowed cap_q lends its first cap_q rows (real rows:
// sound anchors); finalize sends that query to the exact scan as ever.
template <int DT, int NITER, int SLOTS>
__global__ __launch_bounds__(kAnchorWaves * kWave) void reanchor_thr_kernel(const u64* __restrict__ bucket_key, int64_t nbuckets, unsigned bucket_row0,
                                                                            const u64* __restrict__ hits, const unsigned* __restrict__ hit_cnt, int cap_q, int B,
                                                                            int k, const void* __restrict__ rows_, int dpad, const float* __restrict__ qn, float eps,
                                                                            const float* __restrict__ two_eps_q, float* __restrict__ thr,
                                                                            float* __restrict__ thr0, const uint32_t* __restrict__ dead) {
    const int q = blockIdx.x;
    if (q >= B) return;   // (padding queries keep anchor_thr_kernel's +inf)
    const unsigned cnt = hit_cnt[q * kHitCntStride];
    anchor_thr_body<DT, NITER, SLOTS, kMetricDot, true>(bucket_key, nbuckets, B, k, rows_, dpad, qn, eps, two_eps_q, thr, thr0, dead, hits + (int64_t)q * cap_q,
                                                        cnt < (unsigned)cap_q ? cnt : (unsigned)cap_q, bucket_row0);
}

// anchor_thr_kernel for an l2 index: the anchors' exact scores are 0 - (canonical squared distance), so
// thr[q] = -(the largest of the k anchor distances) - eps(q), a threshold on the filter's approximate -|q - c|^2
template <int DT, int NITER, int SLOTS>
__global__ __launch_bounds__(kAnchorWaves * kWave) void sqd_thr_kernel(const u64* __restrict__ bucket_key, int64_t nbuckets, int B, int k,
                                                                              const void* __restrict__ rows_, int dpad, const float* __restrict__ qn,
                                                                              const float* __restrict__ two_eps_q, float* __restrict__ thr,
                                                                              const uint32_t* __restrict__ dead) {
    static_assert(NITER != kWideRows, "the squared-distance filter leg serves rows of 1 .. 4 chunks per lane");
    anchor_thr_body<DT, NITER, SLOTS, kMetricL2>(bucket_key, nbuckets, B, k, rows_, dpad, qn, 0.0f, two_eps_q, thr, nullptr, dead);
}

}  // namespace codd
