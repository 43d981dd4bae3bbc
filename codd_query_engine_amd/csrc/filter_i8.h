// filter_i8.h — the int8 filter GEMM for batches of 65..256 queries on rows of 384 elements or more (3 K-steps),
// second generation.  Same operands, same layouts, same hit lists as gemm_filter_kernel<MODE, 8, EL = 1> in
// filter_gemm.h (which stays the kernel of every other shape); what changed is the schedule:
//
//   * round 1's loop compiled to `ds_read_b128 -> s_waitcnt lgkmcnt(0) -> 2 MFMA` 32 times per K-step with ONE query
//     fragment register set: every MFMA pair paid a full LDS round trip (profiles/r2/i8_v1_isa_excerpt.txt; matrix pipe
//     38 % busy, LDS array 26 % busy, waves parked 56 % of their cycles).  Here the query fragments run through a ring
//     of kBD register sets and the order of a K-step is pinned;
//   * the query slices go L2 -> LDS by LDS-DMA (buffer_load ... lds), not through 16 staging registers and ds_write: with
//     128 accumulator and 48 corpus-ring registers the staging set pushed the wave over the 256 registers it has at two
//     waves per SIMD (hipcc spilled, and every scratch reload waits vmcnt(0));
//   * EVERY vector-memory operation of the loop is issued by inline asm and waited for by hand with counted vmcnt
//     (the queue retires in order; per interval it receives, in this order: 1 scale load, 4 DMA, 4 corpus loads).
//     hipcc sees no load in flight, so it inserts no wait of its own: with the DMA visible it ordered every LDS access
//     it could see behind the youngest DMA, and a false register dependency on an in-flight load cost a vmcnt(0)
//     inside the epilogue (measured: 5 us per tile).  The fragment reads of the MFMA phase are inline asm too, with
//     counted lgkmcnt; values flow from each wait asm to their consumers as in/out operands;
//   * waves 4..7 (the SIMD partners of waves 0..3) can run one K-step behind (CODD_I8_LAG), and a tile's epilogue is
//     deferred to the start of the wave's next interval;
//   * the epilogue tests a block pair on its largest accumulator first — max of the lane's 8 accumulators of (2 row blocks x
//     1 query block) times the block's scale against the query's threshold: 9 vector instructions per pair instead of 26.
//     The int8 shadow carries ONE scale per 32-row block (= per wave tile), so that pre-test is exact at pair level and only
//     pairs that hold a hit (about one in eight) take the per-value test — same expression as the first-generation kernel,
//     so the hit lists are the same — which runs straight-line (select + count, one append) unless a lane holds two hits;
//   * the sample mode folds the wave's 32 rows as packed (accumulator << 5 | 31 - row) ints: integer max, two lane swaps,
//     one (score, row) key per query and wave;
//   * row scales reach the epilogue through LDS (one small DMA per wave and interval), not through global loads inside a
//     conditional region;
//   * the workgroup's hit-list bookkeeping rides on the interval barrier: no extra barriers per tile;
//   * instantiations: NQB = 16 / 8 query blocks (129..256 / 65..128 queries); RES: rows of <= 4 K-steps keep the whole query
//     block in the four LDS slices (staged once per workgroup, no slice DMA per interval) and synchronise once per tile
//     instead of once per K-step (hit lists and sample keys double-buffered by tile parity).
//
// LDS: 4 query slices x 32 KiB | 1088 bookkeeping words | 2 row-scale buffers x (256 + 16) floats | hit list.
#pragma once
#include "filter_gemm.h"
#include "geometry.h"

#if !CODD_EXPERIMENTS && (defined(CODD_I8_EXP_NOEPI) || defined(CODD_I8_EXP_NODMA) || defined(CODD_I8_EXP_SAMETILE) || defined(CODD_I8_EXP_NOBARRIER) || \
                          defined(CODD_I8_EXP_NOBREAD) || defined(CODD_I8_EXP_NOHITS) || defined(CODD_I8_EXP_NOAPPEND) || defined(CODD_I8_EXP_NOFLUSH) || defined(CODD_I8_EXP_NOGLOBAL) || \
                          defined(CODD_I8_EXP_STAMPS))
#error "the CODD_I8_EXP_* switches return wrong results or race: they exist only in -DCODD_EXPERIMENTS=1 builds (build_variant)"
#endif

namespace codd {

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kI8SliceBytes = 32768;  // one 128-wide K slice of the 256-query block
constexpr int kI8RsBufs = 2;          // row-scale buffers (tile ordinal & 1): a tile's scales are read (its epilogue, at the start of the next tile) before the tile after next requests its own
constexpr int kI8RsStride = 272;      // floats per buffer: 256 row scales + 8 per-wave maxima (+ pad)
#if !CODD_EXPERIMENTS && (defined(CODD_I8_BDEPTH) || defined(CODD_I8_EARLY_FRAGS) || defined(CODD_I8_LAG) || defined(CODD_I8_SPREAD_VM) || defined(CODD_I8_FUSE_EPI) || \
                          defined(CODD_I8_EARLY_A))
#error "CODD_I8_BDEPTH / CODD_I8_EARLY_FRAGS / CODD_I8_LAG / CODD_I8_EARLY_A ... are schedule experiments: only their defaults are under test; -DCODD_EXPERIMENTS=1 builds (build_variant) may set them"
#endif
#ifndef CODD_I8_BDEPTH
#define CODD_I8_BDEPTH 4              // query-fragment register sets in flight
#endif
constexpr int kBD = CODD_I8_BDEPTH;
#ifndef CODD_I8_EARLY_FRAGS
#define CODD_I8_EARLY_FRAGS 1         // the first fragment reads of a K-step go out before the interval's DMA / corpus-load instructions (0: behind them)
#endif
#ifndef CODD_I8_LAG
#define CODD_I8_LAG 0                 // 1: waves 4..7 run one K-step behind waves 0..3 (measured 12 % slower twice, profiles/r2/i8_tile_ablation.txt; experiment builds only)
#endif
#ifndef CODD_I8_SPREAD_VM
#define CODD_I8_SPREAD_VM 0           // pair program: 1 = the interval's vector-memory operations are issued one at a time behind MFMA groups instead of in a
                                      // block in front of them; 2 = ... the SIMD partners taking turns (waves 0..3 behind even groups, 4..7 behind odd ones)
#endif
#ifndef CODD_I8_EARLY_A
#define CODD_I8_EARLY_A 3             // static six-step program, bit mask: the corpus loads of interval 2 (bit 0) / 4 (bit 1) go out in the tail of the odd interval
                                      // in front of it, BEFORE the barrier (0: in the interval's own head, behind the barrier, with everything else)
#endif
#ifndef CODD_I8_FUSE_EPI
#define CODD_I8_FUSE_EPI 0            // 1: the tile-structured filter program tests tile i's accumulators INSIDE the first K-step of tile i + 1 (epi_pair in front
                                      // of the MFMAs that restart the pair).  Built, bit-equal, measured 1.7-3 % SLOWER (profiles/r3/i8_tile_ablation.txt): the
                                      // pre-tests' vector instructions slow the MFMA stream they sit in by as much as the standalone block costs
#endif

// ---- hand-issued memory operations (see the header) --------------------------------------------------------------
// HAZARD (found in round 3 as non-deterministic lost neighbours): gfx9 needs 5 wait states between a VALU instruction that
// WRITES an SGPR (v_readfirstlane, and v_readlane — which is how hipcc reloads the SGPRs this kernel spills to VGPR lanes,
// 2,400 times in the program) and a vector-memory instruction that READS that SGPR (descriptor, soffset).  hipcc pads its
// own instructions for this; it does not look inside inline asm.  A descriptor word produced right in front of one of
// these statements was read STALE: a K-step's corpus fragment came from a wrong address, non-deterministically, and whether
// it happened depended on register pressure (it appeared with one more live SGPR).  Every statement below therefore
// carries its own wait states in front of the memory instruction (the s_mov to m0 counts as one).
// buffer descriptor (4 SGPRs): base, 48-bit address | stride 0, bytes, gfx950 raw-buffer flags; out-of-range reads return 0
__device__ __forceinline__ i32x4 i8_rsrc(const void* p, unsigned bytes) {
    const unsigned long long a = (unsigned long long)p;
    i32x4 r;  // (readfirstlane: the asm operands are SGPR tuples whatever hipcc's uniformity analysis concludes)
    r[0] = __builtin_amdgcn_readfirstlane((int)(unsigned)a);
    r[1] = __builtin_amdgcn_readfirstlane((int)((unsigned)(a >> 32) & 0xffffu));
    r[2] = __builtin_amdgcn_readfirstlane((int)bytes);
    r[3] = 0x00020000;
    return r;
}
template <int OFF>
__device__ __forceinline__ void i8_load_b128_nt(u32x4& dst, int voff, i32x4 rsrc) {  // read-once stream: non-temporal
    // (s_nop 4: the HAZARD note above)
    asm volatile("s_nop 4\n\tbuffer_load_dwordx4 %0, %1, %2, 0 offen offset:%3 nt" : "=v"(dst) : "v"(voff), "s"(rsrc), "n"(OFF));
}
// (m0 is on the clobber lists: hipcc reserves it for its own implicit uses — each is preceded by its own s_mov m0 — and warns that a
// reserved register "may not be preserved"; listing it is what keeps its scheduler from placing these statements between such a pair)
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"
// 64 lanes x 16 bytes: global (rsrc + voff + soff) -> LDS [lds_addr + 16 * lane]
__device__ __forceinline__ void i8_dma_b128(unsigned lds_addr, int voff, i32x4 rsrc, int soff) {
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 3\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds" ::"s"(__builtin_amdgcn_readfirstlane((int)lds_addr)), "v"(voff), "s"(rsrc),
                 "s"(__builtin_amdgcn_readfirstlane(soff))
                 : "memory", "m0");
}
// the same for operands that ARE scalar registers already (the static tile program: a v_readfirstlane hipcc does not fold costs a
// vector register for its source, and that one — loop-invariant — was spilled to scratch and reloaded with a vmcnt(0) per tile)
__device__ __forceinline__ void i8_dma_b128_s(unsigned lds_addr, int voff, i32x4 rsrc, int soff) {
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 3\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds" ::"s"(lds_addr), "v"(voff), "s"(rsrc), "s"(soff) : "memory", "m0");
}
// 64 lanes x 4 bytes: global (rsrc + voff + soff) -> LDS [lds_addr + 4 * lane]
__device__ __forceinline__ void i8_dma_b32(unsigned lds_addr, int voff, i32x4 rsrc, int soff) {
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 3\n\tbuffer_load_dword %1, %2, %3 offen lds" ::"s"(__builtin_amdgcn_readfirstlane((int)lds_addr)), "v"(voff), "s"(rsrc),
                 "s"(__builtin_amdgcn_readfirstlane(soff))
                 : "memory", "m0");
}
#pragma clang diagnostic pop
template <int N>
__device__ __forceinline__ void i8_wait_vm(u32x4& a, u32x4& b, u32x4& c, u32x4& d) {
    asm volatile("s_waitcnt vmcnt(%4)" : "+v"(a), "+v"(b), "+v"(c), "+v"(d) : "n"(N));
}
template <int OFF>
__device__ __forceinline__ void lds_read_b128_asm(i32x4& dst, unsigned addr) {
#ifdef CODD_I8_EXP_NOBREAD
    asm volatile("; no read %0 %1 %2" : "=v"(dst) : "v"(addr), "n"(OFF));  // diagnostic: no LDS read at all
#else
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(OFF));
#endif
}
template <int N>
__device__ __forceinline__ void lgkm_wait_asm(i32x4& v) {
    asm volatile("s_waitcnt lgkmcnt(%1)" : "+v"(v) : "n"(N));
}

__device__ __forceinline__ float i8_wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}

// vector-memory operations per interval, in issue order: scale DMA, kDmaPerIv slice DMA, kAPerIv corpus loads
// (kDmaPerIv = NQB / 4: a slice of 16 NQB queries is NQB / 2 chunks of 1 KiB per wave pair... 2 NQB KiB in all, 8 waves)
constexpr int kAPerIv = 4;
// bookkeeping words behind the slices: [0..127] pre-test thresholds, two bf16 per word (layout: the kernel's set-up); [256], [257] hit counts;
// [260..263] the waves' maxima of u_q; [320..575] query scales; [576..831] exact thresholds (thr0 / qscale), by query; [832..1087] scratch of the in-loop flush.
// SAMPLE: [0..511] = 256 u64 keys.
constexpr int kI8Words = 1344;   // ... [1088..1343] u_q = B(q) / qscale_q (FILTER)

// (does the resident program apply?  i8_tile_resident(): geometry.h)

__host__ __device__ constexpr size_t i8_lds_bytes(int mode) {
    return (size_t)4 * kI8SliceBytes + kI8Words * 4 + kI8RsBufs * kI8RsStride * 4 + (mode == MODE_FILTER ? (size_t)kHitCap * 12 : 0);
}

// STEPS3: the row has a multiple of 3 K-steps (the host picks the instantiation): tiles start at corpus-ring phase 0.
// NQB: query blocks of 16 the launch multiplies: 16 (129..256 queries) or 8 (65..128: half the MFMAs, half the slice bytes;
// the slices keep their 32 KiB slots and the bookkeeping its 256-query layout).
// RES: the whole query block fits the four LDS slices (rows of <= 4 K-steps; <= 8 K-steps with 8 query blocks, whose slices
// are half as big): every workgroup loads it once and no slice is re-staged per tile (the host picks it: i8_tile_resident();
// LAG builds keep the staged program).
// TS (tile structure; the host picks it): 0 = generic interval loop; 1 = rows whose K-steps are a multiple of 3 (tiles start at
// corpus-ring phase 0: the tile-structured program, "STEPS3"); 2 = ... a multiple of 6 (768 elements), staged slices: the same
// program with ONE workgroup barrier per TWO K-steps.  The four LDS slices hold the two slices being read and the two
// landing; the barrier behind every odd K-step hands both pairs over at once (the barrier behind an even K-step protected
// nothing that the next one does not: slot (t + 2) & 3, requested during step t, was last read during step t - 2).
// F16 (round 3): the same program over the 2-BYTE shadow (fp16; filter_gemm.h: identical piece order, a 128-byte K-step is 64 elements, two
// v_mfma_f32_16x16x32_f16 per block pair instead of two v_mfma_i32_16x16x64_i8 — byte for byte the same operand traffic and the same matrix time per
// byte).  The accumulators ARE the approximate scores (no scales, no quantisation error: the bound lives in thr[q] = L - eps, anchor_thr_kernel),
// `thr` holds one threshold per query, `bmeta` only has to be 256 readable bytes (the per-tile metadata DMA is kept so that the counted waits stay the
// same: what it fetches is never read), `rscale` and `qscale` are not read.  Filter pass only (the sample pass of the 2-byte filter stays gemm_filter_kernel's).
// The program itself is filter_i8_body.inc, the body of both kernels below (as filter_gemm_body.inc is of the first generation's): a
// wrapper around an inlined function template moved registers in half of the instantiations, so the text is shared instead.
template <int MODE, int TS, int NQB = 16, bool RES = false, bool F16 = false>
__global__ __launch_bounds__(512, 2) void i8_tile_kernel(const uint4* __restrict__ shadow8, const uint4* __restrict__ qfrag8, int64_t n, int nsteps,
                                                         int64_t ntiles_run, int64_t tile_stride, const float* __restrict__ thr,
                                                         u64* __restrict__ bucket_key, u64* __restrict__ hits, unsigned* __restrict__ hit_cnt,
                                                         int cap_q, unsigned* __restrict__ flags, const float* __restrict__ rscale,
                                                         const float* __restrict__ qscale, const float2* __restrict__ bmeta = nullptr, float eb_scale = 1.0f,
                                                         int skip_d = 0) {
    constexpr bool SWEEP = false;
#include "filter_i8_body.inc"
}

// SWEEP: the static six-step program with the K order turned round on tiles of odd ordinal, so that a tile stages two query slices
// instead of six (geometry.h: the sweep_* plan).  int32 accumulation is associative: the accumulators, and with them
// the hit lists, hold the same bits in either order.  The filter pass over rows of exactly 6 K-steps (768 elements), staged int8
// operands: i8_tile_kernel<MODE_FILTER, 3, NQB>'s arguments, LDS and hit lists.  (Only NQB is meant to be chosen.)
template <int NQB, int MODE = MODE_FILTER, int TS = 3, bool RES = false, bool F16 = false, bool SWEEP = true>
__global__ __launch_bounds__(512, 2) void i8_sweep_kernel(const uint4* __restrict__ shadow8, const uint4* __restrict__ qfrag8, int64_t n, int nsteps,
                                                         int64_t ntiles_run, int64_t tile_stride, const float* __restrict__ thr,
                                                         u64* __restrict__ bucket_key, u64* __restrict__ hits, unsigned* __restrict__ hit_cnt,
                                                         int cap_q, unsigned* __restrict__ flags, const float* __restrict__ rscale,
                                                         const float* __restrict__ qscale, const float2* __restrict__ bmeta, float eb_scale,
                                                         int skip_d) {
    static_assert(MODE == MODE_FILTER && TS == 3 && !RES && !F16 && SWEEP, "the sweep form of the static filter program");
#include "filter_i8_body.inc"
}

}  // namespace codd
