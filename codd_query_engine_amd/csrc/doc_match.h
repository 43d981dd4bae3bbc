// doc_match.h — substring match over the document arena: which documents contain a needle, as a row bitmap.
//
// The arena holds every row slot's document back to back, one 0x00 behind each, zeros from the last separator to the end of the
// allocation: document r = arena[offsets[r] .. offsets[r + 1] - 1), offsets[count] = the arena's bytes.  A needle holds no 0x00, so
//   - a match cannot span two documents (it would have to contain the separator between them), and
//   - no position in the zero padding, and no window that reaches into it, can match: every load below is unconditional.
//
// doc_match_kernel is position-parallel: its cost is the arena's bytes whatever the documents' lengths are.  A workgroup takes
// tiles of kDocTile arena bytes (grid-stride), brings a tile and kDocOverlap bytes behind it into LDS with 16-byte loads, and
// every lane tests the 16 start positions of each of its 16-byte chunks: the needle's first (up to four) bytes against a window
// shifted out of two registers, and only where that holds the rest of the needle, byte by byte from LDS.  A match at arena
// position p belongs to the document r with offsets[r] <= p < offsets[r + 1] (binary search) and sets bit r; a lane remembers the
// document it marked last and skips the search and the atomic for further matches inside it, and tests the bit before the atomic.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace codd {

constexpr int kDocMaxNeedle = 256;             // == CODD_KNN_MAX_NEEDLE
constexpr int kDocTile = 16384;                // start positions per tile ("doc_tile_bytes")
constexpr int kDocOverlap = kDocMaxNeedle;     // bytes staged behind a tile: a needle that starts at its last byte ends inside them
constexpr int kDocThreads = 256;
constexpr int kDocStaged16 = (kDocTile + kDocOverlap) / 16;          // 16-byte pieces staged per tile
constexpr int kDocChunksPerThread = kDocTile / 16 / kDocThreads;     // 16-byte chunks of start positions per thread and tile
static_assert(kDocTile % (16 * kDocThreads) == 0 && kDocOverlap % 16 == 0 && kDocOverlap >= kDocMaxNeedle, "tile shape");

// the allocation that makes every staged load of ceil(bytes / kDocTile) tiles land inside it
__host__ __device__ constexpr int64_t doc_arena_alloc_bytes(int64_t bytes) {
    return (bytes + kDocTile - 1) / kDocTile * kDocTile + kDocOverlap;
}

// the needle travels as a kernel argument: copied at launch, the caller's bytes are not read again
struct DocNeedle {
    uint32_t w[kDocMaxNeedle / 4];   // its bytes, zero padded
};

// grid: any number of workgroups up to `tiles`; bits[] cleared by the caller on the same stream
__global__ __launch_bounds__(kDocThreads) void doc_match_kernel(const uint4* __restrict__ arena, int64_t bytes, int64_t tiles,
                                                                const int64_t* __restrict__ offsets, int64_t count, DocNeedle needle,
                                                                int len, uint32_t* __restrict__ bits) {
    __shared__ uint4 s_tile[kDocStaged16];
    __shared__ uint32_t s_needle[kDocMaxNeedle / 4];
    const int tid = (int)threadIdx.x;
    if (tid < kDocMaxNeedle / 4) s_needle[tid] = needle.w[tid];
    const uint32_t head = needle.w[0];                                        // the pre-test: the first min(len, 4) bytes
    const uint32_t head_mask = len >= 4 ? 0xffffffffu : (1u << (8 * len)) - 1u;
    const uint8_t* tile_bytes = reinterpret_cast<const uint8_t*>(s_tile);
    const uint32_t* tile_words = reinterpret_cast<const uint32_t*>(s_tile);
    const uint8_t* needle_bytes = reinterpret_cast<const uint8_t*>(s_needle);

    int64_t hit_begin = 0, hit_end = 0;   // arena range of the document this lane set the bit of last: a frequent needle (" | ", "e")
                                          // matches many times per document, and only the first match pays the search and the atomic
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int64_t base = t * kDocTile;
        const uint4* src = arena + base / 16;
        __syncthreads();   // (the previous tile's readers are done; the needle is in LDS)
#pragma unroll
        for (int i = 0; i < (kDocStaged16 + kDocThreads - 1) / kDocThreads; ++i) {
            const int at = i * kDocThreads + tid;
            if (at < kDocStaged16) s_tile[at] = src[at];
        }
        __syncthreads();
#pragma unroll 1   // (one chunk's sixteen tests at a time: unrolled over the chunks the kernel holds 134 registers, three waves per SIMD)
        for (int i = 0; i < kDocChunksPerThread; ++i) {
            const int c = i * kDocThreads + tid;   // chunk of the tile: start positions c * 16 .. c * 16 + 15
            const uint4 v = s_tile[c];
            const uint32_t w[5] = {v.x, v.y, v.z, v.w, tile_words[c * 4 + 4]};
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const uint64_t two = ((uint64_t)w[j / 4 + 1] << 32) | (uint64_t)w[j / 4];
                const uint32_t window = (uint32_t)(two >> (8 * (j % 4)));
                if (((window ^ head) & head_mask) != 0u) continue;
                const int at = c * 16 + j;
                bool same = true;
                for (int b = 4; b < len; ++b)
                    if (tile_bytes[at + b] != needle_bytes[b]) { same = false; break; }
                const int64_t p = base + at;
                if (!same || p >= bytes) continue;   // (p < bytes always: a match holds no 0x00, the padding nothing else)
                if (p >= hit_begin && p < hit_end) continue;   // the document this lane marked last: its bit is set
                int64_t lo = 0, hi = count;          // the document with offsets[lo] <= p < offsets[lo + 1]
                while (hi - lo > 1) {
                    const int64_t mid = lo + (hi - lo) / 2;
                    if (offsets[mid] <= p) lo = mid; else hi = mid;
                }
                hit_begin = offsets[lo];
                hit_end = offsets[lo + 1];
                const uint32_t bit = 1u << (uint32_t)(lo & 31);
                if ((__builtin_nontemporal_load(&bits[lo >> 5]) & bit) == 0u) atomicOr(&bits[lo >> 5], bit);   // (a stale read costs one redundant atomic)
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// A mask that is already on the device (codd_knn_search_masked_dev): the caller's words clipped to [0, n) into the index's own
// allow buffer, and the rows they leave visible — allowed and not dead — counted into *visible (zeroed by the caller on the
// same stream): per workgroup one LDS reduction and one atomic.
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mask_clip_count_kernel(const uint32_t* __restrict__ in, const uint32_t* __restrict__ dead, int64_t n, int64_t nwords,
                                                              uint32_t* __restrict__ allow, unsigned long long* __restrict__ visible) {
    __shared__ unsigned s_sum[256];
    const int tid = (int)threadIdx.x;
    const int64_t w = (int64_t)blockIdx.x * 256 + tid;
    unsigned mine = 0u;
    if (w < nwords) {
        const int64_t left = n - w * 32;
        const uint32_t a = in[w] & (left >= 32 ? 0xffffffffu : (left > 0 ? (1u << (uint32_t)left) - 1u : 0u));
        allow[w] = a;
        mine = (unsigned)__popc(a & ~(dead ? dead[w] : 0u));
    }
    s_sum[tid] = mine;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (tid < off) s_sum[tid] += s_sum[tid + off];
        __syncthreads();
    }
    if (tid == 0 && s_sum[0] != 0u) atomicAdd(visible, (unsigned long long)s_sum[0]);
}

// ---------------------------------------------------------------------------------------------------------------------------
// A shard's words out of a mask over GLOBAL rows (codd_knn_slice_mask): out word w holds the global bits
// [row_base + 32 w, row_base + 32 w + 32) — a funnel shift of the two global words they lie in, row_base being arbitrary — with
// the bits past global_rows or past the shard's count zero.  One thread per output word; no load past the last global word.
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mask_slice_kernel(const uint32_t* __restrict__ global_bits, int64_t global_rows, int64_t row_base, int64_t count,
                                                         uint32_t* __restrict__ out, int64_t nwords) {
    const int64_t w = (int64_t)blockIdx.x * 256 + (int64_t)threadIdx.x;
    if (w >= nwords) return;
    const int64_t gwords = (global_rows + 31) >> 5;
    const int64_t first = row_base + w * 32;   // the global row of this word's bit 0
    const int64_t gw = first >> 5;
    const uint32_t sh = (uint32_t)(first & 31);
    const uint32_t lo = gw < gwords ? global_bits[gw] : 0u;
    const uint32_t hi = sh != 0u && gw + 1 < gwords ? global_bits[gw + 1] : 0u;
    const uint32_t v = sh != 0u ? (lo >> sh) | (hi << (32u - sh)) : lo;
    const int64_t left_g = global_rows - first, left_c = count - w * 32;
    const int64_t left = left_g < left_c ? left_g : left_c;
    out[w] = v & (left >= 32 ? 0xffffffffu : (left > 0 ? (1u << (uint32_t)left) - 1u : 0u));
}

}  // namespace codd
