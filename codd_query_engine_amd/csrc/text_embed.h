// text_embed.h — the hashing embedder on the device: ASCII text in, the bits of HashingEmbeddingFunction out.
//
// The arena holds the texts back to back WITHOUT separators: text r = bytes[off[r] .. off[r + 1]), and 0x00 is an ordinary non-word
// byte.  A word byte is [0-9A-Za-z_], low() maps A-Z to a-z, a token is a maximal run of word bytes inside one text.  For every
// word byte at position p, in increasing p:
//     if p starts a token:  out[crc32("w:" + low(token)) % dim] += 1.0f
//     always:               out[crc32("t:" + a + low(b[p]) + c) % dim] += tw      a = low(b[p - 1]) or '^' at a token's start,
//                                                                                  c = low(b[p + 1]) or '$' at its end
// — the host's word feature and its "^tok$" trigrams, in the host's order.  A bucket is an fp32 sum taken in exactly that order, and
// fp32 addition does not commute with itself: the order is part of the result's bits.
//
// text_embed_kernel: one 64-lane workgroup (one wave) per text, grid-stride over the texts.  The wave keeps the text's `dim` floats
// in LDS and walks the text 64 positions per step; a lane hashes its position's trigram, and the lane at a token's start walks the
// token for the word feature.  A step's up to 128 features are numbered f = 2 * lane (word) and 2 * lane + 1 (trigram): text order.
// They are added in rounds: every pending feature claims its bucket's TAG with an LDS atomicMin of f, the feature whose number the
// tag then holds adds its weight (a plain LDS read-modify-write: it is alone on that bucket), clears the tag and retires; the others
// come back in the next round.  A bucket therefore takes its additions in increasing f, whatever the lanes' timing — no float atomic
// exists in the kernel.  kEmbedTags tags serve all buckets (tag of bucket b: b % kEmbedTags): two buckets that share a tag only wait
// for each other, each still sees its own features in order.  The accumulator leaves as coalesced dword stores: every element of
// out[n][dim] is written, a bucket without a feature as +0.0.
//
// Every load is bounds-checked against the text's own [off[r], off[r + 1]): nothing outside the arena is touched whatever the
// offsets are, and a byte at or above 0x80 (the host refuses them) is a non-word byte.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace codd {

constexpr int kEmbedThreads = 64;        // one wave: __syncthreads() orders its LDS phases and costs no s_barrier
constexpr int kEmbedTags = 256;          // static LDS: 1 KiB of tags; dynamic LDS: dim floats
constexpr int kEmbedMinDim = 8, kEmbedMaxDim = 4096;
constexpr uint32_t kEmbedNoTag = 0xffffffffu;
static_assert(kEmbedThreads == 64, "text_embed_kernel votes with __any: its workgroup is exactly one wave");

__host__ __device__ constexpr uint32_t crc32_byte(uint32_t state, uint32_t byte) {   // zlib's: reflected 0xEDB88320, one byte into the running state
    state ^= byte;
    for (int i = 0; i < 8; ++i) state = (state >> 1) ^ (0xEDB88320u & (0u - (state & 1u)));
    return state;
}
constexpr uint32_t kCrcAfterW = crc32_byte(crc32_byte(0xffffffffu, 'w'), ':');   // the state behind "w:" ...
constexpr uint32_t kCrcAfterT = crc32_byte(crc32_byte(0xffffffffu, 't'), ':');   // ... and behind "t:"
static_assert((crc32_byte(crc32_byte(crc32_byte(0xffffffffu, 'a'), 'b'), 'c') ^ 0xffffffffu) == 0x352441c2u, "crc32(\"abc\")");

__host__ __device__ constexpr bool embed_is_word(uint32_t c) {
    return (c >= '0' && c <= '9') || (c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z') || c == '_';
}
__host__ __device__ constexpr uint32_t embed_low(uint32_t c) { return c >= 'A' && c <= 'Z' ? c + 32u : c; }

// grid: any number of workgroups up to n; dynamic LDS: dim * sizeof(float)
__global__ __launch_bounds__(kEmbedThreads) void text_embed_kernel(const uint8_t* __restrict__ bytes, const int64_t* __restrict__ off, int64_t n, int dim,
                                                                   float tw, float* __restrict__ out) {
    extern __shared__ float s_acc[];            // [dim]
    __shared__ uint32_t s_tag[kEmbedTags];
    const int lane = (int)threadIdx.x;
    const uint32_t udim = (uint32_t)dim;
    for (int i = lane; i < kEmbedTags; i += kEmbedThreads) s_tag[i] = kEmbedNoTag;

    for (int64_t r = blockIdx.x; r < n; r += gridDim.x) {
        for (int i = lane; i < dim; i += kEmbedThreads) s_acc[i] = 0.0f;
        __syncthreads();
        const int64_t begin = off[r], end = off[r + 1];
        for (int64_t base = begin; base < end; base += kEmbedThreads) {
            const int64_t p = base + lane;
            const bool inside = p < end;
            const uint32_t c = inside ? bytes[p] : 0u;
            uint32_t pending = 0u, bucket_w = 0u, bucket_t = 0u;   // bit 0: the word feature, bit 1: the trigram
            if (embed_is_word(c)) {
                const uint32_t before = p > begin ? bytes[p - 1] : 0u, behind = p + 1 < end ? bytes[p + 1] : 0u;
                const bool starts = !embed_is_word(before), ends = !embed_is_word(behind);
                uint32_t crc = crc32_byte(kCrcAfterT, starts ? (uint32_t)'^' : embed_low(before));
                crc = crc32_byte(crc, embed_low(c));
                crc = crc32_byte(crc, ends ? (uint32_t)'$' : embed_low(behind));
                bucket_t = (crc ^ 0xffffffffu) % udim;
                pending = 2u;
                if (starts) {
                    uint32_t wcrc = kCrcAfterW;
                    for (int64_t q = p; q < end; ++q) {
                        const uint32_t b = bytes[q];
                        if (!embed_is_word(b)) break;
                        wcrc = crc32_byte(wcrc, embed_low(b));
                    }
                    bucket_w = (wcrc ^ 0xffffffffu) % udim;
                    pending = 3u;
                }
            }
            const uint32_t f_w = 2u * (uint32_t)lane, f_t = f_w + 1u;
            const uint32_t tag_w = bucket_w % kEmbedTags, tag_t = bucket_t % kEmbedTags;
            for (;;) {
                __syncthreads();                       // (behind the previous round's adds and clears)
                if (!__any((int)pending)) break;       // (the workgroup is one wave: a wave vote is a workgroup vote)
                if (pending & 1u) atomicMin(&s_tag[tag_w], f_w);
                if (pending & 2u) atomicMin(&s_tag[tag_t], f_t);
                __syncthreads();
                const bool wins_w = (pending & 1u) && s_tag[tag_w] == f_w, wins_t = (pending & 2u) && s_tag[tag_t] == f_t;
                __syncthreads();
                // a winner is alone on its tag, so alone on its bucket; a lane that wins both holds two different buckets
                if (wins_w) {
                    s_acc[bucket_w] += 1.0f;
                    s_tag[tag_w] = kEmbedNoTag;
                    pending &= ~1u;
                }
                if (wins_t) {
                    s_acc[bucket_t] += tw;
                    s_tag[tag_t] = kEmbedNoTag;
                    pending &= ~2u;
                }
            }
        }
        __syncthreads();
        float* row = out + r * (int64_t)dim;
        for (int i = lane; i < dim; i += kEmbedThreads) row[i] = s_acc[i];
        __syncthreads();   // (the next text zeroes the accumulator)
    }
}

}  // namespace codd
