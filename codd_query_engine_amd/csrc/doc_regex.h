// doc_regex.h — a byte DFA run over every document of the arena: which documents a regular expression matches,
// as a row bitmap.  The table comes from codd_query_engine_amd/regex_dfa.py, whose ByteDfa.matches is this kernel on the CPU.
//
// A substring test is position-parallel (doc_match.h); a DFA carries a state along each document, so doc_regex_kernel is
// DOCUMENT-parallel: one lane per document, a workgroup per run of kRegexDocs consecutive documents.  Their bytes are one
// contiguous arena range, offsets[r0] .. offsets[r0 + n), separators included.  It comes into LDS kRegexTile bytes at a time with
// 16-byte loads from a 16-byte aligned base, the class map and the table sit beside it, and each lane walks the intersection of
// its document with the segment — a word of the segment per LDS read, then per byte the class and the table entry — and carries
// its state to the next segment.  A lane whose state is absorbing (the match is made, or can no longer be made) stops reading; a
// workgroup none of whose lanes still reads stops loading.  The separator is the document's last symbol: state after it ==
// accept <=> the document matches.
//
// The result is a wave ballot: 64 documents are two words, every word of the bitmap is written exactly once, by one lane.  No
// atomic, no memset, no search for the document of a position: the last match of a frequent pattern costs what the first does.
//
// Bounds: every loop runs over [offsets[r], offsets[r + 1]), which codd_knn_set_documents_host validated as monotone and inside
// the arena; a staged piece starts below offsets[r0 + n] <= the arena's bytes, and the allocation is a multiple of 16.  A table
// entry never leads outside the table: codd_knn_match_documents_dfa checks every entry on the host before it uploads.  No
// workgroup waits for another.  A document of many megabytes is walked by one lane, its workgroup loading segment after segment:
// slow and correct.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace codd {

constexpr int kRegexTile = 8192;           // arena bytes per segment ("doc_regex_tile_bytes")
constexpr int kRegexDocs = 256;            // documents per workgroup, one per lane ("doc_regex_run_docs")
constexpr int kRegexMaxStates = 255;       // == CODD_KNN_MAX_DFA_STATES
constexpr int kRegexMaxTable = 8192;       // == CODD_KNN_MAX_DFA_TABLE: bytes of next[nstates][nclasses]
constexpr int kRegexClassWords = 256 / 4;  // the class map in front of the table, in the device buffer and in LDS
constexpr int kRegexTableWords = kRegexClassWords + kRegexMaxTable / 4;
static_assert(kRegexTile % 16 == 0 && kRegexDocs % 64 == 0, "segment and ballot shape");
// (8,192 + 8,448 bytes of LDS: eight workgroups per compute unit, eight waves per SIMD)

// grid: ceil(count / kRegexDocs) workgroups of kRegexDocs threads.  table: [kRegexClassWords] class_of, then next[], zero padded to a
// word; table_words: how many of next[]'s.  reject: an absorbing state other than accept, or -1.
__global__ __launch_bounds__(kRegexDocs) void doc_regex_kernel(const uint4* __restrict__ arena, const int64_t* __restrict__ offsets, int64_t count,
                                                               const uint32_t* __restrict__ table, int table_words, int nclasses, int start,
                                                               int accept, int reject, uint32_t* __restrict__ bits, int64_t nwords) {
    __shared__ uint4 s_tile[kRegexTile / 16];
    __shared__ uint32_t s_table[kRegexTableWords];
    const int tid = (int)threadIdx.x;
    for (int i = tid; i < kRegexClassWords + table_words; i += kRegexDocs) s_table[i] = table[i];
    const uint8_t* class_of = reinterpret_cast<const uint8_t*>(s_table);
    const uint8_t* next = class_of + 256;
    const uint32_t* tile_words = reinterpret_cast<const uint32_t*>(s_tile);

    const int64_t r0 = (int64_t)blockIdx.x * kRegexDocs, r = r0 + tid;
    const int64_t r1 = r0 + kRegexDocs < count ? r0 + kRegexDocs : count;
    const int64_t run_begin = offsets[r0], run_end = offsets[r1];
    const bool mine = r < count;
    int64_t pos = mine ? offsets[r] : run_end;          // the next byte of this lane's document
    const int64_t end = mine ? offsets[r + 1] : run_end;   // one past its separator
    uint32_t state = (uint32_t)start;
    bool reading = mine && state != (uint32_t)accept && state != (uint32_t)reject;

    for (int64_t seg = run_begin & ~(int64_t)15; seg < run_end; seg += kRegexTile) {
        if (!__syncthreads_or(reading ? 1 : 0)) break;   // (also: the previous segment's readers are done; the table is in LDS)
        const uint4* src = arena + seg / 16;
        const int64_t left = (run_end - seg + 15) / 16;
        const int pieces = left < kRegexTile / 16 ? (int)left : kRegexTile / 16;
        for (int i = tid; i < pieces; i += kRegexDocs) s_tile[i] = src[i];
        __syncthreads();
        const int64_t stop = end < seg + kRegexTile ? end : seg + kRegexTile;
        if (reading && pos < stop) {   // (pos >= seg: the segments cover the run in order)
            const int p = (int)(pos - seg), h = (int)(stop - seg);
            for (int w = p & ~3; w < h && reading; w += 4) {
                const uint32_t word = tile_words[w >> 2];
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const int at = w + b;
                    if (at >= p && at < h && reading) {
                        state = next[state * (uint32_t)nclasses + class_of[(word >> (8 * b)) & 0xffu]];
                        reading = state != (uint32_t)accept && state != (uint32_t)reject;
                    }
                }
            }
            pos = stop;
            if (pos >= end) reading = false;
        }
    }
    const unsigned long long matched = __ballot(mine && state == (uint32_t)accept);
    if ((tid & 63) == 0) {
        const int64_t w = r >> 5;
        if (w < nwords) bits[w] = (uint32_t)matched;
        if (w + 1 < nwords) bits[w + 1] = (uint32_t)(matched >> 32);
    }
}

}  // namespace codd
