// where_eval.h — metadata filters on the device: a predicate program over per-key columns, as a row bitmap.
//
// A column holds, per row slot, a tag (0 absent, 1 bool, 2 number, 3 str) and a 64-bit cell: 0 / 1, the order-preserving key of a
// float64 (unsigned comparison of keys is numeric comparison: no floating-point operation happens here), or a dictionary code.
// A program (codd_knn_where_program, include/codd_knn.h) is a list of leaves — (column, tag class, kind, negate, literal range) —
// and a postfix expression over them: PUSH leaf, AND, OR.
//
// where_eval_kernel is a pure stream: 9 bytes per row and distinct column, each read once, coalesced.  The program travels by
// value as a kernel argument (2.9 KB with the column pointers) and is uniform across the lanes, so leaf dispatch, the literal
// scans and the postfix walk are scalar work and control flow never diverges.  A lane owns kWhereRows rows per step, 64 rows
// apart, so that a wave has kWhereRows loads per array in flight; a leaf's result is one bit of a 32-bit word per row, the postfix
// stack a 64-bit integer per row (push = shift in, AND / OR = combine the two low bits).  The verdicts leave through the 64-bit
// wave ballot: two lanes write the two words of each 64 rows after masking with the tombstones — every output word is written
// exactly once, so there is neither a memset nor an atomic.
//
// THE PROGRAM IS VALIDATED ON THE HOST (where_program_error below) before anything is launched: on the device every column, leaf
// and literal index is in bounds by construction and the stack neither underflows nor outgrows its 64 bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "codd_knn.h"
#include "wave_topk.h"

namespace codd {

constexpr int kWhereThreads = 256;
constexpr int kWhereRows = 4;                                           // rows per lane and step
constexpr int kWhereWaveRows = 64 * kWhereRows;                         // rows per wave and step
constexpr int kWhereBlockRows = kWhereWaveRows * (kWhereThreads / 64);  // rows per workgroup and step
constexpr int kWhereMaxStack = 32;                                      // postfix stack entries (one bit each of a 64-bit word)
static_assert(CODD_KNN_WHERE_MAX_LEAVES <= 32, "a row's leaf results are the bits of one 32-bit word");
static_assert(CODD_KNN_WHERE_MAX_LEAVES <= CODD_KNN_WHERE_AND, "an operator below CODD_KNN_WHERE_AND pushes that leaf");

// what the kernel takes by value: the program and where each column lives
struct WhereArgs {
    codd_knn_where_program prog;
    const uint8_t* tags[CODD_KNN_MAX_COLUMNS];
    const uint64_t* cells[CODD_KNN_MAX_COLUMNS];
};
static_assert(sizeof(WhereArgs) <= 3072, "the program travels in the kernel's argument segment");

// null, or why `p` cannot run: the host check of codd_knn_eval_where (everything but "the column has been set")
inline const char* where_program_error(const codd_knn_where_program* p) {
    if (!p) return "eval_where: null program%s";
    if (p->nleaves < 1 || p->nleaves > CODD_KNN_WHERE_MAX_LEAVES) return "eval_where: nleaves out of range [1,32]%s";
    if (p->nliterals < 0 || p->nliterals > CODD_KNN_WHERE_MAX_LITERALS) return "eval_where: nliterals out of range [0,256]%s";
    if (p->nops < 1 || p->nops > CODD_KNN_WHERE_MAX_OPS) return "eval_where: nops out of range [1,64]%s";
    for (int i = 0; i < p->nleaves; ++i) {
        const codd_knn_where_leaf& l = p->leaves[i];
        if (l.column >= CODD_KNN_MAX_COLUMNS) return "eval_where: a leaf's column is not below CODD_KNN_MAX_COLUMNS%s";
        if (l.tag < CODD_KNN_WHERE_TAG_BOOL || l.tag > CODD_KNN_WHERE_TAG_STR) return "eval_where: a leaf's tag class is none of bool, number, str%s";
        if (l.kind > CODD_KNN_WHERE_GE) return "eval_where: unknown leaf kind%s";
        if (l.negate > 1) return "eval_where: negate must be 0 or 1%s";
        if ((int)l.lit_first + (int)l.lit_count > p->nliterals) return "eval_where: a leaf's literal range leaves the literals%s";
        if (l.kind != CODD_KNN_WHERE_IN && (l.tag != CODD_KNN_WHERE_TAG_NUMBER || l.lit_count != 1))
            return "eval_where: a comparison leaf is on class number with exactly one literal%s";
    }
    int depth = 0;
    for (int i = 0; i < p->nops; ++i) {
        const uint8_t op = p->ops[i];
        if (op == CODD_KNN_WHERE_AND || op == CODD_KNN_WHERE_OR) {
            if (depth < 2) return "eval_where: the postfix program underflows its stack%s";
            --depth;
        } else {
            if (op >= p->nleaves) return "eval_where: a postfix operator pushes a leaf the program does not have%s";
            if (++depth > kWhereMaxStack) return "eval_where: the postfix program needs more than 32 stack entries%s";
        }
    }
    if (depth != 1) return "eval_where: the postfix program must leave exactly one value%s";
    return nullptr;
}

// grid: any number of workgroups (grid-stride over steps of kWhereBlockRows rows).  bits: ceil(n / 32) words, each written once.
// dead: the tombstone bits, null = none.  Every column the program names holds at least n slots.
__global__ __launch_bounds__(kWhereThreads) void where_eval_kernel(WhereArgs a, const uint32_t* __restrict__ dead, int64_t n, int64_t nwords,
                                                                   uint32_t* __restrict__ bits) {
    const int lane = lane_id();
    const int64_t steps = (n + kWhereWaveRows - 1) / kWhereWaveRows;
    const int nleaves = a.prog.nleaves, nops = a.prog.nops;
    for (int64_t s = (int64_t)blockIdx.x * (kWhereThreads / 64) + (threadIdx.x >> 6); s < steps; s += (int64_t)gridDim.x * (kWhereThreads / 64)) {
        const int64_t base = s * kWhereWaveRows + lane;   // this lane's rows: base + 64 j
        uint32_t tag[kWhereRows], leaf_bits[kWhereRows];
        u64 cell[kWhereRows];
#pragma unroll
        for (int j = 0; j < kWhereRows; ++j) { tag[j] = 0u; cell[j] = 0ull; leaf_bits[j] = 0u; }
        int loaded = -1;   // the column tag[] and cell[] hold: leaves of one column in a row share its loads
        for (int i = 0; i < nleaves; ++i) {
            const codd_knn_where_leaf leaf = a.prog.leaves[i];
            if ((int)leaf.column != loaded) {
                loaded = (int)leaf.column;
                const uint8_t* __restrict__ col_tags = a.tags[loaded];
                const uint64_t* __restrict__ col_cells = a.cells[loaded];
#pragma unroll
                for (int j = 0; j < kWhereRows; ++j) {
                    const int64_t r = base + 64 * j;
                    tag[j] = r < n ? (uint32_t)col_tags[r] : 0u;
                    cell[j] = r < n ? (u64)col_cells[r] : 0ull;
                }
            }
            bool hit[kWhereRows];
            if (leaf.kind == CODD_KNN_WHERE_IN) {
#pragma unroll
                for (int j = 0; j < kWhereRows; ++j) hit[j] = false;
                for (int l = 0; l < (int)leaf.lit_count; ++l) {
                    const u64 lit = a.prog.literals[(int)leaf.lit_first + l];
#pragma unroll
                    for (int j = 0; j < kWhereRows; ++j) hit[j] = hit[j] || cell[j] == lit;
                }
            } else {
                const u64 lit = a.prog.literals[leaf.lit_first];
#pragma unroll
                for (int j = 0; j < kWhereRows; ++j)
                    hit[j] = leaf.kind == CODD_KNN_WHERE_LT ? cell[j] < lit : leaf.kind == CODD_KNN_WHERE_LE ? cell[j] <= lit
                           : leaf.kind == CODD_KNN_WHERE_GT ? cell[j] > lit : cell[j] >= lit;
            }
#pragma unroll
            for (int j = 0; j < kWhereRows; ++j) {
                const bool pass = (tag[j] == (uint32_t)leaf.tag && hit[j]) != (leaf.negate != 0);
                leaf_bits[j] |= (pass ? 1u : 0u) << i;
            }
        }
        u64 stack[kWhereRows];
#pragma unroll
        for (int j = 0; j < kWhereRows; ++j) stack[j] = 0ull;
        for (int p = 0; p < nops; ++p) {
            const uint32_t op = a.prog.ops[p];
#pragma unroll
            for (int j = 0; j < kWhereRows; ++j) {
                if (op < CODD_KNN_WHERE_AND) stack[j] = (stack[j] << 1) | (u64)((leaf_bits[j] >> op) & 1u);
                else {
                    const u64 top = stack[j] & 1ull;
                    stack[j] >>= 1;
                    stack[j] = op == CODD_KNN_WHERE_AND ? stack[j] & (top | ~1ull) : stack[j] | top;
                }
            }
        }
#pragma unroll
        for (int j = 0; j < kWhereRows; ++j) {
            const u64 verdicts = __ballot((stack[j] & 1ull) != 0ull && base + 64 * j < n);
            const int64_t w = (s * kWhereWaveRows + 64 * j) / 32 + lane;   // lanes 0 and 1 write the two words of these 64 rows
            if (lane < 2 && w < nwords) bits[w] = (uint32_t)(verdicts >> (32 * lane)) & ~(dead ? dead[w] : 0u);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// Column maintenance.  column_set_kernel writes n (slot, tag, cell) triples (distinct slots); column_compact_kernel moves a
// column with the rows of codd_knn_compact: the live row r at or above `first` goes to its rank among the live rows (the
// prefix sums live_prefix_kernel left), out of place into a zero-filled copy.
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void column_set_kernel(const int64_t* __restrict__ slots, const uint8_t* __restrict__ tags,
                                                         const uint64_t* __restrict__ cells, int64_t n, uint8_t* __restrict__ col_tags,
                                                         uint64_t* __restrict__ col_cells) {
    const int64_t i = (int64_t)blockIdx.x * 256 + (int64_t)threadIdx.x;
    if (i >= n) return;
    col_tags[slots[i]] = tags[i];
    col_cells[slots[i]] = cells[i];
}

__global__ __launch_bounds__(256) void column_compact_kernel(const uint32_t* __restrict__ dead, int64_t n, const unsigned* __restrict__ prefix,
                                                             const unsigned* __restrict__ block_base, int64_t first,
                                                             const uint8_t* __restrict__ tags_in, const uint64_t* __restrict__ cells_in,
                                                             uint8_t* __restrict__ tags_out, uint64_t* __restrict__ cells_out) {
    const int64_t r = first + (int64_t)blockIdx.x * 256 + (int64_t)threadIdx.x;
    if (r >= n || row_dead(dead, (uint32_t)r)) return;
    const int64_t w = r >> 5;
    const int64_t left = n - w * 32;
    const uint32_t live = ~dead[w] & (left >= 32 ? 0xffffffffu : (1u << (uint32_t)left) - 1u);
    const int64_t to = (int64_t)block_base[w >> 8] + prefix[w] + __popc(live & ((1u << (uint32_t)(r & 31)) - 1u));
    if (to > r) return;   // (cannot happen: rows only move down)
    tags_out[to] = tags_in[r];
    cells_out[to] = cells_in[r];
}

}  // namespace codd
