// search_plan.h — which kernels answer a search, decided once and in one place: pure functions of the index's shape, its option
// knobs and the batch.  No HIP, no heap: plain C++17 (tests/host/search_plan_main.cpp compiles it alone with a host compiler), and
// cheap enough for the single-query latency path.  codd_knn.hip holds one FilterKnobs and one FilterWatch per index, fills an
// IndexShape per call (shape_of) and launches what plan_search() and filter_program() name; nothing in here reads the index.
#pragma once
#include <stdint.h>
#include <string.h>

#include "codd_knn.h"
#include "geometry.h"

namespace codd {

// The option-settable integers of the search paths (codd_knn_set_option; kKnobTable below has the names and bounds of most)
struct FilterKnobs {
    int scan_blocks_per_cu = 4;  // the exact scan's grid: workgroups per compute unit, at most
    int filter_enabled = 1;
    int64_t filter_min_rows = 1;             // batches >= filter_min_batch: only the tile-count condition applies
    int64_t filter_min_rows_small = 100000;  // batches below filter_min_batch: filter when rows * B reaches this
    int filter_min_batch = 9;
    int sample_tiles = 4096;  // upper bound on sampled tiles (reached from 42M rows on)
    int sample_div = 40;      // sample about 1/40 of the tiles (2.5 % extra GEMM work), see sample_tile_count()
    int hit_cap_q = 131072;  // candidates kept per query before it falls back to the exact scan (256 MiB per searching stream at 256 queries:
                             // a cluster of 60,000 near-identical rows — closer to each other than either filter's slack — stays on the filter path)
    // int8 shadow for small batches (optional; rebuilt lazily from the stored rows when they have changed)
    int shadow8_enabled = 1;
    int shadow8_max_batch = 256;  // batches up to this size (one query pass) take the int8 filter
    int resident_q = 1;           // rows of <= 512 int8 elements: the query block stays in LDS ("resident_q" option)
    int i8v2 = 2;                 // batches of 65..256 queries on rows of >= 384 elements (3 K-steps) take i8_tile_kernel (filter_i8.h); 1: only rows of
                                  // more than 512 elements (below, the first-generation kernel keeps the query block resident in LDS: 6-12 % slower); 0: never
    int i8v2_half = 1;            // ... and so do batches of 65..128 queries (its 8-query-block instantiation)
    int fuse_fallback = 1;        // k <= 64, one finalize workgroup per query (the 2-byte passes; int8 passes above 64 queries): finalize and the exact-scan
                                  // fallback in one launch ("fuse_fallback": 0 = two launches)
    int small_batch_max = 0;      // 1: a single query is answered in one launch by small_batch_kernel where it applies.  OFF by default: measured SLOWER than the
                                  // six-launch chain (1M x 768, B = 1: kernel 0.27 ms, p50 0.33 ms against 0.25 ms; profiles/r3/small_batch_latency.txt)
    int per_block = 7;            // the int8 bound per 32-row block: bit 0 in i8_tile_kernel, bit 1 in finalize ("per_block" option; 0 = the device-wide bound everywhere;
                                  // bit 2 chose between block metadata and per-row scales in the tile kernel's filter pass until the per-row path was removed: ignored)
    int i8_pair = 2;              // rows of 6, 12, ... K-steps: the staged tile program with one workgroup barrier per two K-steps ("i8_pair" option: 0 = one per K-step;
                                  // 2 = ... and rows of exactly 6 K-steps its static form, i8_tile_kernel<., 3, ., false>)
    int sample_div8 = 28;         // its thresholds come from a larger sample (the int8 slack is ~5x the bf16 one)
    int sample_rounds8 = 2;       // ... of at least this many rounds of workgroups (one tile each) when the batch has more than 32 queries (3 until the round-3 epilogue:
                                  // at 1.25M rows two rounds trade 13 us of sample for 7 us of filter, gpurun_out/r3n/ab_sample_1p25m.txt)
    // the int8 filter leg of an ip or l2 index ("space_filter" option, off by default)
    int space_filter = 0;
    int f16_tile = 1;             // the 2-byte filter of 129..256 queries over rows of 6, 12, ... 64-element K-steps (768 elements: 12) runs the tile program of
                                  // filter_i8.h on fp16 operands ("f16_tile" option; 0 = gemm_filter_kernel)
    float shadow8_max_eps = 0.04f;  // a worst row error norm above this: the index keeps the 2-byte filter (plan_search: eps_ok)
    int shadow8_max_surv = 4000;    // FilterWatch: survivors per query above which the int8 passes start a cooldown ...
    int shadow8_cooldown = 256;     // ... of this many searches
    int ivf_share = 1;            // IVF search: from 1,024 (query, list) pairs on, a probed list is scanned once for all its queries ("ivf_share": 0 = per pair)
    // IVF on an ip or l2 index ("space_ivf" option, off by default): the coarse index in the index's own space, raw
    // centroids, the list scans by the index's metric.  No effect on a cosine index.
    int space_ivf = 0;
    // masked search
    int mask_route = 0;        // "mask_route": 0 = by the routing rule, 1 = always the list route, 2 = always the dense route
    int mask_list_pct = 100;   // "mask_list_pct": the list route's side of the cost comparison, in percent (100 = the derived rule)
    // the sample cascade (cascade_plan below).  Plain integers in a range like the rows of kKnobTable, but not rows of it:
    // tests/test_search_plan.py pins that table's length and feeds every row to its host program, so codd_knn_set_option checks these itself
    int sample_cascade = 1;        // "sample_cascade": 0 = off, 1 = where today's sample has cascade_min_rounds rounds of workgroups, 2 = wherever it applies
    int cascade_d = 16;            // "cascade_d": the stage that fixes the thresholds scans every (d + 1)-th tile; d is the divisor of the grid in [16, 64] nearest this
    int cascade_min_rounds = 3;    // "cascade_min_rounds": the size rule of sample_cascade = 1 (3 rounds: from ~5M rows of 768 elements on 256 compute units)
    // the sweep form of the static int8 tile program (checked by codd_knn_set_option like the cascade's)
    int i8_sweep = 1;              // "i8_sweep": 1 = 129..256 queries on rows of exactly 6 K-steps run i8_sweep_kernel (two query slices staged per tile); 0 = i8_tile_kernel<., 3> (six)
};

// the options that are "an integer in [lo, hi], stored into one knob"; `message` is the whole fail() format of a value outside
struct KnobRow {
    const char* name;
    int FilterKnobs::*knob;
    int64_t lo, hi;
    const char* message;
};
constexpr KnobRow kKnobTable[] = {
    {"scan_blocks_per_cu", &FilterKnobs::scan_blocks_per_cu, 1, 8, "scan_blocks_per_cu must be in [1,8]%s"},
    {"shadow8", &FilterKnobs::shadow8_enabled, 0, 1, "shadow8 must be 0 or 1%s"},
    {"space_filter", &FilterKnobs::space_filter, 0, 1, "space_filter must be 0 or 1%s"},
    {"shadow8_max_batch", &FilterKnobs::shadow8_max_batch, 1, 256, "shadow8_max_batch must be in [1,256]%s"},
    {"shadow8_max_surv", &FilterKnobs::shadow8_max_surv, 1, 1000000, "shadow8_max_surv must be in [1,1000000]%s"},
    {"shadow8_cooldown", &FilterKnobs::shadow8_cooldown, 0, 1000000, "shadow8_cooldown must be in [0,1000000]%s"},
    {"i8v2", &FilterKnobs::i8v2, 0, 2, "i8v2 must be 0, 1 or 2%s"},
    {"space_ivf", &FilterKnobs::space_ivf, 0, 1, "space_ivf must be 0 or 1%s"},
    {"f16_tile", &FilterKnobs::f16_tile, 0, 1, "f16_tile must be 0 or 1%s"},
    {"ivf_share", &FilterKnobs::ivf_share, 0, 1, "ivf_share must be 0 or 1%s"},
    {"fuse_fallback", &FilterKnobs::fuse_fallback, 0, 1, "fuse_fallback must be 0 or 1%s"},
    {"small_batch_max", &FilterKnobs::small_batch_max, 0, 1, "small_batch_max must be 0 or 1%s"},
    {"per_block", &FilterKnobs::per_block, 0, 7, "per_block must be in [0,7]%s"},
    {"i8_pair", &FilterKnobs::i8_pair, 0, 2, "i8_pair must be 0, 1 or 2%s"},
    {"i8v2_half", &FilterKnobs::i8v2_half, 0, 1, "i8v2_half must be 0 or 1%s"},
    {"resident_q", &FilterKnobs::resident_q, 0, 1, "resident_q must be 0 or 1%s"},
    {"sample_rounds8", &FilterKnobs::sample_rounds8, 1, 16, "sample_rounds8 must be in [1,16]%s"},
    {"sample_div8", &FilterKnobs::sample_div8, 1, 1000, "sample_div8 must be in [1,1000]%s"},
    {"sample_tiles", &FilterKnobs::sample_tiles, 1, 65536, "sample_tiles must be in [1,65536]%s"},
    {"sample_div", &FilterKnobs::sample_div, 1, 4096, "sample_div must be in [1,4096]%s"},
    {"mask_route", &FilterKnobs::mask_route, 0, 2, "mask_route must be 0 (auto), 1 (list) or 2 (dense)%s"},
    {"mask_list_pct", &FilterKnobs::mask_list_pct, 0, 100000, "mask_list_pct must be in [0,100000]%s"},
    {"hit_cap", &FilterKnobs::hit_cap_q, 16, 1 << 20, "hit_cap must be in [16,2^20]%s"},
};
// the table's row for `key`, or null
inline const KnobRow* find_knob(const char* key) {
    for (const KnobRow& row : kKnobTable)
        if (strcmp(key, row.name) == 0) return &row;
    return nullptr;
}
// stores a value inside [lo, hi] and returns null; outside, changes nothing and returns the row's message
inline const char* set_knob(FilterKnobs& kn, const KnobRow& row, int64_t value) {
    if (value < row.lo || value > row.hi) return row.message;
    kn.*row.knob = (int)value;
    return nullptr;
}

// what the route rules need to know of an index (codd_knn.hip: shape_of)
struct IndexShape {
    int64_t count = 0;
    int dim = 0, dpad = 0, dtype = 0, metric = 0, num_cus = 256;
    bool all_normalized = true;
};

inline bool metric_is_cosine(const IndexShape& s) { return s.metric == CODD_KNN_METRIC_COSINE; }
inline size_t elem_size(int dtype) { return dtype == DT_F32 ? 4 : 2; }
inline int elems_per_chunk(int dtype) { return dtype == DT_F32 ? 4 : 8; }
// chunks of the padded row per lane: the NITER of the exact-score row kernels
inline int niter_of(const IndexShape& s) { return (s.dpad / elems_per_chunk(s.dtype) + kWave - 1) / kWave; }
inline int dpad8_of(const IndexShape& s) { return (s.dpad + 127) / 128 * 128; }
// 256-row tiles of `count` rows
inline int64_t tiles_of(int64_t count) { return (count + kTileRows - 1) / kTileRows; }
// 32-query blocks a filter pass of nq <= 256 queries multiplies: 1, 2, 4 or 8
inline int nbq_of(int nq) { return nq <= 32 ? 1 : (nq <= 64 ? 2 : (nq <= 128 ? 4 : 8)); }
// may a batch of B queries take the int8 filter?  Every pass of <= 256 queries prepares its own block (a batch above 256 queries is
// several passes)
inline bool int8_batch_ok(const FilterKnobs& kn, int B) {
    return kn.shadow8_enabled && CODD_MFMA16 && (B <= kn.shadow8_max_batch || (B > kTileQ && kn.shadow8_max_batch >= kTileQ));
}
// workgroups per query of a pass's finalize: the int8 filter leaves thousands of survivors per query and is only used for a handful
// of queries, so each query's re-scoring is shared out between several workgroups, whose lists are merged
inline int finalize_parts(bool use8, int nq) { return use8 ? (nq <= 8 ? 16 : (nq <= 32 ? 8 : (nq <= 64 ? 4 : 1))) : 1; }

// how many evenly spaced tiles set the thresholds: ~ntiles/sample_div (so the sample costs a fixed
// fraction of the main pass at every shard size and the hit volume per query stays ~k*sample_div),
// at least max(64, 4k) where the corpus has that many tiles, at most sample_tiles
inline int64_t sample_tile_count(const FilterKnobs& kn, const IndexShape& s, int64_t ntiles, int k, bool use8 = false, int nbq = 8) {
    int64_t ts = ntiles / (use8 ? (nbq == 1 ? 2 * kn.sample_div8 : kn.sample_div8) : kn.sample_div);
    if (use8) {
        // the int8 filter pays more per hit (wider slack, more of them) and less per sampled tile: "sample_rounds8" rounds of
        // workgroups (2 since round 3's cheaper epilogue; 3 before) where that is still under a quarter of the corpus
        // (1/10 of a 1.25M-row shard, 1/28 of 10M rows; twice as sparse for <= 32 queries, whose sample is a pure byte stream)
        const int64_t rounds = (nbq == 1 ? 1 : kn.sample_rounds8) * (int64_t)s.num_cus;
        const int64_t floor8 = rounds < ntiles / 4 ? rounds : ntiles / 4;
        if (ts < floor8) ts = floor8;
    }
    const int64_t lo = 4 * (int64_t)k > 64 ? 4 * (int64_t)k : 64;
    if (ts < lo) ts = lo;
    // a sample of fewer tiles than there are CUs takes as long as one full round of workgroups (one tile each), and a
    // bigger sample means a tighter threshold: fewer hits for the filter's epilogue (scripts/rows_sweep.py)
    if (ts < s.num_cus && ntiles >= 2 * (int64_t)s.num_cus) ts = s.num_cus;
    // whole rounds of workgroups: the last round costs a round whether it is full or not
    if (ts > s.num_cus) ts = (ts + s.num_cus - 1) / s.num_cus * s.num_cus;
    if (ts > kn.sample_tiles) ts = kn.sample_tiles;
    if (ts > ntiles) ts = ntiles;
    return ts < 1 ? 1 : ts;
}

// The program a filter pass runs, chosen once per pass (filter_program); its sample launch and its filter launch both read it.
//   GEMM      gemm_filter_kernel<MODE, nbq, el, res>: el = 1 int8 operands; res = 1 the whole int8 query block resident in LDS,
//             res = 2 two of its six slices (768 elements, 4 query blocks)
//   TILE      i8_tile_kernel<MODE, ts, 2 * nbq, res> (filter_i8.h: the int8 tile program, 16-query blocks; res: the query block
//             resident in LDS); the sample pass runs ts = 0.  sweep: the filter launches of ts = 3, nbq = 8 run i8_sweep_kernel<16>
//             instead, the same program walking K back and forth
//   TILE_F16  i8_tile_kernel<MODE_FILTER, ts, 16, false, true>: the same program on fp16 operands; the sample pass is GEMM's
//             gemm_filter_kernel<MODE_SAMPLE, 8>
struct FilterProgram {
    enum Family { GEMM, TILE, TILE_F16 };
    Family family = GEMM;
    int nbq = 8;  // 32-query blocks the GEMM multiplies
    int ts = 0, res = 0, el = 0;
    bool sqd = false;  // sqd_filter_kernel<MODE, nbq>: the squared-distance epilogue of an l2 index
    bool sweep = false;
};

inline FilterProgram filter_program(const FilterKnobs& kn, const IndexShape& s, int nq, int nsteps, bool use8) {
    FilterProgram p;
    p.nbq = nbq_of(nq);
    p.el = use8 ? 1 : 0;
    // an ip or l2 index: the GEMM family on int8 operands whatever "i8v2" / "f16_tile" say — the tile programs evaluate
    // the per-block, unit-norm form of the bound — and for l2 its staged form with the squared-distance epilogue
    const bool space = !metric_is_cosine(s);
    p.sqd = space && s.metric == CODD_KNN_METRIC_L2;
    const bool resident = use8 && nsteps <= 4 && kn.resident_q && !p.sqd;
    // 65..128 queries only: with <= 64 the kernel is a byte stream (nothing to gain); with 8 query blocks the six-step body
    // needs more than the 256 registers of a wave (hipcc spills, no gain measured)
    const bool partial6 = use8 && nsteps == 6 && nq > 64 && nq <= 128 && kn.resident_q && !p.sqd;
    // full query blocks: the second-generation int8 kernel (filter_i8.h); rows whose query block fits the LDS keep the resident one
    const bool tile_v2 = !space && use8 && (p.nbq == 8 || (p.nbq == 4 && kn.i8v2_half)) && ((kn.i8v2 == 1 && !resident && nsteps >= 3) || (kn.i8v2 == 2 && nsteps >= 3));
    // the 2-byte filter (dense clusters the int8 slack cannot separate, the int8 filter switched off): the same tile program on fp16 operands
    const bool tile_f16 = !space && CODD_SHADOW_F16 && CODD_MFMA16 && !use8 && p.nbq == 8 && nsteps % 6 == 0 && kn.f16_tile;
    if (tile_f16) {
        p.family = FilterProgram::TILE_F16;
        // rows of 768 elements are 12 K-steps of 64, rows of 384 are 6: the static forms of the tile program ("i8_pair" = 2); 18, 24, ...: run-time cursors
        if (nsteps == 12 && kn.i8_pair == 2) p.ts = 4;
        else if (nsteps == 6 && kn.i8_pair == 2) p.ts = 3;
        else p.ts = 2;
    } else if (tile_v2) {
        p.family = FilterProgram::TILE;
        p.res = i8_tile_resident(nsteps, p.nbq) && kn.resident_q;  // the query block fits the four LDS slices: loaded once per workgroup
        // tile structure: rows of 6, 12, ... K-steps (768 elements: the headline shape) run the staged program with one barrier
        // per TWO K-steps; other multiples of 3 one per K-step; the rest the generic interval loop
        // ("i8_pair" = 2, the default: rows of exactly 6 K-steps take that program with every cursor a compile-time constant)
        const bool pair = nsteps % 6 == 0 && kn.i8_pair;
        const bool static6 = nsteps == 6 && kn.i8_pair == 2;
        if (p.res) p.ts = nsteps % 3 == 0 ? 1 : 0;
        else if (static6) p.ts = 3;
        else if (pair) p.ts = 2;
        else p.ts = nsteps % 3 == 0 ? 1 : 0;
        p.sweep = p.ts == 3 && p.nbq == 8 && !p.res && kn.i8_sweep != 0;
    } else if (partial6) {  // 768 int8 elements: two of the six query slices stay in LDS
        p.res = 2;
    } else if (resident) {  // the whole int8 query block fits the LDS slices: loaded once per workgroup
        p.res = 1;
    }
    return p;
}

// ---- the sample cascade ------------------------------------------------------------------------------------
// A pass of the static int8 tile program fixes its thresholds in two steps instead of one, so that the tiles the thresholds come
// from are scanned ONCE, by the filter program, and not a second time by the main launch:
//   A0   the sample program over a0_tiles tiles a0_first + u a0_stride: one round of workgroups; anchor_thr_kernel turns its keys
//        into sound provisional thresholds
//   A1   the filter program over tiles 0, d + 1, 2 (d + 1), ... with those thresholds: candidates straight into the hit lists;
//        reanchor_thr_kernel then tightens the thresholds on (A1's candidates U A0's keys)
//   B    the filter program over every OTHER tile, G workgroups: workgroup u owns tiles cascade_b_first(u) + j b_step — the
//        (u + j G)-th tile that is no multiple of d + 1, which is u + j G + 1 + (u + j G) / d = first(u) + j (G + G / d) when d divides G
// No A0 tile is a multiple of d + 1: a0_first = 1 and a0_stride is a multiple of the smallest prime factor of d + 1, so every A0
// tile is 1 modulo that factor.  (A0's rows and A1's must differ: the re-anchor takes k DISTINCT rows from their union.)
struct CascadePlan {
    bool on = false;
    int d = 0;        // A1 scans every (d + 1)-th tile
    int G = 0;        // workgroups of launch B (d divides G)
    int64_t a0_tiles = 0, a0_stride = 0, a0_first = 0;
    int64_t a1_tiles = 0;   // ceil(ntiles / (d + 1)) run-tiles of stride d + 1
    int64_t b_step = 0;     // G + G / d
};
constexpr int kCascadeDMin = 16, kCascadeDMax = 64;   // the useful range: A1 is 1/17 .. 1/65 of the rows
inline bool cascade_d_admissible(int G, int d) { return d >= kCascadeDMin && d <= kCascadeDMax && G > 0 && G % d == 0; }
// the admissible d nearest `want` (the smaller of two equally near); 0: the grid has no divisor in the range
inline int cascade_pick_d(int G, int want) {
    int best = 0;
    for (int d = kCascadeDMin; d <= kCascadeDMax; ++d) {
        if (!cascade_d_admissible(G, d)) continue;
        const int dist = d > want ? d - want : want - d, best_dist = best > want ? best - want : want - best;
        if (best == 0 || dist < best_dist) best = d;
    }
    return best;
}
inline int smallest_prime_factor(int v) {
    for (int p = 2; p * p <= v; ++p)
        if (v % p == 0) return p;
    return v;
}
// launch B's enumeration, as the tile programs derive it from (blockIdx, gridDim, d): first tile, and how many
inline int64_t cascade_b_first(const CascadePlan& c, int64_t u) { return skip_first<int64_t>(u, c.d); }
inline int64_t cascade_b_my_tiles(const CascadePlan& c, int64_t u, int64_t ntiles) {
    const int64_t first = cascade_b_first(c, u);
    return ntiles > first ? (ntiles - first + c.b_step - 1) / c.b_step : 0;
}
// the geometry for a given admissible d (no applicability test)
// a0_cap: the most tiles A0 may take (the sample's key buffer holds "sample_tiles" tiles per query; never more than one round)
inline CascadePlan cascade_geometry(int G, int d, int64_t ntiles, int64_t a0_cap) {
    CascadePlan c;
    c.d = d;
    c.G = G;
    c.b_step = skip_step<int64_t>(G, d);
    c.a1_tiles = (ntiles + d) / (d + 1);
    const int64_t g = smallest_prime_factor(d + 1);
    const int64_t most = ntiles < 2 ? 0 : (ntiles - 2) / g + 1;   // tiles 1, 1 + g, ... below ntiles (a single tile is A1's: no A0, no cascade)
    c.a0_first = 1;
    if (a0_cap > G) a0_cap = G;
    c.a0_tiles = most < a0_cap ? most : a0_cap;
    c.a0_stride = c.a0_tiles > 1 ? (ntiles - 2) / (c.a0_tiles - 1) / g * g : g;
    return c;
}
// ts_today: what sample_tile_count() gives this pass.  Applies to the static int8 tile program (prog.ts == 3) on a grid with an
// admissible d, where A0 holds 2k tiles (the condition filter_applies() puts on today's sample); "sample_cascade" = 1 adds the size
// rule (profiles/cascade/README.md: below it two more launches cost more than the second scan of the sample).
inline CascadePlan cascade_plan(const FilterKnobs& kn, const IndexShape& s, const FilterProgram& prog, int64_t ntiles, int k, int64_t ts_today) {
    CascadePlan off;
    if (kn.sample_cascade == 0 || prog.family != FilterProgram::TILE || prog.ts != 3 || prog.res || prog.sqd || !metric_is_cosine(s)) return off;
    const int d = cascade_pick_d(s.num_cus, kn.cascade_d);
    if (d == 0 || ntiles < 2) return off;
    CascadePlan c = cascade_geometry(s.num_cus, d, ntiles, kn.sample_tiles);   // (A0 obeys "sample_tiles" as the plain sample does: bucket_max is sized by it)
    if (c.a0_tiles < 2 * (int64_t)k) return off;
    if (kn.sample_cascade == 1 && ts_today < (int64_t)kn.cascade_min_rounds * s.num_cus) return off;
    c.on = true;
    return c;
}

inline bool filter_applies(const FilterKnobs& kn, const IndexShape& s, int B, int k) {
    // the thresholds come from the k-th largest of the sampled tile maxima: need comfortably more tiles than k
    const int64_t ts = sample_tile_count(kn, s, tiles_of(s.count), k);
    if (!(kn.filter_enabled && s.all_normalized) || ts < 2 * (int64_t)k) return false;
    // measured on MI355X (scripts/crossover.py, d = 768): with more than 8 queries the filter wins at every size
    // it is sound for; up to 8 queries the exact scan's single launch wins until rows * B reaches ~100k
    if (B >= kn.filter_min_batch) return s.count >= kn.filter_min_rows;
    return s.count * (int64_t)B >= kn.filter_min_rows_small;
}

// The int8 filter leg of an ip or l2 index: opt-in ("space_filter"), batches of filter_min_batch queries and more
// over filter_min_rows rows and more whose sample holds 2k tiles, both "filter" and "shadow8" on, a build with the int8 MFMA.
// l2 rows wider than 4 chunks per lane stay on the scan.  No usefulness heuristic: a loose bound is slow, never wrong.
inline bool space_filter_applies(const FilterKnobs& kn, const IndexShape& s, int B, int k) {
    if (metric_is_cosine(s) || !kn.space_filter || !CODD_MFMA16 || !kn.filter_enabled || !kn.shadow8_enabled) return false;
    if (s.metric == CODD_KNN_METRIC_L2 && niter_of(s) > 4) return false;
    if (sample_tile_count(kn, s, tiles_of(s.count), k) < 2 * (int64_t)k) return false;
    return B >= kn.filter_min_batch && s.count >= kn.filter_min_rows;
}

// a single query in ONE launch (small_batch_kernel) instead of the filter chain
inline bool small_batch_applies(const FilterKnobs& kn, const IndexShape& s, int B, int k) {
    const int ns = dpad8_of(s) / 128;
    return kn.small_batch_max > 0 && B == 1 && k <= kWave && (ns == 3 || ns == 4 || ns == 6 || ns == 8) && s.count >= 4096;
}

// The route of one search and what its launches need to know, decided before anything is allocated or enqueued.
struct SearchPlan {
    enum Route {
        EMPTY,         // nothing stored: an all-empty answer
        SPACE_FILTER,  // an ip or l2 index's int8 filter leg (space_filter_search)
        EXACT_SCAN,    // one scan of the row store
        SMALL_BATCH,   // one query, one launch of small_batch_kernel over the int8 shadow
        FILTER,        // ceil(B / 256) filter passes
    };
    Route route = EXACT_SCAN;
    bool use8 = false;        // the filter passes run on the int8 shadow (else on the 2-byte one)
    bool can8 = false;        // ... or could: the batch and the options allow it; a cooldown or badly quantised rows keep the 2-byte filter
    bool per_block = false;   // an int8 pass of this batch would run the tile program, whose bound is per 32-row block
    bool fused_prep = false;  // one pass of 2-byte operands: prep_queries_kernel normalises, writes the fragments and clears the control block
    bool small_batch = false; // small_batch_applies(): the route of a search that takes the int8 shadow

    bool filters() const { return route == FILTER || route == SMALL_BATCH; }
    // The 2-byte shadow cannot be allocated: the search is still answered exactly — through the int8 filter where the index may
    // use it (a cooldown or a wide eps_r only make that one slower), else by the exact scan.
    void without_shadow16() {
        if (can8) {
            use8 = true;
            route = small_batch ? SMALL_BATCH : FILTER;
        } else {
            route = EXACT_SCAN;
            fused_prep = false;
        }
    }
};

// cooling: a cooldown of the filter watch is running.  eps_r_known, wide_blocks_known: the worst row's quantisation error norm and
// the number of 32-row blocks above shadow8_max_eps, as last read back from the int8 shadow's build.
inline SearchPlan plan_search(const FilterKnobs& kn, const IndexShape& s, int B, int k, bool cooling, float eps_r_known, int64_t wide_blocks_known) {
    SearchPlan p;
    if (s.count > 0 && space_filter_applies(kn, s, B, k)) {
        p.route = SearchPlan::SPACE_FILTER;
        p.use8 = true;  // (its passes read the int8 shadow; it has no 2-byte leg)
        return p;
    }
    if (!(s.count > 0 && filter_applies(kn, s, B, k))) {
        p.route = s.count > 0 ? SearchPlan::EXACT_SCAN : SearchPlan::EMPTY;
        return p;
    }
    p.can8 = int8_batch_ok(kn, B);
    // A corpus whose WORST block quantises badly keeps the int8 filter for the batches i8_tile_kernel takes as long as such blocks are
    // rare (under 1 %): that kernel and finalize evaluate the bound per 32-row block, so only the bad blocks' rows come through
    // as extra candidates.  The first-generation kernels (other batch sizes, rows under 384 elements) use the device-wide bound.
    p.per_block = B <= kTileQ && filter_program(kn, s, B, dpad8_of(s) / 128, true).family == FilterProgram::TILE;
    const bool eps_ok = eps_r_known <= kn.shadow8_max_eps || (p.per_block && wide_blocks_known * 100 <= (s.count + 31) / 32);
    p.use8 = p.can8 && !cooling && eps_ok;
    p.small_batch = small_batch_applies(kn, s, B, k);
    p.route = p.use8 && p.small_batch ? SearchPlan::SMALL_BATCH : SearchPlan::FILTER;
    p.fused_prep = B <= kTileQ;
    return p;
}

// Which way a masked search of m visible rows goes (time only, both routes give the same bits).  Dense — the
// ordinary dispatch under ~allow | dead — when the sample's anchors can be expected to hold 4k visible rows and the pass over the
// whole index costs less than ceil(B / NB) gathered walks of the list; "mask_list_pct" scales the dense side of that comparison.
inline bool mask_takes_dense(const FilterKnobs& kn, const IndexShape& s, int B, int k, int64_t m) {
    if (kn.mask_route == 1) return false;
    if (kn.mask_route == 2) return true;
    const int64_t n = s.count;
    const int64_t row_bytes = (int64_t)s.dpad * (int64_t)elem_size(s.dtype);
    const int nb = scope_nb(s.dtype, niter_of(s) > 4 ? kWideRows : niter_of(s));
    const double list_bytes = 2.0 * (double)((B + nb - 1) / nb) * (double)m * (double)row_bytes;
    double dense_bytes;
    if (filter_applies(kn, s, B, k)) {
        const bool can8 = int8_batch_ok(kn, B);
        const int64_t ts = sample_tile_count(kn, s, tiles_of(n), k, can8, nbq_of(B < kTileQ ? B : kTileQ));
        if ((double)m * (double)ts < 4.0 * (double)k * (double)n) return false;   // too few visible anchors: the pass would end in the fallback scan
        dense_bytes = (double)((B + kTileQ - 1) / kTileQ) * (double)n * (double)(can8 ? dpad8_of(s) : 2 * s.dpad);
    } else {
        // the exact scan reads the rows once per group of 8 queries, streaming: twice the rate of the gathered walk, as above
        dense_bytes = (double)((B + 7) / 8) * (double)n * (double)row_bytes;
    }
    return list_bytes * 100.0 > dense_bytes * (double)kn.mask_list_pct;
}

// Which filter suits the DATA is watched: on corpora with dense clusters the wider int8 slack lets thousands of rows per query
// through to the exact re-scoring, where the 2-byte filter (a fifth of the slack) is the faster one
// (profiles/r1/clustered_data_check.txt).  The device counters of the filter passes are copied back asynchronously (the pinned
// buffer and its event stay with the index); when the int8 passes since the last look left more than shadow8_max_surv survivors per
// query, or sent queries to the fallback, the next shadow8_cooldown searches take the 2-byte filter, then the int8 one is tried
// again.  Performance only: either filter returns the same bits.
struct FilterWatch {
    bool pending = false;                   // a copy of the counters is in flight
    unsigned long long surv = 0, fb = 0;    // counter values at the last look
    int64_t q8 = 0, q16 = 0;                // queries filtered since then, by path
    int64_t q8_sent = 0, q16_sent = 0;      // ... as of the copy in flight
    int cooldown_left = 0;
    int64_t stat_cooldowns = 0;
    double cooldown_surv8 = 0.0;            // survivors per query of the int8 passes that started the current cooldown
    int64_t cooldown_useless_epoch = -1;    // row epoch at which the 2-byte filter was seen to leave as many survivors as the int8 one: no more cooldowns until rows change

    // is a look due after search number `stat_searches`?  Each of the first 32, then every 8th: the copy is a launch of its own
    static bool due(int64_t stat_searches) { return stat_searches <= 32 || (stat_searches & 7) == 0; }
    // a copy of the counters has been enqueued
    void sent() {
        pending = true;
        q8_sent = q8;
        q16_sent = q16;
    }
    // ... and has arrived: the survivor and fallback counters as copied, at row epoch `epoch`
    void observe(unsigned long long surv_now, unsigned long long fb_now, int64_t epoch, const FilterKnobs& kn) {
        pending = false;
        if (q8_sent > 0 && q16_sent == 0) {  // only int8 passes in the window: the deltas are theirs
            const double per_q = (double)(surv_now - surv) / (double)q8_sent;
            if ((per_q > (double)kn.shadow8_max_surv || (fb_now - fb) * 20 > (unsigned long long)q8_sent) && cooldown_useless_epoch != epoch) {
                cooldown_left = kn.shadow8_cooldown;
                cooldown_surv8 = per_q;  // what the 2-byte filter has to beat
                stat_cooldowns++;
            }
        } else if (q16_sent > 0 && q8_sent == 0) {
            // only 2-byte passes (a cooldown): when those leave the re-scoring just as crowded — rows closer to each other than
            // EITHER slack — the slower 2-byte kernel buys nothing: stay on int8 until rows change
            // (relative, not absolute: the fp16 filter's passes cost about twice an int8 pass, so they pay as soon as they
            // leave well under half of the exact re-scoring — 7,000 survivors per query are a bargain against 62,000)
            const double per_q = (double)(surv_now - surv) / (double)q16_sent;
            if (per_q > (double)kn.shadow8_max_surv && per_q > 0.5 * cooldown_surv8) {
                cooldown_useless_epoch = epoch;
                cooldown_left = 0;
            }
        }
        surv = surv_now;
        fb = fb_now;
        q8 -= q8_sent;
        q16 -= q16_sent;
    }
};

}  // namespace codd
