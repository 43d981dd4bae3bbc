// codd_knn.hip — the one translation unit of libcodd_knn.so: HIP kernels (gfx950 / CDNA4, wave64) and the C ABI of include/codd_knn.h.
//
// What runs here is the arithmetic half of ChromaDB on Codd's search_relevant_metrics path
// (reference call sites: codd_dal/metrics/metrics_semantic_metadata_store.py:60-69 create,
// :236-238 upsert, :314-316 query; scoring :336).  In this order (one translation unit, kernels in the
// anonymous namespace, definition order is part of the build):
//
//   ingest_kernels.h     caller vectors -> stored rows and the bf16 shadow (normalised or raw), query preparation, row read-back
//   scan_kernels.h       the exact scan of the whole row store (dot product and squared L2), finalize + fallback, the key merges
//   shadow8_kernels.h    the int8 shadow, the int8 filter leg's query preparation and bounds, small_batch_kernel
//   list_scan_kernels.h  scans of row lists and what builds the lists: IVF, scopes, tombstones and compaction, masks
//   ivf_follow_kernels.h an IVF layout that follows writes: the pending bitmap, the delta scan, the fold's kernels
//   (here)               host side: the index object (its option knobs and filter watch are search_plan.h's), its workspaces and guards
//   dispatch.h           with_* (run-time value -> template argument), Lds, launch_kernel, launch_by_metric
//   (here)               the exact pass, the filter pass, search_impl, scopes, then the extern "C" entry points with the bodies of the
//                        IVF and masked searches between them
//
// The other headers (exact_score.h, wave_topk.h, row_traits.h, filter_gemm.h, filter_i8.h, doc_match.h, doc_regex.h, text_embed.h,
// where_eval.h, device_mem.h) are interfaces in namespace codd and come first.  Three of them take no HIP: geometry.h (the sizes kernels and host
// share), ivf_follow.h (the pending-row bookkeeping of a layout that follows writes) and search_plan.h, where the ROUTE of a search is decided — plan_search, filter_program, mask_takes_dense and their helpers,
// pure functions of (FilterKnobs, IndexShape, batch).  search_impl and filter_pass launch what those name and decide nothing.
//
// HBM-bound byte streaming throughout: the corpus is read once per pass, each row by exactly one
// wave, straight into registers; results leave as 8-byte keys.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <atomic>
#include <mutex>
#include <new>
#include <type_traits>
#include <vector>

#include "codd_knn.h"
#include "device_mem.h"

#ifndef CODD_EXPERIMENTS
#define CODD_EXPERIMENTS 0  // 1 (build_variant only): the diagnostic switches that can return wrong results exist
#endif
#include "doc_match.h"
#include "doc_regex.h"
#include "exact_score.h"
#include "filter_gemm.h"
#include "filter_i8.h"
#include "ivf_follow.h"
#include "row_traits.h"
#include "search_plan.h"
#include "text_embed.h"
#include "wave_topk.h"
#include "where_eval.h"

using namespace codd;

#include "ingest_kernels.h"
#include "scan_kernels.h"
#include "shadow8_kernels.h"
#include "list_scan_kernels.h"
#include "ivf_follow_kernels.h"

// =============================================================================================
// host side: the index object and the C ABI
// =============================================================================================

enum { EV_SCAN = 0, EV_FILTER = 1, EV_SAMPLE = 2, EV_FINALIZE = 3, EV_KINDS = 4 };
static const char* const kEvNames[EV_KINDS] = {"scan", "filter", "sample", "finalize"};

// device control block of one filter pass (zeroed by ONE memset per pass)
struct FilterCtl {
    unsigned hit_cnt[kTileQ * kHitCntStride];
    unsigned flags[FLAG_WORDS];
    unsigned fb_count;         // queries queued for the exact-scan fallback ...
    unsigned fb_done;          // ... blocks of the fallback scan that have finished (the last one merges)
    unsigned sb_ticket;        // small_batch_kernel's arrival counter (its last workgroup puts it back to zero)
    unsigned pad_[1];
    unsigned fb_list[kTileQ];  // ... and which ones
};

// What the last filter_pass on a workspace ran, for codd_knn_debug_last_pass: host fields only, no device state
struct LastPass {
    bool valid = false;
    int family = 0, nbq = 0, ts = 0, res = 0, el = 0, sqd = 0;
    int nq = 0, k = 0;
    int64_t n = 0, sample_tiles = 0, sample_stride = 0;
    int hit_cap = 0;
    float eps = 0.0f;
    int per_block_filter = 0, per_block_finalize = 0;
    int cascade_d = 0;   // the sample cascade ran with this d: sample_tiles, sample_stride are A0's, whose first tile is 1
};

// Search workspace.  An index keeps up to kMaxWork of them, one per HIP stream that searches it, so that searches
// issued on different streams (the next batch while this batch's small kernels and its collective are still in
// flight) never share scratch memory.  The index inherits one set of these fields: WorkScope loads the calling
// stream's set into them for the duration of one call and stores it back (a swap each way: one owner at any time).
struct WorkBufs {
    LastPass last;                // the last filter_pass that ran on this workspace (codd_knn_debug_last_pass)
    // (grown on demand, never inside a captured region after warm-up)
    DevBuf<float> qn;             // [B][dpad] normalised queries
    DevBuf<u64> partial;          // [B][blocks][k]
    DevBuf<u64> keys_tmp;         // [B][k]
    DevBuf<uint4> qfrag;          // pieces
    DevBuf<float> thr;            // [512]: thr[256], thr0[256]
    DevBuf<u64> bucket_max;       // [256][sample tiles] best (score, row) key per sampled tile
    DevBuf<u64> hits;             // [256][hit_cap_q]
    DevBuf<FilterCtl> ctl;        // device
    DevBuf<u64> fb_partial;       // [256][blocks][k] partials of the fallback scan
    DevBuf<uint4> qfrag8;         // int8 query fragments (pieces)
    DevBuf<float> qmeta;          // [1024]: per query: scale, 2*eps (device-wide bound), A, B (eps per block = A + B e_block)
    DevBuf<u64> sb_cand;          // small_batch_kernel: [waves][kSbKeep] published keys, then [waves] dropmax
    DevBuf<u64> probe_keys;       // IVF: [B][nprobe] coarse keys
    DevBuf<u64> ivf_partial;
    DevBuf<unsigned> ivf_group;   // IVF at batch: [nlist] counters, [nlist+1] pair starts, [nlist+1] item starts, [B*nprobe] pairs by list
    DevBuf<uint32_t> ivf_deny;    // IVF with rows pending: [ceil(count / 32)] the call's deny bits | the pending bits
    DevBuf<unsigned> scope_group; // scoped search: [B] queries in (scope, query) order, [B] their ranks inside the scope
    // masked search: the call's allow bits, and what the two routes derive from them
    PinnedBuf<uint32_t> mask_host;  // pinned staging of the allow words; mask_uploaded: its last copy to the device
    Event mask_uploaded; bool mask_upload_pending = false;
    DevBuf<uint32_t> mask_allow;    // [ceil(count / 32)] device copy of the allow words
    DevBuf<uint32_t> mask_deny;     // dense route: [ceil(capacity / 32)] ~allow | dead, ones past the mask
    DevBuf<unsigned> mask_prefix;   // list route: [words] prefixes, [blocks] totals, [blocks + 1] bases
    DevBuf<uint32_t> mask_list;     // list route: [m] visible row slots, ascending
    // codd_knn_search_masked_dev: the visible rows of a device mask, counted on the device and read back through pinned memory
    DevBuf<unsigned long long> mask_m_dev;
    PinnedBuf<unsigned long long> mask_m_host;
    // codd_knn_match_documents_dfa: the call's class map and table, staged in pinned memory and copied to the device
    // on the calling stream — per stream, so two threads' patterns cannot overwrite each other
    PinnedBuf<uint32_t> dfa_host;   // [kRegexTableWords]; dfa_uploaded: its last copy to the device
    Event dfa_uploaded; bool dfa_upload_pending = false;
    DevBuf<uint32_t> dfa_dev;       // [kRegexTableWords]
};
static_assert(!std::is_copy_constructible<WorkBufs>::value, "a workspace has one owner (WorkScope swaps, never copies)");
constexpr int kMaxWork = 4;
struct WorkSlot {
    WorkBufs bufs;
    hipStream_t stream = nullptr;
    Event handover;                 // recorded on the old stream when the slot changes hands
    bool used = false;
    uint64_t tick = 0;              // last use (LRU)
};

struct codd_knn_index : WorkBufs {
    int device = 0;
    int dim = 0;
    int dpad = 0;
    int dtype = 0;
    int metric = 0;
    int num_cus = 256;
    int64_t capacity = 0;  // row slots allocated
    int64_t count = 0;     // highest written slot + 1
    DevBuf<unsigned char> rows;  // [capacity][dpad] storage dtype, as bytes; zero at and past `count` (a never-written slot below the count is a zero row)
    // bf16 fragment-order copy, whole 256-row tiles.  Derived data like the int8 shadow: built lazily from the stored rows by the
    // first search that needs it (batches above 256 queries, an index with the int8 filter off or cooling down, the IVF
    // build), brought up to date incrementally over the rows written since
    DevBuf<uint4> shadow;
    int64_t shadow_rows = 0;       // rows the shadow allocation covers (multiple of 256)
    int64_t shadow_epoch = -1;
    int64_t dirty16_lo = 0, dirty16_hi = 0;
    hipStream_t shadow_stream = nullptr;
    Event shadow_ready;
    int64_t stat_shadow_builds = 0;
    int64_t shadow_nomem_epoch = -1;   // row epoch at which allocating the bf16 shadow failed: not retried until rows change
    int64_t stat_shadow_nomem = 0;
    int debug_fail_shadow_alloc = 0;   // test hook ("debug_fail_shadow_alloc"): the next bf16-shadow allocation reports out of memory
    int debug_num_cus = 0;             // test hook ("debug_num_cus"): > 0 = the filter passes plan and launch as if the device had this many compute units
    // stored rows written on a caller's stream (upsert_device): searches on other streams wait for this on the device
    Event rows_ready;
    hipStream_t rows_stream = nullptr;
    bool rows_event_set = false;
    // ... and rows read on a caller's stream outside a search (copy_rows_f32): the next writer on another stream waits for it
    Event reader_done;
    hipStream_t reader_stream = nullptr;
    bool reader_event_set = false;
    // staging of codd_knn_upsert_host (kept between calls: the indexer job upserts in small batches)
    DevBuf<float> stage_vec;
    DevBuf<int64_t> stage_slot;
    bool all_normalized = true;    // false once a caller stored rows with normalize = 0

    FilterKnobs knobs;   // the option-settable integers of the filter path (search_plan.h: plan_search reads them, never the index)

    DevBuf<unsigned long long> dstats;                     // device counters: hits, survivors, fallback queries

    // int8 shadow for small batches (optional; rebuilt lazily from the stored rows when they have changed)
    int64_t stat_small_batch = 0;
    DevBuf<uint4> shadow8;
    int64_t shadow8_rows = 0;     // rows the allocation covers (multiple of 256)
    DevBuf<float> rscale;         // [shadow8_rows]
    DevBuf<float2> bmeta;         // [shadow8_rows / 32]: per 32-row block {scale, largest error norm |c - c~| of its rows}; NaN scale: no row of the block exists
    DevBuf<unsigned> eps_r_bits;     // device scalar: max row error norm (float bits)
    // the int8 filter leg of an ip or l2 index ("space_filter" option, off by default).  Derived with the int8 shadow,
    // over the same dirty rows, and only for such an index: rnorm2[row] = the row's canonical sum of squares; *rmax_bits = the float
    // bits of R >= |c| for every row ever stored (it only grows: delete and compact never lower it)
    DevBuf<float> rnorm2;            // [shadow8_rows]
    DevBuf<unsigned> rmax_bits;
    int64_t shadow8_epoch = -1;
    int64_t dirty_lo = 0, dirty_hi = 0;  // rows written since the int8 shadow was last brought up to date: [lo, hi)
    hipStream_t shadow8_stream = nullptr;  // the stream the last rebuild ran on, and its completion
    Event shadow8_ready;
    int64_t stat_shadow8_builds = 0, stat_shadow8_passes = 0, stat_i8v2_passes = 0, stat_f16_tile_passes = 0;
    // the worst row's quantisation error, copied back asynchronously after every build: a corpus with badly
    // quantisable rows (one large element, many small ones) would make the int8 bound useless and send every small batch
    // to the exact-scan fallback, so such an index keeps the bf16 filter.  Performance only: never needed for exactness.
    PinnedBuf<float> eps_r_host;
    Event eps_r_copied;
    float eps_r_known = 0.0f;
    int64_t wide_blocks_known = 0;      // blocks whose error norm exceeds shadow8_max_eps, as last read back
    // the filter watch (search_plan.h): its state, and the asynchronous copy of dstats[0..3] that feeds it
    FilterWatch watch;
    PinnedBuf<unsigned long long> watch_host;
    Event watch_copied;
    float exp_slack_scale = 1.0f;  // always 1 in the shipped library; "exp_slack_pct" exists only in -DCODD_EXPERIMENTS=1 builds

    // IVF (optional): rows regrouped by coarse list, original slots, list offsets, the coarse index
    codd_knn_index* coarse = nullptr;  // nlist centroids, f32 (owned: destroyed through codd_knn_destroy)
    DevBuf<unsigned char> rows_ivf;
    DevBuf<uint32_t> ivf_ids;
    DevBuf<int64_t> ivf_offsets;       // [nlist + 1]
    int64_t ivf_count = 0;             // rows covered by the IVF layout (must equal count to be fresh)
    int ivf_nlist = 0;
    int64_t ivf_epoch = -1, epoch = 0;  // epoch bumps on every row write; search requires ivf_epoch == epoch
    // ... a layout that follows writes ("ivf_follow", off by default): a write through upsert_host, upsert_device or
    // load_rows marks its slots pending and keeps ivf_epoch at the epoch; the searches scan the lists under deny | pending and the
    // pending rows from the row store; a fold (codd_knn_ivf_refresh, or the write that crosses "ivf_fold_rows") rebuilds the layout
    int ivf_follow = 0;
    int64_t ivf_fold_rows = 0;         // "ivf_fold_rows": fold when more rows than this are pending (0 = one mean list)
    PendingRows pend;                  // host mirror of pend_bits and the number of distinct pending slots (ivf_follow.h)
    DevBuf<uint32_t> pend_bits;        // [ceil(capacity / 32)] device words, null until the first pending row
    DevBuf<uint32_t> pend_list;        // [>= pend.count] the distinct pending slots, in the order they became pending
    PinnedBuf<uint32_t> pend_stage;    // staging of the slots a write appends to pend_list; pend_staged: its last copy to the device
    Event pend_staged; bool pend_stage_pending = false;
    DevBuf<uint32_t> list_of;          // [>= count] the list of every row slot, built from ivf_ids / ivf_offsets by the first fold after an install
    bool list_of_valid = false;
    DevBuf<float> fold_q;              // the fold: [<= CODD_KNN_MAX_BATCH][dim] stored rows widened to fp32 (the coarse index's queries)
    DevBuf<unsigned> fold_cnt;         // ... [nlist] rows per list, then the scatter's fill counters
    DevBuf<int64_t> fold_perm;         // ... [count] slots by list position (gather_rows_kernel's permutation)
    int64_t stat_ivf_refreshes = 0, stat_ivf_delta = 0;   // folds; searches that ran a delta scan

    // scopes (optional): a label per row slot and, derived from it like the shadows, the row slots grouped by label
    DevBuf<uint32_t> scope_of;         // [capacity], 0 = no label; allocated by the first call that needs it
    DevBuf<uint32_t> scope_perm;       // [count] row slots grouped by scope
    DevBuf<unsigned> scope_offsets;    // [nlist + 1] group starts, then [nlist] counters of the build
    uint32_t max_scope = 0;            // highest label ever set
    int64_t scope_gen = 0;             // bumps on every codd_knn_set_scopes_host
    int64_t scope_built_gen = -1, scope_built_count = -1;  // what scope_perm / scope_offsets were built from
    hipStream_t scope_stream = nullptr;  // the stream the last build ran on, and its completion
    Event scope_ready;
    int64_t stat_scoped_searches = 0, stat_scope_builds = 0;

    // masked search
    DevBuf<unsigned long long> mask_dstats;     // the device counters of the dense masked passes: kept apart from dstats, which the filter watch reads
    int64_t stat_masked_searches = 0, stat_mask_list = 0, stat_mask_dense = 0, stat_last_mask_rows = 0;
    int64_t stat_masked_dev = 0;   // ... those of them whose mask was on the device already (codd_knn_search_masked_dev)

    // document snapshot (optional, derived data like the shadows): every row slot's document in one byte arena, a 0x00
    // behind each, zeros to the end of the allocation (csrc/doc_match.h), and the [count + 1] arena offsets.  Valid while the row
    // epoch and the count are what they were when codd_knn_set_documents_host took it.
    DevBuf<uint8_t> doc_arena;
    DevBuf<int64_t> doc_offsets;
    int64_t doc_bytes = 0;             // the arena: the documents' bytes plus one separator each
    int64_t doc_count = -1, doc_epoch = -1;
    int64_t stat_doc_matches = 0;
    int64_t stat_doc_regex_matches = 0;   // codd_knn_match_documents_dfa calls that launched

    // metadata columns (optional, derived data): per column a tag and a cell for every row slot, kept like scope_of —
    // allocated by the first codd_knn_set_column_host that names the column, [capacity], zero = absent, regrown by grow_rows, moved by
    // codd_knn_compact, dropped by codd_knn_load_rows
    struct WhereColumn {
        DevBuf<uint8_t> tags;
        DevBuf<uint64_t> cells;
    };
    WhereColumn columns[CODD_KNN_MAX_COLUMNS];
    int64_t where_max_blocks = 0;      // "where_max_blocks" option: workgroups of where_eval_kernel at most (0 = eight per compute unit)
    int64_t stat_where_evals = 0;

    // tombstones: one bit per row slot, set = deleted.  Null until the first codd_knn_delete_host — the kernels
    // take a null pointer as "nothing was ever deleted" and load nothing.  The host keeps a mirror: the write paths refuse dead
    // slots from it and compaction derives the row mapping from it, so nothing is ever read back.
    DevBuf<uint32_t> dead_bits;                                     // [ceil(capacity / 32)] device words
    std::vector<uint32_t> dead_host;                                // the same bits
    int64_t dead_count = 0;                                         // dead slots below `count`
    int64_t first_dead = INT64_MAX;                                 // lowest dead slot
    int64_t compact_chunk_rows = 0;                                 // "compact_chunk_rows" option: source rows per compaction chunk (0 = what 64 MiB hold)
    int64_t stat_delete_calls = 0, stat_compactions = 0;

    int64_t stat_searches = 0, stat_scan_launches = 0, stat_last_scan_blocks = 0;
    int64_t stat_last_scan_group = 0;       // queries per pass over the rows of the last exact scan (1, 4 or 8; wide 2-byte rows: at most 4)
    int64_t stat_last_finalize_parts = 0;   // workgroups per query of the last filter pass's finalize
    int64_t stat_ivf_shared = 0;            // IVF searches that scanned each probed list once for all its queries (ivf_scan_shared_kernel)
    int64_t stat_ivf_masked = 0;            // IVF searches under a row mask (codd_knn_ivf_search_masked, _masked_dev: DESIGN.md §17)
    int64_t stat_filter_passes = 0;
    int64_t stat_sweep_passes = 0, stat_last_sweep = 0;   // filter passes whose filter launches ran i8_sweep_kernel, and whether the last pass was one
    int64_t stat_cascade_passes = 0, stat_last_cascade_d = 0;   // filter passes that took the sample cascade, and the d of the last pass (0: none)

    // optional HIP-event timing of the heavy kernels (bench.py's roofline figure): one (start, stop)
    // pair per launch, recorded on the launch stream, read after a sync
    bool profile = false;
    std::vector<Event> ev;  // 2 * pairs
    std::vector<int> ev_kind;
    int ev_used = 0;

    WorkSlot slots[kMaxWork];
    uint64_t tick = 0;
    std::mutex mu;  // one host thread at a time enqueues a search (the launches themselves are asynchronous)

    // (the members free themselves: the caller has made `device` current and idle, see codd_knn_destroy)
    ~codd_knn_index() { (void)codd_knn_destroy(coarse); }
};
static_assert(!std::is_copy_constructible<codd_knn_index>::value, "an index owns its device memory");

// what the route rules of search_plan.h see of an index
inline IndexShape shape_of(const codd_knn_index* ix) {
    IndexShape s;
    s.count = ix->count; s.dim = ix->dim; s.dpad = ix->dpad; s.dtype = ix->dtype; s.metric = ix->metric; s.num_cus = ix->num_cus;
    s.all_normalized = ix->all_normalized;
    return s;
}

// The device embedder: no index behind it — an index does not exist before the first upsert fixes the width.
// One pinned staging buffer and its device copy, both laid out [n + 1 offsets][bytes]; `uploaded` frees the staging buffer for
// the next call, `embedded` orders a call on another stream behind the kernel that still reads the device copy.
struct codd_knn_embedder {
    int device = 0;
    int dim = 0;
    float trigram_weight = 0.0f;
    bool device_seen = false;          // the first call that embeds checks that `device` exists; create and destroy touch no device before
    PinnedBuf<unsigned char> stage_host;
    DevBuf<unsigned char> stage_dev;
    Event uploaded, embedded;
    bool upload_pending = false, embedded_set = false;
    hipStream_t last_stream = nullptr;
    std::mutex mu;                     // one host thread at a time stages and enqueues
};

namespace {

thread_local char g_err[512] = "";

int fail(int code, const char* fmt, const char* detail = "") {
    snprintf(g_err, sizeof(g_err), fmt, detail);
    return code;
}

// every row write: bumps the epoch (IVF / int8 shadow staleness) and widens the dirty row range
void rows_written(codd_knn_index* ix, int64_t lo, int64_t hi) {
    ix->epoch++;
    if (ix->dirty_hi <= ix->dirty_lo) { ix->dirty_lo = lo; ix->dirty_hi = hi; }
    else {
        if (lo < ix->dirty_lo) ix->dirty_lo = lo;
        if (hi > ix->dirty_hi) ix->dirty_hi = hi;
    }
    if (ix->dirty16_hi <= ix->dirty16_lo) { ix->dirty16_lo = lo; ix->dirty16_hi = hi; }
    else {
        if (lo < ix->dirty16_lo) ix->dirty16_lo = lo;
        if (hi > ix->dirty16_hi) ix->dirty16_hi = hi;
    }
}

// the end of every write of row slots inside [lo, hi): raises the count, then rows_written.  A write that starts above the count
// brings the slots in between into existence unwritten.  They are zero rows: the row store holds zeros at and
// past the count (grow_rows, codd_knn_compact), but both shadows still hold there whatever they held — int8 block meta data that
// reads NaN since the allocation, rows from before a compaction — so they are dirty from the old count on.
void slots_written(codd_knn_index* ix, int64_t lo, int64_t hi) {
    if (hi > ix->count) {
        if (lo > ix->count) lo = ix->count;
        ix->count = hi;
    }
    rows_written(ix, lo, hi);
}

#define HIP_TRY(expr)                                                                        \
    do {                                                                                     \
        hipError_t e__ = (expr);                                                             \
        if (e__ != hipSuccess) {                                                             \
            snprintf(g_err, sizeof(g_err), "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__), __FILE__, __LINE__); \
            return e__ == hipErrorOutOfMemory ? CODD_KNN_ENOMEM : CODD_KNN_EDEVICE;          \
        }                                                                                    \
    } while (0)

struct DeviceGuard {
    int prev = -1;
    bool changed = false;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) == hipSuccess && prev != dev) changed = hipSetDevice(dev) == hipSuccess;
    }
    ~DeviceGuard() {
        if (changed) (void)hipSetDevice(prev);
    }
};

struct EvScope {  // records a (start, stop) pair around one launch when profiling is on
    codd_knn_index* ix;
    hipStream_t st;
    int slot = -1;
    EvScope(codd_knn_index* ix_, int kind, hipStream_t st_) : ix(ix_), st(st_) {
        if (ix->profile && 2 * (ix->ev_used + 1) <= (int)ix->ev.size()) {
            slot = ix->ev_used++;
            ix->ev_kind[slot] = kind;
            (void)hipEventRecord(ix->ev[2 * slot], st);
        }
    }
    // the pair ends here instead of at the end of the scope
    void stop() {
        if (slot >= 0) (void)hipEventRecord(ix->ev[2 * slot + 1], st);
        slot = -1;
    }
    ~EvScope() { stop(); }
};

// Loads the calling stream's workspace into the index for one call (see WorkBufs).  A stream keeps its slot; a new
// stream takes a free slot, or the least recently used one after making itself wait for everything the previous
// owner has enqueued so far (no host synchronisation; if that stream no longer exists the device is drained instead).
struct WorkScope {
    codd_knn_index* ix;
    int slot = 0;
    WorkScope(codd_knn_index* ix_, hipStream_t st) : ix(ix_) {
        ix->mu.lock();
        int free_slot = -1, lru = 0;
        slot = -1;
        for (int i = 0; i < kMaxWork; ++i) {
            WorkSlot& w = ix->slots[i];
            if (w.used && w.stream == st) { slot = i; break; }
            if (!w.used && free_slot < 0) free_slot = i;
            if (w.used && ix->slots[lru].used && w.tick < ix->slots[lru].tick) lru = i;
        }
        if (slot < 0 && free_slot >= 0) slot = free_slot;
        if (slot < 0) {
            slot = lru;
            WorkSlot& w = ix->slots[slot];
            bool ordered = false;
            (void)w.handover.ensure();
            if (w.handover && hipEventRecord(w.handover, w.stream) == hipSuccess) ordered = hipStreamWaitEvent(st, w.handover, 0) == hipSuccess;
            if (!ordered) {
                (void)hipGetLastError();
                (void)hipDeviceSynchronize();
            }
        }
        WorkSlot& w = ix->slots[slot];
        w.used = true;
        w.stream = st;
        w.tick = ++ix->tick;
        std::swap(static_cast<WorkBufs&>(*ix), w.bufs);
    }
    ~WorkScope() {
        std::swap(static_cast<WorkBufs&>(*ix), ix->slots[slot].bufs);
        ix->mu.unlock();
    }
    WorkScope(const WorkScope&) = delete;
    WorkScope& operator=(const WorkScope&) = delete;
};

int grow_dead_bits(codd_knn_index* ix, int64_t slots);
int grow_pend_bits(codd_knn_index* ix, int64_t slots);

// (re)allocate row storage for at least `need` slots, preserving contents (the shadows are derived data with their own
// allocations: ensure_shadow / ensure_shadow8)
int grow_rows(codd_knn_index* ix, int64_t need, bool exact) {
    if (need <= ix->capacity) return CODD_KNN_OK;
    int64_t cap = need;
    if (!exact) {
        cap = ix->capacity > 0 ? ix->capacity : 1024;
        while (cap < need) cap += cap / 2 + 1024;
    }
    const size_t row_bytes = (size_t)ix->dpad * elem_size(ix->dtype);
    DevBuf<unsigned char> fresh;
    HIP_TRY(fresh.reset(cap * (int64_t)row_bytes));
    hipError_t e = hipMemset(fresh, 0, (size_t)cap * row_bytes);
    if (e == hipSuccess && ix->rows && ix->count > 0) e = hipMemcpy(fresh, ix->rows, (size_t)ix->count * row_bytes, hipMemcpyDeviceToDevice);
    if (e != hipSuccess) return fail(CODD_KNN_EDEVICE, "row copy on growth failed: %s", hipGetErrorString(e));
    if (ix->scope_of && ix->scope_of.cap() < cap) {  // the labels grow with the row store: new slots start with scope 0
        DevBuf<uint32_t> labels;
        e = labels.reset(cap);
        if (e == hipSuccess) e = hipMemset(labels, 0, (size_t)cap * sizeof(uint32_t));
        if (e == hipSuccess) e = hipMemcpy(labels, ix->scope_of, (size_t)ix->scope_of.bytes(), hipMemcpyDeviceToDevice);
        if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? CODD_KNN_ENOMEM : CODD_KNN_EDEVICE, "growing the scope labels failed: %s", hipGetErrorString(e));
        ix->scope_of = std::move(labels);
    }
    if (ix->dead_bits) {  // ... and so do the tombstone bits, once they exist
        const int rc = grow_dead_bits(ix, cap);
        if (rc != 0) return rc;
    }
    if (ix->pend_bits) {  // ... and the pending bits of an IVF layout that follows writes
        const int rc = grow_pend_bits(ix, cap);
        if (rc != 0) return rc;
    }
    for (auto& col : ix->columns) {  // ... and the metadata columns that exist: new slots read absent
        if (!col.tags || col.tags.cap() >= cap) continue;
        DevBuf<uint8_t> tags;
        DevBuf<uint64_t> cells;
        e = tags.reset(cap);
        if (e == hipSuccess) e = cells.reset(cap);
        if (e == hipSuccess) e = hipMemset(tags, 0, (size_t)cap);
        if (e == hipSuccess) e = hipMemset(cells, 0, (size_t)cap * sizeof(uint64_t));
        if (e == hipSuccess) e = hipMemcpy(tags, col.tags, (size_t)col.tags.bytes(), hipMemcpyDeviceToDevice);
        if (e == hipSuccess) e = hipMemcpy(cells, col.cells, (size_t)col.cells.bytes(), hipMemcpyDeviceToDevice);
        if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? CODD_KNN_ENOMEM : CODD_KNN_EDEVICE, "growing a metadata column failed: %s", hipGetErrorString(e));
        col.tags = std::move(tags);
        col.cells = std::move(cells);
    }
    ix->rows = std::move(fresh);
    ix->capacity = cap;
    return CODD_KNN_OK;
}

// the tombstone bits cover `slots` row slots (device words and host mirror; contents kept, new words zero).  Exclusive callers only.
int grow_dead_bits(codd_knn_index* ix, int64_t slots) {
    const int64_t words = (slots + 31) / 32;
    if (words <= ix->dead_bits.cap()) return CODD_KNN_OK;
    try {
        ix->dead_host.resize((size_t)words, 0u);
    } catch (const std::bad_alloc&) {
        return fail(CODD_KNN_ENOMEM, "host allocation failed%s");
    }
    DevBuf<uint32_t> fresh;
    hipError_t e = fresh.reset(words);
    if (e == hipSuccess) e = hipMemset(fresh, 0, (size_t)words * sizeof(uint32_t));
    if (e == hipSuccess && ix->dead_bits) e = hipMemcpy(fresh, ix->dead_bits, (size_t)ix->dead_bits.bytes(), hipMemcpyDeviceToDevice);
    if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? CODD_KNN_ENOMEM : CODD_KNN_EDEVICE, "growing the tombstone bits failed: %s", hipGetErrorString(e));
    ix->dead_bits = std::move(fresh);
    return CODD_KNN_OK;
}

// the pending bits cover `slots` row slots (device words only: the mirror grows where it is marked; contents kept, new words zero).
// Exclusive callers with the device drained only (grow_rows); the device is idle again when it returns.
int grow_pend_bits(codd_knn_index* ix, int64_t slots) {
    const int64_t words = (slots + 31) / 32;
    if (words <= ix->pend_bits.cap()) return CODD_KNN_OK;
    DevBuf<uint32_t> fresh;
    hipError_t e = fresh.reset(words);
    if (e == hipSuccess) e = hipMemset(fresh, 0, (size_t)words * sizeof(uint32_t));
    if (e == hipSuccess && ix->pend_bits) e = hipMemcpy(fresh, ix->pend_bits, (size_t)ix->pend_bits.bytes(), hipMemcpyDeviceToDevice);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? CODD_KNN_ENOMEM : CODD_KNN_EDEVICE, "growing the pending bits failed: %s", hipGetErrorString(e));
    ix->pend_bits = std::move(fresh);
    return CODD_KNN_OK;
}

bool slot_dead(const codd_knn_index* ix, int64_t slot) {
    return ix->dead_count > 0 && slot >= 0 && (slot >> 5) < (int64_t)ix->dead_host.size() && ((ix->dead_host[(size_t)(slot >> 5)] >> (slot & 31)) & 1u);
}
// any dead slot in [lo, hi)?  (the write paths: a dead slot stays dead until codd_knn_compact)
bool range_has_dead(const codd_knn_index* ix, int64_t lo, int64_t hi) {
    if (ix->dead_count == 0 || hi <= ix->first_dead) return false;
    for (int64_t r = lo > ix->first_dead ? lo : ix->first_dead; r < hi && r < ix->count; ++r)
        if (slot_dead(ix, r)) return true;
    return false;
}
// live slots in [lo, hi), from the host mirror
int64_t live_in_range(const codd_knn_index* ix, int64_t lo, int64_t hi) {
    int64_t dead = 0;
    for (int64_t r = lo; r < hi;) {
        if ((r & 31) == 0 && r + 32 <= hi) { dead += __builtin_popcount(ix->dead_host[(size_t)(r >> 5)]); r += 32; }
        else { dead += (ix->dead_host[(size_t)(r >> 5)] >> (r & 31)) & 1u; ++r; }
    }
    return (hi - lo) - dead;
}

}  // namespace

#include "dispatch.h"

namespace {

int launch_normalize(int dtype, const float* in, int64_t n, int d, int dpad, int normalize, const int64_t* slots,
                     int64_t first_slot, void* out, uint2* shadow, hipStream_t st) {
    if (n <= 0) return CODD_KNN_OK;
    const dim3 grid((unsigned)((n + 3) / 4)), block(256);
    const int rc = with_dtype(dtype, [&](auto dt) {
        return launch_kernel<normalize_rows_kernel<dt>>(grid, block, 0, st, in, n, d, dpad, normalize, slots, first_slot, out, shadow);
    });
    if (rc != 0) return rc;
    HIP_TRY(hipGetLastError());
    return CODD_KNN_OK;
}

// raw_rows_kernel: vectors as given (non-finite and all-zero ones as zeros), padded and rounded to `dtype`
int launch_raw_rows(int dtype, const float* in, int64_t n, int d, int dpad, const int64_t* slots, int64_t first_slot, void* out, hipStream_t st) {
    if (n <= 0) return CODD_KNN_OK;
    const dim3 grid((unsigned)((n + 3) / 4)), block(256);
    const int rc = with_dtype(dtype, [&](auto dt) { return launch_kernel<raw_rows_kernel<dt>>(grid, block, 0, st, in, n, d, dpad, slots, first_slot, out); });
    if (rc != 0) return rc;
    HIP_TRY(hipGetLastError());
    return CODD_KNN_OK;
}

// the metric of an index as its exact-score kernels see it: ip scores with the dot-product kernels that cosine runs
static_assert(kMetricDot == CODD_KNN_METRIC_COSINE && kMetricL2 == CODD_KNN_METRIC_L2, "exact_score.h and codd_knn.h disagree");
bool metric_is_cosine(const codd_knn_index* ix) { return ix->metric == CODD_KNN_METRIC_COSINE; }
// IVF: cosine always; ip and l2 with "space_ivf" on
bool ivf_allowed(const codd_knn_index* ix) { return metric_is_cosine(ix) || ix->knobs.space_ivf; }
int kernel_metric(int metric) { return metric == CODD_KNN_METRIC_L2 ? kMetricL2 : kMetricDot; }

// the ingest launch of every upsert.  normalize = 0 on an ip or l2 index still zeroes non-finite rows (the contract of those
// spaces); on a cosine index it stores the values as they come, as it always did
int launch_ingest(const codd_knn_index* ix, const float* in, int64_t n, int normalize, const int64_t* slots, int64_t first_slot, hipStream_t st) {
    if (!normalize && !metric_is_cosine(ix)) return launch_raw_rows(ix->dtype, in, n, ix->dim, ix->dpad, slots, first_slot, ix->rows.get(), st);
    return launch_normalize(ix->dtype, in, n, ix->dim, ix->dpad, normalize, slots, first_slot, ix->rows.get(), nullptr, st);
}

// the queries of an exact-score pass, fp32 [B][dpad] in ix->qn: normalised for cosine, as given for ip and l2
int prep_exact_queries(codd_knn_index* ix, const float* dev_queries, int B, hipStream_t st) {
    if (metric_is_cosine(ix)) return launch_normalize(DT_F32, dev_queries, B, ix->dim, ix->dpad, 1, nullptr, 0, ix->qn, nullptr, st);
    return launch_raw_rows(DT_F32, dev_queries, B, ix->dim, ix->dpad, nullptr, 0, ix->qn.get(), st);
}

// ---- exact scan dispatch ---------------------------------------------------------------------

struct ScanArgs {
    const void* rows;
    int64_t n;
    int dpad;
    const float* qn;
    int nq, k;
    uint32_t row_base;
    u64* partial;
    int64_t stride_q;
    const unsigned* qlist = nullptr;   // LISTED mode (device-side fallback queue)
    const unsigned* qcount = nullptr;
    unsigned* merge_done = nullptr;    // LISTED mode: the last block merges and writes the answers (one launch)
    u64* merged_keys = nullptr;
    float* merged_dist = nullptr;
    int64_t* merged_rows = nullptr;
    unsigned long long* count_total = nullptr;
    const uint32_t* dead = nullptr;    // tombstone bits (null: nothing was ever deleted)
};

// queries per pass of the wide scan: 2-byte rows take at most 4 (8 would spill: the kernel walks a larger batch 4 queries at a time)
constexpr int wide_scan_nb(int dt, int nb) { return dt == DT_F32 || nb < 4 ? nb : 4; }
// ... and of the wide l2 scan: the same, but 2-byte rows with two list slots per lane (k > 64) take 2 (the subtraction's temporaries on top
// of 4 queries' accumulators and 8 list registers spill one vector register in scan_topk_wide_l2<bf16, 4, 2>)
constexpr int wide_scan_nb_l2(int dt, int nb, int slots) { return dt != DT_F32 && slots == 2 && nb >= 4 ? 2 : wide_scan_nb(dt, nb); }

// one exact-scan launch, queries in groups of `nb` (1, 4 or 8) per pass over the rows
// (l2: the squared-distance kernels, dense queries only)
int launch_scan(int dtype, int nb, int niter, dim3 grid, hipStream_t st, const ScanArgs& a, int metric = kMetricDot) {
    if (metric == kMetricL2 && (a.qlist || a.qcount)) return fail(CODD_KNN_EINVAL, "the l2 scan takes dense queries only%s");
    return with_dtype(dtype, [&](auto dt) {
        constexpr int DT = decltype(dt)::value;
        return with_int<1, 4, 8>(nb, "bad query group%s", [&](auto nbc) {
            constexpr int NB = decltype(nbc)::value;
            return with_slots(a.k, [&](auto sl) {
                constexpr int SLOTS = decltype(sl)::value;
                return with_niter(niter, "row too wide for the scan kernel%s", [&](auto ni) {
                    constexpr int NITER = decltype(ni)::value;
                    if constexpr (NITER == kWideRows) {
                        // rows of more than 4 chunks per lane: scan_topk_wide_kernel, one 8-wave workgroup per compute unit (scan_geometry sizes the grid)
                        constexpr int NBW = wide_scan_nb(DT, NB);
                        constexpr int E = RowTraits<DT>::E;
                        if (metric == kMetricL2) {
                            constexpr int NBL = wide_scan_nb_l2(DT, NB, SLOTS);
                            const size_t qbytes = (size_t)NBL * wide_qfloats(a.dpad / E, E) * sizeof(float);
                            const size_t lbytes = (size_t)kWideScanWaves * NBL * SLOTS * kWave * sizeof(u64);
                            return launch_kernel<scan_topk_wide_l2<DT, NBL, SLOTS>>(grid, dim3(kWideScanWaves * kWave),
                                                                                    Lds(qbytes > lbytes ? qbytes : lbytes, (size_t)NBL * kWideMaxFloats * sizeof(float)),
                                                                                    st, a.rows, a.n, a.dpad, a.qn, a.nq, a.k, a.row_base, a.partial, a.stride_q, a.dead);
                        }
                        const size_t qbytes = (size_t)NBW * wide_qfloats(a.dpad / E, E) * sizeof(float);
                        const size_t lbytes = (size_t)kWideScanWaves * NBW * SLOTS * kWave * sizeof(u64);
                        const size_t lds = qbytes > lbytes ? qbytes : lbytes;   // the lists take the queries' place once a group is scanned
                        return launch_kernel<scan_topk_wide_kernel<DT, NBW, SLOTS>>(
                            grid, dim3(kWideScanWaves * kWave), Lds(lds, (size_t)NBW * kWideMaxFloats * sizeof(float)), st, a.rows, a.n, a.dpad, a.qn, a.nq,
                            a.k, a.row_base, a.partial, a.stride_q, a.qlist, a.qcount, a.merge_done, a.merged_keys, a.merged_dist, a.merged_rows, a.count_total, a.dead);
                    } else {
                        const size_t lds = (size_t)4 * NB * SLOTS * kWave * sizeof(u64);
                        if (metric == kMetricL2)
                            return launch_kernel<scan_topk_l2<DT, NB, NITER, SLOTS>>(grid, dim3(256), lds, st, a.rows, a.n, a.dpad, a.qn, a.nq, a.k, a.row_base,
                                                                                     a.partial, a.stride_q, a.dead);
                        return launch_kernel<scan_topk_kernel<DT, NB, NITER, SLOTS>>(
                            grid, dim3(256), lds, st, a.rows, a.n, a.dpad, a.qn, a.nq, a.k, a.row_base, a.partial, a.stride_q, a.qlist, a.qcount,
                            a.merge_done, a.merged_keys, a.merged_dist, a.merged_rows, a.count_total, a.dead);
                    }
                });
            });
        });
    });
}

int launch_merge(const u64* in, int B, int64_t m, int64_t in_stride, int k, u64* out_keys, float* out_dist, int64_t* out_rows,
                 hipStream_t st, const unsigned* out_list = nullptr, const unsigned* count_ptr = nullptr,
                 unsigned long long* count_total = nullptr, int64_t seg_len = 0, int64_t seg_stride = 0, int metric = kMetricDot) {
    if (seg_len <= 0) seg_len = m > 0 ? m : 1;
    if (metric == kMetricL2 && (out_list || count_ptr)) return fail(CODD_KNN_EINVAL, "the l2 merge takes no query list%s");
    const int rc = with_slots(k, [&](auto sl) {
        if (metric == kMetricL2)
            return launch_kernel<merge_keys_l2<sl>>(dim3(B), dim3(256), 0, st, in, m, in_stride, seg_len, seg_stride, k, out_keys, out_dist, out_rows);
        return launch_kernel<merge_keys_kernel<sl>>(dim3(B), dim3(256), 0, st, in, m, in_stride, seg_len, seg_stride, k, out_keys, out_dist, out_rows,
                                                    out_list, count_ptr, count_total);
    });
    if (rc != 0) return rc;
    HIP_TRY(hipGetLastError());
    return CODD_KNN_OK;
}

// the merge behind an index's own exact-score passes: distances by the index's metric
int launch_merge_of(const codd_knn_index* ix, const u64* in, int B, int64_t m, int k, u64* out_keys, float* out_dist, int64_t* out_rows, hipStream_t st) {
    return launch_merge(in, B, m, m, k, out_keys, out_dist, out_rows, st, nullptr, nullptr, nullptr, 0, 0, kernel_metric(ix->metric));
}

int scan_geometry(const codd_knn_index* ix, int64_t n, int* niter, int64_t* blocks) {
    *niter = niter_of(shape_of(ix));
    if (*niter > kMaxNiter) return fail(CODD_KNN_ENOTSUP, "dim too large (<= 4096 elements)%s");
    const int64_t ngroups = (n + 3) / 4;
    if (*niter > 4) {  // scan_topk_wide_kernel: workgroups of 8 waves, one per compute unit (its query block fills the LDS)
        int64_t b = (ngroups + kWideScanWaves - 1) / kWideScanWaves;
        if (b > ix->num_cus) b = ix->num_cus;
        *blocks = b < 1 ? 1 : b;
        return CODD_KNN_OK;
    }
    int64_t b = (ngroups + 3) / 4;
    const int64_t cap_blocks = (int64_t)ix->num_cus * ix->knobs.scan_blocks_per_cu;
    if (b > cap_blocks) b = cap_blocks;
    if (b < 1) b = 1;
    *blocks = b;
    return CODD_KNN_OK;
}

// exact scan of `nqueries` dense normalised queries -> keys_out[nqueries][k]
// (deny: the bitmap of rows no answer may hold — the tombstone bits, or a masked search's ~allow | dead; null = none)
int exact_scan(codd_knn_index* ix, const float* qn, int nqueries, int k, uint32_t row_base, u64* keys_out, float* dist_out,
               int64_t* rows_out, hipStream_t st, const uint32_t* deny) {
    const int64_t n = ix->count;
    int niter;
    int64_t blocks;
    int rc = scan_geometry(ix, n, &niter, &blocks);
    if (rc != 0) return rc;
    ix->stat_last_scan_blocks = blocks;
    const int64_t stride_q = blocks * k;
    HIP_TRY(ix->partial.ensure((int64_t)nqueries * stride_q));
    {
        // ONE launch: up to 8 queries ride along per pass over the rows; a larger batch loops over groups
        // of 8 inside the kernel (small corpora stay L2-resident across the groups, and a batch costs one
        // launch instead of B/8)
        const int nb = nqueries == 1 ? 1 : (nqueries <= 4 ? 4 : 8);
        ix->stat_last_scan_group = niter <= 4 ? nb : (ix->metric == CODD_KNN_METRIC_L2 ? wide_scan_nb_l2(ix->dtype, nb, k <= 64 ? 1 : 2) : wide_scan_nb(ix->dtype, nb));
        ScanArgs a{ix->rows, n, ix->dpad, qn, nqueries, k, row_base, ix->partial, stride_q};
        a.dead = deny;
        {
            EvScope ev(ix, EV_SCAN, st);
            rc = launch_scan(ix->dtype, nb, niter, dim3((unsigned)blocks), st, a, kernel_metric(ix->metric));
        }
        if (rc != 0) return rc;
        HIP_TRY(hipGetLastError());
        ix->stat_scan_launches++;
    }
    return launch_merge_of(ix, ix->partial, nqueries, stride_q, k, keys_out, dist_out, rows_out, st);
}

// ---- filter path -----------------------------------------------------------------------------

float filter_eps(const codd_knn_index* ix) {
    // |approx - exact| for unit-norm q and c.  u = unit roundoff of the shadow element type under round-to-nearest:
    // half the spacing of the significand grid relative to the value (bf16: 8 significant bits, spacing 2^-7 -> u = 2^-8;
    // fp16: 11 significant bits -> u = 2^-11).  Round 1 shipped 2^-9 for bf16, half the true bound: a unit vector of 239
    // equal entries scores 0.99286 against itself in bf16 (error 0.0071 > the old eps 0.0040):
    //   rounding  : (2u + u^2) when q and the stored row are both rounded (Cauchy-Schwarz over the
    //               element-wise relative errors); u when the stored rows already are exactly
    //               representable (bf16 rows under a bf16 shadow, f16 rows under an fp16 shadow);
    //   subnormal : fp16 only — below 2^-14 the grid is absolute (2^-25 per element, <= sqrt(dpad) * 2^-25
    //               per operand after Cauchy-Schwarz against a unit vector);
    //   summation : two fp32 accumulations of <= dpad terms whose magnitudes sum to <= 1: dpad * 2^-24 each.
#if CODD_SHADOW_F16
    const float u = 4.8828125e-4f;
    const bool exact_rows = ix->dtype == DT_F16;
    const float subnormal = 2.0f * sqrtf((float)ix->dpad) * 2.9802322e-8f;
#else
    const float u = 0.00390625f;
    const bool exact_rows = ix->dtype == DT_BF16;
    const float subnormal = 0.0f;
#endif
    const float rounding = exact_rows ? u : 2.0f * u + u * u;
    const float summation = (float)ix->dpad * 1.1920929e-7f;  // dpad * 2^-23
    return (rounding + subnormal + summation) * 1.001f;
}

size_t filter_lds_bytes(int mode) {
    return (size_t)kLdsQBytes + kLdsWords * 4 + (mode == MODE_FILTER ? (size_t)kHitCap * 12 : 0);
}

int ensure_filter_workspace(codd_knn_index* ix) {
    HIP_TRY(ix->qfrag.ensure((int64_t)kTileQ * (ix->dpad / 8)));
    HIP_TRY(ix->bucket_max.ensure((int64_t)ix->knobs.sample_tiles * kTileQ));
    HIP_TRY(ix->hits.ensure((int64_t)kTileQ * ix->knobs.hit_cap_q));
    if (!ix->thr) HIP_TRY(ix->thr.reset(2 * kTileQ));  // thr[q], then thr0[q] (per-block form, int8 tile kernel)
    if (!ix->ctl) {
        HIP_TRY(ix->ctl.reset(1));
        HIP_TRY(hipMemset(ix->ctl, 0, sizeof(FilterCtl)));  // (the filter passes clear it per pass; small_batch_kernel relies on zeros left behind)
    }
    if (!ix->dstats) {
        HIP_TRY(ix->dstats.reset(4));
        HIP_TRY(hipMemset(ix->dstats, 0, 4 * sizeof(unsigned long long)));
    }
    return CODD_KNN_OK;
}

// Searches on a stream other than the one rows were last written on (codd_knn_upsert_device is asynchronous on the caller's
// stream) wait for that write on the device before they read rows or rebuild a shadow from them.
int wait_rows(codd_knn_index* ix, hipStream_t st) {
    if (ix->rows_event_set && st != ix->rows_stream) HIP_TRY(hipStreamWaitEvent(st, ix->rows_ready, 0));
    return CODD_KNN_OK;
}

// Before a derived buffer is freed (a shadow outgrown by the corpus): wait on the host for the streams that search THIS index
// — what they have enqueued so far may still read the old allocation — not for the whole device.  (Growth is the one
// place where a search call blocks; steady-state searches never do.)
int wait_searching_streams(codd_knn_index* ix) {
    for (WorkSlot& w : ix->slots) {
        if (!w.used) continue;
        HIP_TRY(w.handover.ensure());
        if (hipEventRecord(w.handover, w.stream) == hipSuccess) HIP_TRY(hipEventSynchronize(w.handover));
        else (void)hipGetLastError();  // (a stream that no longer exists has nothing in flight)
    }
    return CODD_KNN_OK;
}

// The bf16 shadow, like the int8 one, is derived data: (re)built from the stored rows on the searching stream whenever rows
// have been written since the last build, over the dirty row range only.  An index that only ever sees batches of <= 256
// queries (the int8 filter) never allocates it: 38 GB instead of 54 GB for the 10M x 768 fp32 corpus.
int ensure_shadow(codd_knn_index* ix, hipStream_t st) {
    const int64_t n = ix->count;
    if (ix->shadow_epoch == ix->epoch && ix->shadow) {
        if (st != ix->shadow_stream && ix->shadow_ready) HIP_TRY(hipStreamWaitEvent(st, ix->shadow_ready, 0));
        return CODD_KNN_OK;
    }
    const int64_t need = tiles_of(n) * kTileRows;
    int64_t first = ix->dirty16_lo, m = ix->dirty16_hi - ix->dirty16_lo;
    if (first + m > n) m = n > first ? n - first : 0;  // (never past the count: the allocation below is only checked against it)
    if (need > ix->shadow_rows) {
        // A failed allocation is remembered until rows change (no multi-GB hipMalloc retried by every search); the caller
        // answers the search another way (search_impl: the int8 filter or the exact scan).
        if (ix->shadow_nomem_epoch == ix->epoch) return CODD_KNN_ENOMEM;
        int rc;
        if ((rc = wait_searching_streams(ix)) != 0) return rc;
        (void)ix->shadow.reset();
        ix->shadow_rows = 0;
        const int64_t rows = need + need / 8;
        const int64_t rows_al = tiles_of(rows) * kTileRows;
        hipError_t me = ix->debug_fail_shadow_alloc ? hipErrorOutOfMemory : ix->shadow.reset(rows_al * ix->dpad * 2 / (int64_t)sizeof(uint4));
        if (me != hipSuccess) {
            (void)hipGetLastError();
            ix->shadow_nomem_epoch = ix->epoch;
            ix->stat_shadow_nomem++;
            return fail(CODD_KNN_ENOMEM, "bf16 shadow: %s", hipGetErrorString(me));
        }
        ix->shadow_rows = rows_al;
        HIP_TRY(hipMemsetAsync(ix->shadow, 0, (size_t)rows_al * ix->dpad * 2, st));  // rows beyond the count are masked, their bytes only have to be defined
        first = 0; m = n;
    }
    HIP_TRY(ix->shadow_ready.ensure());
    if (m > 0) {
        const dim3 grid((unsigned)((m + 3) / 4)), block(256);
        uint2* sh = reinterpret_cast<uint2*>(ix->shadow.get());
        const int rc = with_dtype(ix->dtype, [&](auto dt) {
            return launch_kernel<shadow_from_rows_kernel<dt>>(grid, block, 0, st, ix->rows, first, m, ix->dpad, sh);
        });
        if (rc != 0) return rc;
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(ix->shadow_ready, st));
    ix->shadow_stream = st;
    ix->shadow_epoch = ix->epoch;
    ix->dirty16_lo = ix->dirty16_hi = 0;
    ix->stat_shadow_builds++;
    return CODD_KNN_OK;
}

// The int8 shadow is derived data: (re)built from the stored rows on the searching stream whenever rows have been
// written since the last build.  Other streams that search before the build has finished wait for it on the device.
int ensure_shadow8(codd_knn_index* ix, hipStream_t st) {
    const int64_t n = ix->count;
    const int dpad8 = dpad8_of(shape_of(ix));
    if (ix->shadow8_epoch == ix->epoch && ix->shadow8) {
        if (st != ix->shadow8_stream && ix->shadow8_ready) HIP_TRY(hipStreamWaitEvent(st, ix->shadow8_ready, 0));
        return CODD_KNN_OK;
    }
    const int64_t need = tiles_of(n) * kTileRows;
    int64_t first = ix->dirty_lo, m = ix->dirty_hi - ix->dirty_lo;  // rows to (re)quantise
    if (first + m > n) m = n > first ? n - first : 0;  // (never past the count: the allocation below is only checked against it)
    if (!ix->eps_r_bits) {
        HIP_TRY(ix->eps_r_bits.reset(2));
        HIP_TRY(hipMemsetAsync(ix->eps_r_bits, 0, 2 * sizeof(unsigned), st));
    }
    const bool norms = !metric_is_cosine(ix);  // (an ip or l2 index comes here through its filter leg only: the norms follow the shadow)
    if (norms && !ix->rmax_bits) {
        HIP_TRY(ix->rmax_bits.reset(1));
        HIP_TRY(hipMemsetAsync(ix->rmax_bits, 0, sizeof(unsigned), st));
    }
    if (need > ix->shadow8_rows) {
        // (every stream that may still read the old allocation has to be done with it)
        int rcw;
        if ((rcw = wait_searching_streams(ix)) != 0) return rcw;
        (void)ix->shadow8.reset();
        (void)ix->rscale.reset();
        (void)ix->bmeta.reset();
        ix->shadow8_rows = 0;
        const int64_t rows = need + need / 8;  // head room: appends do not reallocate every time
        const int64_t rows_al = tiles_of(rows) * kTileRows;
        // the three belong together: built in locals, handed over together (a failure leaves the index without an int8 shadow, not with a third of one)
        DevBuf<uint4> s8;
        DevBuf<float> rs;
        DevBuf<float2> bm;
        HIP_TRY(s8.reset(rows_al * dpad8 / (int64_t)sizeof(uint4)));
        HIP_TRY(rs.reset(rows_al));
        HIP_TRY(bm.reset(rows_al / 32 + 64));  // (+64: a wave's DMA reads 32 blocks from a tile's first one)
        if (norms) {
            (void)ix->rnorm2.reset();
            HIP_TRY(ix->rnorm2.reset(rows_al));
        }
        ix->shadow8 = std::move(s8);
        ix->rscale = std::move(rs);
        ix->bmeta = std::move(bm);
        HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)ix->bmeta.get(), (int)0x7fc00000, (size_t)(rows_al / 32 + 64) * 2, st));  // NaN: no such block yet
        ix->shadow8_rows = rows_al;
        // rows beyond the count are masked (row < n), their bytes only have to be defined
        HIP_TRY(hipMemsetAsync(ix->shadow8, 0, (size_t)rows_al * dpad8, st));
        HIP_TRY(hipMemsetAsync(ix->eps_r_bits, 0, 2 * sizeof(unsigned), st));
        first = 0; m = n;  // a fresh allocation holds nothing yet
    }
    HIP_TRY(ix->shadow8_ready.ensure());
    if (m > 0) {
        // Whole 32-row blocks (one scale per block): the rows that share a block with the dirty range are quantised again,
        // with the block's new scale, and the block's error norm is measured again.
        const int64_t last = first + m;
        first = first / 32 * 32;
        m = (last + 31) / 32 * 32 - first;
        const dim3 grid((unsigned)(m / 32)), block(256);
        uint4* s8 = ix->shadow8;
        const int rc = with_dtype(ix->dtype, [&](auto dt) {
            return launch_kernel<shadow8_from_rows_kernel<dt>>(grid, block, 0, st, ix->rows, first, n, ix->dpad, dpad8, s8, ix->rscale, ix->bmeta);
        });
        if (rc != 0) return rc;
        HIP_TRY(hipGetLastError());
        // the device-wide maximum of the block error norms, over the rows stored now (not a running maximum)
        hipLaunchKernelGGL(eps_max_kernel, dim3(1), dim3(1024), 0, st, ix->bmeta, (n + 31) / 32, ix->eps_r_bits, ix->knobs.shadow8_max_eps);
        HIP_TRY(hipGetLastError());
        if (norms) {  // the same rows' sums of squares, and the bound on every row's norm
            const int64_t mn = first + m > n ? n - first : m;
            const int rcn = with_dtype(ix->dtype, [&](auto dt) {
                return launch_kernel<row_sqnorm_kernel<dt>>(dim3((unsigned)((mn + 3) / 4)), block, 0, st, ix->rows, first, mn, ix->dpad, ix->rnorm2, ix->rmax_bits);
            });
            if (rcn != 0) return rcn;
            HIP_TRY(hipGetLastError());
        }
    }
    {
        // i8_tile_kernel reads whole tiles of scales: rows past the count carry NaN (`acc * NaN >= thr` is false for every
        // threshold, so its epilogue needs no row < count test).  Rows appended later get real scales from the build above.
        const int64_t pad = need - n;
        if (pad > 0) HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)(ix->rscale + n), (int)0x7fc00000, (size_t)pad, st));
    }
    HIP_TRY(hipEventRecord(ix->shadow8_ready, st));
    if (!ix->eps_r_host) {
        HIP_TRY(ix->eps_r_host.reset(2));
        ix->eps_r_host[0] = 0.0f;
        ix->eps_r_host[1] = 0.0f;
        HIP_TRY(ix->eps_r_copied.ensure());
    }
    HIP_TRY(hipMemcpyAsync(ix->eps_r_host, ix->eps_r_bits, 2 * sizeof(float), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipEventRecord(ix->eps_r_copied, st));
    ix->shadow8_stream = st;
    ix->shadow8_epoch = ix->epoch;
    ix->dirty_lo = ix->dirty_hi = 0;
    ix->stat_shadow8_builds++;
    return CODD_KNN_OK;
}

// the arguments gemm_filter_kernel and i8_tile_kernel share, in their order; each launch expands them into its kernel's list
struct FilterArgs {
    const uint4* shadow;
    const uint4* qfrag;
    int64_t n;
    int nsteps;
    int64_t ntiles_run, tile_stride;
    const float* thr;
    u64* bucket_key;
    u64* hits;
    unsigned* hit_cnt;
    int cap_q;
    unsigned* flags;
    const float* rscale;  // int8 operands only
    const float* qscale;
    const float2* bmeta;  // i8_tile_kernel only
    float eb_scale;
    const float* rnorm2 = nullptr;  // sqd_filter_kernel only: the rows' and the queries' sums of squares
    const float* qn2 = nullptr;
    int skip_d = 0;                 // i8_tile_kernel only: d of the sample cascade's launch B (0: every run-tile)
};

// one launch of program `p` in pass MODE (MODE_SAMPLE or MODE_FILTER)
template <int MODE>
int launch_filter_program(const FilterProgram& p, dim3 grid, hipStream_t st, const FilterArgs& a) {
    using No = std::false_type;
    using Yes = std::true_type;
    const dim3 block(kFilterThreads);
    auto gemm = [&](auto nbq, auto el, auto res) {
        return launch_kernel<gemm_filter_kernel<MODE, nbq, el, res>>(grid, block, filter_lds_bytes(MODE), st, a.shadow, a.qfrag, a.n, a.nsteps,
                                                                     a.ntiles_run, a.tile_stride, a.thr, a.bucket_key, a.hits, a.hit_cnt, a.cap_q,
                                                                     a.flags, (float*)nullptr, a.rscale, a.qscale);
    };
    auto tile = [&](auto ts, auto nqb, auto res, auto f16) {
        return launch_kernel<i8_tile_kernel<MODE, ts, nqb, res, f16>>(grid, block, i8_lds_bytes(MODE), st, a.shadow, a.qfrag, a.n, a.nsteps,
                                                                      a.ntiles_run, a.tile_stride, a.thr, a.bucket_key, a.hits, a.hit_cnt, a.cap_q,
                                                                      a.flags, a.rscale, a.qscale, a.bmeta, a.eb_scale, a.skip_d);
    };
    if (p.sqd) {
        return with_nbq(p.nbq, [&](auto nbq) {
            return launch_kernel<sqd_filter_kernel<MODE, nbq>>(grid, block, filter_lds_bytes(MODE), st, a.shadow, a.qfrag, a.n, a.nsteps, a.ntiles_run,
                                                               a.tile_stride, a.thr, a.bucket_key, a.hits, a.hit_cnt, a.cap_q, a.flags, (float*)nullptr, a.rscale,
                                                               a.qscale, a.rnorm2, a.qn2);
        });
    }
    if (p.family == FilterProgram::TILE) {
        return with_int<4, 8>(p.nbq, "bad query block count%s", [&](auto nbq) {
            const IntC<2 * decltype(nbq)::value> nqb;
            if constexpr (MODE == MODE_SAMPLE) {
                // (the sample pass keeps the generic program: its tile-structured instantiations — the static six-step one too, tried in round 3 —
                //  spill inside the loop: the fold's registers on top of two corpus ring slots in flight)
                return p.res ? tile(IntC<0>{}, nqb, Yes{}, No{}) : tile(IntC<0>{}, nqb, No{}, No{});
            } else if (p.sweep) {  // (filter_program: ts = 3, 16 query blocks of 16, staged)
                if constexpr (decltype(nqb)::value == 16) {
                    return launch_kernel<i8_sweep_kernel<16>>(grid, block, i8_lds_bytes(MODE), st, a.shadow, a.qfrag, a.n, a.nsteps, a.ntiles_run, a.tile_stride, a.thr,
                                                              a.bucket_key, a.hits, a.hit_cnt, a.cap_q, a.flags, a.rscale, a.qscale, a.bmeta, a.eb_scale, a.skip_d);
                } else {
                    return fail(CODD_KNN_EINVAL, "bad tile program%s");
                }
            } else if (p.res) {  // (the pair programs stage the query block)
                return with_int<0, 1>(p.ts, "bad tile program%s", [&](auto ts) { return tile(ts, nqb, Yes{}, No{}); });
            } else {
                return with_int<0, 1, 2, 3>(p.ts, "bad tile program%s", [&](auto ts) { return tile(ts, nqb, No{}, No{}); });
            }
        });
    }
    if constexpr (MODE == MODE_FILTER) {
        if (p.family == FilterProgram::TILE_F16)
            return with_int<2, 3, 4>(p.ts, "bad tile program%s", [&](auto ts) { return tile(ts, IntC<16>{}, No{}, Yes{}); });
    }
    // GEMM (and TILE_F16's sample pass: 8 query blocks, 2-byte operands)
    if (p.el == 0) return with_nbq(p.nbq, [&](auto nbq) { return gemm(nbq, IntC<0>{}, IntC<0>{}); });
    if (p.res == 2) return gemm(IntC<4>{}, IntC<1>{}, IntC<2>{});
    return with_nbq(p.nbq, [&](auto nbq) { return p.res ? gemm(nbq, IntC<1>{}, IntC<1>{}) : gemm(nbq, IntC<1>{}, IntC<0>{}); });
}

// The list-driven exact-scan fallback: at most one workgroup per compute unit (bounds the queue's partial buffer) and the
// buffer of its per-block partials.
int fallback_geometry(codd_knn_index* ix, int k, int64_t* blocks, int64_t* stride_q) {
    int niter, rc;
    if ((rc = scan_geometry(ix, ix->count, &niter, blocks)) != 0) return rc;
    if (*blocks > ix->num_cus) *blocks = ix->num_cus;
    *stride_q = *blocks * k;
    HIP_TRY(ix->fb_partial.ensure((int64_t)kTileQ * *stride_q));
    return CODD_KNN_OK;
}

// exact-scan fallback for the queries a pass queued (normally none), entirely on the device and in ONE launch: the scan walks
// the queue (an empty queue costs one empty launch), its last block merges the per-block partials and writes each answer into
// its query's slot.  No host round trip: the whole search stays asynchronous on `st`.
int listed_fallback(codd_knn_index* ix, const float* qn, int k, uint32_t row_base, u64* keys_out, float* dist_out, int64_t* rows_out,
                    hipStream_t st, const uint32_t* deny, int metric = kMetricDot) {
    int64_t blocks, stride_q;
    int rc;
    if ((rc = fallback_geometry(ix, k, &blocks, &stride_q)) != 0) return rc;
    if (metric == kMetricL2) {  // the list-driven squared-distance scan (the dense l2 scans take no query list)
        FilterCtl* c = ix->ctl;
        {
            EvScope ev(ix, EV_SCAN, st);
            rc = with_row_form(ix, k, "row too wide for the listed squared-distance scan%s", [&](auto dt, auto ni, auto sl) {
                if constexpr (decltype(ni)::value == kWideRows) {
                    return fail(CODD_KNN_ENOTSUP, "row too wide for the listed squared-distance scan%s");
                } else {
                    return launch_kernel<sqd_listed_scan_kernel<dt, ni, sl>>(dim3((unsigned)blocks), dim3(256), (size_t)4 * 4 * decltype(sl)::value * kWave * sizeof(u64), st,
                                                                            ix->rows, ix->count, ix->dpad, qn, k, row_base, ix->fb_partial, stride_q, c->fb_list,
                                                                            &c->fb_count, &c->fb_done, keys_out, dist_out, rows_out, &ix->dstats[2], deny);
                }
            });
        }
        if (rc != 0) return rc;
        HIP_TRY(hipGetLastError());
        return CODD_KNN_OK;
    }
    ScanArgs a{ix->rows, ix->count, ix->dpad, qn, 0, k, row_base, ix->fb_partial, stride_q, ix->ctl->fb_list, &ix->ctl->fb_count};
    a.merge_done = &ix->ctl->fb_done;
    a.merged_keys = keys_out;
    a.merged_dist = dist_out;
    a.merged_rows = rows_out;
    a.count_total = &ix->dstats[2];
    a.dead = deny;
    {
        EvScope ev(ix, EV_SCAN, st);
        rc = launch_scan(ix->dtype, 8, niter_of(shape_of(ix)), dim3((unsigned)blocks), st, a);
    }
    if (rc != 0) return rc;
    HIP_TRY(hipGetLastError());
    return CODD_KNN_OK;
}

// one pass of <= 256 queries through sample -> threshold -> filter -> finalize (+ exact fallback)
// keys_out and / or (dist_out, rows_out): what the caller wants written per query (any may be null)
int filter_pass(codd_knn_index* ix, const float* qn, int nq, int k, uint32_t row_base, u64* keys_out, float* dist_out, int64_t* rows_out,
                hipStream_t st, const uint32_t* deny, bool prepared = false, bool use8 = false) {
    const int64_t n = ix->count;
    IndexShape shape = shape_of(ix);
    // ("debug_num_cus": the pass's plan and its sample and filter launches count this many compute units — a small corpus then gives a workgroup several tiles)
    const int num_cus = ix->debug_num_cus > 0 ? ix->debug_num_cus : ix->num_cus;
    shape.num_cus = num_cus;
    const FilterKnobs& knobs = ix->knobs;
    const int nsteps = use8 ? dpad8_of(shape) / 128 : ix->dpad / 64;
    const uint4* shadow = use8 ? ix->shadow8 : ix->shadow;
    const uint4* qfrag = use8 ? ix->qfrag8 : ix->qfrag;
    const float* slack_q = use8 ? ix->qmeta + 256 : nullptr;  // int8: 2*eps per query, written by prep_queries8_kernel
    const float* rscale = use8 ? ix->rscale : nullptr;
    const float* qscale = use8 ? ix->qmeta : nullptr;
    const bool cosine = metric_is_cosine(ix);
    if (use8) ix->stat_shadow8_passes++;
    const int64_t ntiles = tiles_of(n);
    const int slots = k <= 64 ? 1 : 2;
    const float eps = filter_eps(ix);
    int rc;
    ix->stat_filter_passes++;

    if (!prepared) {  // (a batch of <= 256 queries arrives with its fragments and a cleared control block: prep_queries_kernel)
        hipLaunchKernelGGL(qfrag_kernel, dim3((kTileQ * (ix->dpad / 8) + 255) / 256), dim3(256), 0, st, qn, nq, ix->dpad, ix->qfrag,
                           reinterpret_cast<unsigned*>(ix->ctl.get()), (int)(sizeof(FilterCtl) / 4));
        HIP_TRY(hipGetLastError());
    }

    const FilterProgram prog = filter_program(knobs, shape, nq, nsteps, use8);
    if (prog.family == FilterProgram::TILE) ix->stat_i8v2_passes++;
    if (prog.family == FilterProgram::TILE_F16) ix->stat_f16_tile_passes++;
    // sample: every `stride`-th tile; or the sample cascade (search_plan.h: cascade_plan), whose first sample A0 is one round from tile a0_first on
    const int64_t ts_plain = sample_tile_count(knobs, shape, ntiles, k, use8, prog.nbq);
    const CascadePlan cas = use8 ? cascade_plan(knobs, shape, prog, ntiles, k, ts_plain) : CascadePlan();
    const int64_t ts = cas.on ? cas.a0_tiles : ts_plain;
    const int64_t stride = cas.on ? cas.a0_stride : ntiles / ts;
    ix->stat_last_cascade_d = cas.on ? cas.d : 0;
    ix->stat_last_sweep = prog.sweep ? 1 : 0;
    if (prog.sweep) ix->stat_sweep_passes++;
    if (cas.on) ix->stat_cascade_passes++;
    {
        LastPass& lp = ix->last;
        lp.valid = true;
        lp.family = (int)prog.family; lp.nbq = prog.nbq; lp.ts = prog.ts; lp.res = prog.res; lp.el = prog.el; lp.sqd = prog.sqd ? 1 : 0;
        lp.nq = nq; lp.k = k; lp.n = n; lp.sample_tiles = ts; lp.sample_stride = stride; lp.hit_cap = ix->knobs.hit_cap_q;
        lp.eps = eps;
        lp.per_block_filter = prog.family == FilterProgram::TILE && (ix->knobs.per_block & 1) ? 1 : 0;
        lp.per_block_finalize = slack_q && (ix->knobs.per_block & 2) && cosine ? 1 : 0;
        lp.cascade_d = cas.on ? cas.d : 0;
    }
    // one launch of the pass's filter program over run-tiles [0, ntiles_run) of stride tile_stride, appending to the pass's hit lists
    auto filter_launch = [&](int64_t ntiles_run, int64_t tile_stride, int64_t grid, int skip_d) -> int {
        const dim3 g((unsigned)grid);
        FilterArgs fa{shadow, qfrag, n, nsteps, ntiles_run, tile_stride, ix->thr, nullptr, ix->hits, ix->ctl->hit_cnt, ix->knobs.hit_cap_q, ix->ctl->flags, rscale, qscale, nullptr, 0.0f};
        fa.skip_d = skip_d;
        if (prog.sqd) { fa.rnorm2 = ix->rnorm2; fa.qn2 = ix->qmeta + 512; }
        if (prog.family == FilterProgram::TILE) {
            // the per-block bound (per_block & 1): thr0[q] and the blocks' error norms
            fa.thr = (ix->knobs.per_block & 1) ? ix->thr + kTileQ : ix->thr;
            fa.bmeta = ix->bmeta;
            fa.eb_scale = (ix->knobs.per_block & 1) ? 1.0f : 0.0f;
#ifdef CODD_I8_EXP_STAMPS  // (diagnostic build: the filter pass writes its per-wave phase stamps over the sample's bucket keys, which the anchor kernels have consumed)
            if (tile_stride == 1) fa.bucket_key = ix->bucket_max;   // (the main launch; the cascade's A1 runs before the re-anchor has read the keys)
#endif
        } else if (prog.family == FilterProgram::TILE_F16) {
            // (thr doubles as the 256 readable bytes the kernel's per-tile metadata request needs; fp16 operands carry no scales)
            fa.bmeta = reinterpret_cast<const float2*>(ix->thr.get());
        }
        return launch_filter_program<MODE_FILTER>(prog, g, st, fa);
    };
    // A0 reads the corpus from row slot `row0` on (cas.a0_first whole tiles in: none of its tiles is one of A1's): the sample program and
    // anchor_thr_kernel are given every per-row array from there, so their row numbers count from row0 — reanchor_thr_kernel adds it back
    const int64_t row0 = cas.on ? cas.a0_first * kTileRows : 0;
    {
        // (the cascade: one event pair from A0 to the re-anchor, everything that fixes the thresholds; else the sample launch alone, as ever)
        EvScope ev(ix, EV_SAMPLE, st);
        {
            const dim3 g((unsigned)(ts < num_cus ? ts : num_cus));
            FilterArgs sa{shadow + row0 * (dpad8_of(shape) / 16), qfrag, n - row0, nsteps, ts, stride, nullptr, ix->bucket_max, nullptr, nullptr, 0, nullptr,
                          rscale ? rscale + row0 : nullptr, qscale, nullptr, 1.0f};
            if (prog.sqd) { sa.rnorm2 = ix->rnorm2; sa.qn2 = ix->qmeta + 512; }
            if ((rc = launch_filter_program<MODE_SAMPLE>(prog, g, st, sa)) != 0) return rc;
        }
        if (!cas.on) ev.stop();
        HIP_TRY(hipGetLastError());
        // thresholds anchored on the exact scores of the k best sampled rows (anchor_thr_kernel)
        const unsigned char* rows_s = ix->rows.get() + row0 * (int64_t)ix->dpad * (int64_t)elem_size(ix->dtype);
        const uint32_t* deny_s = deny ? deny + row0 / 32 : nullptr;
        rc = with_row_form(ix, k, "row too wide for the threshold kernel%s", [&](auto dt, auto ni, auto sl) {
            if constexpr (decltype(ni)::value != kWideRows) {
                if (prog.sqd)
                    return launch_kernel<sqd_thr_kernel<dt, ni, sl>>(dim3(kTileQ), dim3(kAnchorWaves * kWave), 0, st, ix->bucket_max, ts, nq, k, ix->rows, ix->dpad,
                                                                            qn, slack_q, ix->thr, deny);
            }
            return launch_kernel<anchor_thr_kernel<dt, ni, sl>>(dim3(kTileQ), dim3(kAnchorWaves * kWave), 0, st, ix->bucket_max, ts, nq, k, rows_s,
                                                                ix->dpad, qn, eps, slack_q, ix->thr, use8 ? ix->thr + kTileQ : nullptr, deny_s);
        });
        if (rc != 0) return rc;
        HIP_TRY(hipGetLastError());
        if (cas.on) {
            // A1: the filter program over tiles 0, d + 1, ... with the provisional thresholds (timed with the sample: it is what fixes the thresholds)
            if ((rc = filter_launch(cas.a1_tiles, cas.d + 1, cas.a1_tiles < num_cus ? cas.a1_tiles : num_cus, 0)) != 0) return rc;
            HIP_TRY(hipGetLastError());
            rc = with_row_form(ix, k, "row too wide for the threshold kernel%s", [&](auto dt, auto ni, auto sl) {
                return launch_kernel<reanchor_thr_kernel<dt, ni, sl>>(dim3(nq), dim3(kAnchorWaves * kWave), 0, st, ix->bucket_max, ts, (unsigned)row0, ix->hits,
                                                                      ix->ctl->hit_cnt, ix->knobs.hit_cap_q, nq, k, ix->rows, ix->dpad, qn, eps, slack_q, ix->thr,
                                                                      ix->thr + kTileQ, deny);
            });
            if (rc != 0) return rc;
            HIP_TRY(hipGetLastError());
        }
    }
    {
        // the main launch: every tile, or (the cascade's launch B) every tile that is no multiple of d + 1, on a grid d divides
        EvScope ev(ix, EV_FILTER, st);
        if ((rc = filter_launch(ntiles, 1, cas.on ? cas.G : (ntiles < num_cus ? ntiles : num_cus), cas.on ? cas.d : 0)) != 0) return rc;
    }
    HIP_TRY(hipGetLastError());
    const int niter = niter_of(shape);
    // (an int8 pass of a handful of queries: several workgroups per query, their lists merged below)
    const int nparts = finalize_parts(use8, nq);
    ix->stat_last_finalize_parts = nparts;
    if (nparts > 1) HIP_TRY(ix->partial.ensure((int64_t)nq * nparts * k));
    const float2* bm = slack_q && (ix->knobs.per_block & 2) && cosine ? ix->bmeta : nullptr;  // (the int8 passes: slack per 32-row block; ip, l2: the device-wide bound)
    FilterCtl* c = ix->ctl;
    // one list slot per lane and one workgroup per query (the large batches): finalize and the exact-scan fallback share ONE
    // launch — the scan workgroups derive the queue from the hit counters and leave at once when it is empty
    if (slots == 1 && nparts == 1 && ix->knobs.fuse_fallback && niter <= 4 && !(ix->dtype != DT_F32 && niter == 4) && !prog.sqd) {  // (2-byte rows above 1536 elements: the fused kernel spills; wide rows take the separate fallback launch)
        int64_t blocks, stride_q;
        if ((rc = fallback_geometry(ix, k, &blocks, &stride_q)) != 0) return rc;
        EvScope ev(ix, EV_FINALIZE, st);
        const dim3 grid((unsigned)(nq + blocks), 1);
        const size_t lds = (size_t)(kFinThreads / kWave) * 4 * kWave * sizeof(u64);   // the scan role's lists: 8 waves x 4 queries x 64 keys
        rc = with_dtype(ix->dtype, [&](auto dt) {
            return with_niter(niter, "row too wide for the finalize kernel%s", [&](auto ni) {
                if constexpr (decltype(ni)::value == kWideRows) {
                    return fail(CODD_KNN_ENOTSUP, "row too wide for the finalize kernel%s");
                } else {
                    return launch_kernel<finalize_fb_kernel<decltype(dt)::value, ni>>(
                        grid, dim3(kFinThreads), lds, st, ix->rows, ix->dpad, qn, ix->hits, c->hit_cnt, ix->knobs.hit_cap_q, c->flags, k, 2.0f * eps, row_base,
                        keys_out, ix->dstats, slack_q, (u64*)nullptr, dist_out, rows_out, bm, nq, n, ix->fb_partial, stride_q, &c->fb_done, deny);
                }
            });
        });
        if (rc != 0) return rc;
        HIP_TRY(hipGetLastError());
        return CODD_KNN_OK;
    }
    {
        EvScope ev(ix, EV_FINALIZE, st);
        rc = with_row_form(ix, k, "row too wide for the finalize kernel%s", [&](auto dt, auto ni, auto sl) {
            if constexpr (decltype(ni)::value != kWideRows) {
                if (prog.sqd)
                    return launch_kernel<sqd_fin_kernel<dt, ni, sl>>(dim3(nq, nparts), dim3(kFinThreads), 0, st, ix->rows, ix->dpad, qn, ix->hits, c->hit_cnt,
                                                                          ix->knobs.hit_cap_q, c->flags, k, row_base, keys_out, &c->fb_count, c->fb_list, ix->dstats, slack_q,
                                                                          ix->partial, dist_out, rows_out, deny);
            }
            return launch_kernel<finalize_kernel<dt, ni, sl>>(dim3(nq, nparts), dim3(kFinThreads), 0, st, ix->rows, ix->dpad, qn, ix->hits, c->hit_cnt,
                                                              ix->knobs.hit_cap_q, c->flags, k, 2.0f * eps, row_base, keys_out, &c->fb_count, c->fb_list,
                                                              ix->dstats, slack_q, ix->partial, dist_out, rows_out, bm, deny);
        });
    }
    if (rc != 0) return rc;
    HIP_TRY(hipGetLastError());
    const int km = prog.sqd ? kMetricL2 : kMetricDot;
    if (nparts > 1 && (rc = launch_merge(ix->partial, nq, (int64_t)nparts * k, (int64_t)nparts * k, k, keys_out, dist_out, rows_out, st, nullptr, nullptr, nullptr, 0, 0, km)) != 0)
        return rc;
    return listed_fallback(ix, qn, k, row_base, keys_out, dist_out, rows_out, st, deny, km);
}

// ---- one launch for a single query (small_batch_kernel) + the (normally empty) list-driven fallback scan ----
template <int DT, int NS>
int launch_small_batch(int64_t nunits, hipStream_t st, const codd_knn_index* ix, const float* dev_queries, int k, uint32_t row_base, u64* cand,
                       u64* out_keys, float* out_dist, int64_t* out_rows, const uint32_t* deny) {
    constexpr int E = DT == DT_F32 ? 4 : 8;
    constexpr int NITER = (NS * 128 / E + kWave - 1) / kWave;  // chunks of the PADDED row per lane (dpad <= NS * 128)
    constexpr int kWavesPerWg = kSbThreads / kWave;
    // one round of workgroups: as many as are resident at once (the last one to arrive answers the query)
    static std::atomic<int> per_cu{0};
    int nb = per_cu.load(std::memory_order_relaxed);
    if (nb == 0) {
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, (const void*)&small_batch_kernel<DT, NITER, NS>, kSbThreads, 0) != hipSuccess || nb < 1) nb = 1;
        if (nb > 2) nb = 2;
        (void)hipGetLastError();
        per_cu.store(nb, std::memory_order_relaxed);
    }
    int64_t G = (int64_t)nb * ix->num_cus;
    if (G * kWavesPerWg > nunits) G = (nunits + kWavesPerWg - 1) / kWavesPerWg;
    const dim3 grid((unsigned)G);
    u64* dropmax = cand + G * kWavesPerWg * kSbKeep;
    FilterCtl* c = ix->ctl;
    return launch_kernel<small_batch_kernel<DT, NITER, NS>>(grid, dim3(kSbThreads), 0, st, ix->shadow8, ix->bmeta, ix->rows, ix->count, ix->dim, ix->dpad,
                                                            dev_queries, k, row_base, ix->eps_r_bits, ix->qn, cand, dropmax, &c->sb_ticket, &c->fb_count,
                                                            c->fb_list, out_keys, out_dist, out_rows, ix->dstats, deny);
}
int small_batch_search(codd_knn_index* ix, const float* dev_queries, int B, int k, uint32_t row_base, u64* out_keys, float* out_dist, int64_t* out_rows,
                       hipStream_t st, const uint32_t* deny) {
    (void)B;
    const int ns = dpad8_of(shape_of(ix)) / 128;
    const int64_t n = ix->count;
    constexpr int kWavesPerWg = kSbThreads / kWave;
    const int64_t nunits = (n + 15) / 16;
    int rc;
    HIP_TRY(ix->sb_cand.ensure((int64_t)(2 * ix->num_cus) * kWavesPerWg * (kSbKeep + 1)));
    u64* cand = ix->sb_cand;
    ix->stat_small_batch++;
    {
        EvScope ev(ix, EV_FILTER, st);
        rc = with_dtype(ix->dtype, [&](auto dt) {
            return with_int<3, 4, 6, 8>(ns, "small batch: unsupported row width%s", [&](auto nsc) {
                return launch_small_batch<decltype(dt)::value, nsc>(nunits, st, ix, dev_queries, k, row_base, cand, out_keys, out_dist, out_rows, deny);
            });
        });
    }
    if (rc != 0) return rc;
    HIP_TRY(hipGetLastError());
    // a query the margin test could not clear (normally none): the list-driven exact scan, its last block merges
    return listed_fallback(ix, ix->qn, k, row_base, out_keys, out_dist, out_rows, st, deny);
}

int launch_prep_raw(codd_knn_index* ix, const float* dev_queries, int nq, float* qn, hipStream_t st) {
    hipLaunchKernelGGL(prep_queries8_raw_kernel, dim3(kTileQ / 4), dim3(256), 0, st, dev_queries, nq, ix->dim, ix->dpad, dpad8_of(shape_of(ix)), qn,
                       reinterpret_cast<uint32_t*>(ix->qfrag8.get()), ix->qmeta, ix->eps_r_bits, ix->rmax_bits, reinterpret_cast<unsigned*>(ix->ctl.get()),
                       (int)(sizeof(FilterCtl) / 4), ix->metric == CODD_KNN_METRIC_L2 ? 1 : 0);
    HIP_TRY(hipGetLastError());
    return CODD_KNN_OK;
}

// what an int8 pass of an ip or l2 index needs beside the rows: the workspace, the shadow with the rows' norms, the query buffers
int ensure_space_filter(codd_knn_index* ix, hipStream_t st) {
    int rc;
    if ((rc = ensure_filter_workspace(ix)) != 0) return rc;
    if ((rc = ensure_shadow8(ix, st)) != 0) return rc;
    HIP_TRY(ix->qfrag8.ensure((int64_t)kTileQ * (dpad8_of(shape_of(ix)) / 16)));
    if (!ix->qmeta) HIP_TRY(ix->qmeta.reset(1024));
    return CODD_KNN_OK;
}

// ... and the search: ceil(B / 256) passes, each with its own preparation.  The survivor watch, the cooldown and the eps_r switch to
// the 2-byte filter never engage: they are unit-norm quantities, and the 2-byte filter's analytic bound does not hold here.
int space_filter_search(codd_knn_index* ix, const float* dev_queries, int B, int k, uint32_t row_base, u64* out_keys, float* out_dist, int64_t* out_rows,
                        hipStream_t st, const uint32_t* deny) {
    int rc;
    if ((rc = ensure_space_filter(ix, st)) != 0) return rc;
    for (int q0 = 0; q0 < B; q0 += kTileQ) {
        const int nq = B - q0 < kTileQ ? B - q0 : kTileQ;
        float* qn = ix->qn + (int64_t)q0 * ix->dpad;
        if ((rc = launch_prep_raw(ix, dev_queries + (int64_t)q0 * ix->dim, nq, qn, st)) != 0) return rc;
        if ((rc = filter_pass(ix, qn, nq, k, row_base, out_keys ? out_keys + (int64_t)q0 * k : nullptr, out_dist ? out_dist + (int64_t)q0 * k : nullptr,
                              out_rows ? out_rows + (int64_t)q0 * k : nullptr, st, deny, true, true)) != 0)
            return rc;
    }
    return CODD_KNN_OK;
}

// the index looks at its own device counters now and then (one look in flight; FilterWatch::due says when: the copy is a launch
// of its own on the searching stream)
int after_filter_search(codd_knn_index* ix, int B, bool use8, hipStream_t st) {
    FilterWatch& w = ix->watch;
    (use8 ? w.q8 : w.q16) += B;
    if (ix->knobs.shadow8_enabled && !w.pending && ix->dstats && FilterWatch::due(ix->stat_searches)) {
        if (!ix->watch_host) {
            HIP_TRY(ix->watch_host.reset(4));
            HIP_TRY(ix->watch_copied.ensure());
        }
        HIP_TRY(hipMemcpyAsync(ix->watch_host, ix->dstats, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipEventRecord(ix->watch_copied, st));
        w.sent();
    }
    return CODD_KNN_OK;
}

// the two asynchronous read-backs a search looks at before it plans: the int8 shadow's worst quantisation error (ensure_shadow8)
// and the filter watch's counters (after_filter_search).  Neither is waited for.
void poll_read_backs(codd_knn_index* ix) {
    if (ix->eps_r_copied) {
        if (hipEventQuery(ix->eps_r_copied) == hipSuccess) {
            ix->eps_r_known = ix->eps_r_host[0];
            ix->wide_blocks_known = (int64_t)reinterpret_cast<const unsigned*>(ix->eps_r_host.get())[1];
        }
        else (void)hipGetLastError();  // "not ready" must not surface in a later error check
    }
    if (ix->watch.pending && ix->watch_copied) {
        if (hipEventQuery(ix->watch_copied) == hipSuccess) ix->watch.observe(ix->watch_host[1], ix->watch_host[2], ix->epoch, ix->knobs);
        else (void)hipGetLastError();
    }
}

// the whole shard-local search: validate, look at the read-backs, plan (search_plan.h: plan_search decides the route, nothing below
// does), make sure of the buffers the plan names, launch the route.
// deny: the rows no answer may hold — ix->dead_bits, or, `masked`, the ~allow | dead of a masked search's dense route (DESIGN.md
// §15).  A masked search says nothing about the corpus: it neither feeds the filter watch nor uses up a cooldown.
int search_impl(codd_knn_index* ix, const float* dev_queries, int B, int k, uint32_t row_base, u64* out_keys,
                float* out_dist, int64_t* out_rows, hipStream_t st, const uint32_t* deny, bool masked = false) {
    if (!ix) return fail(CODD_KNN_EINVAL, "null index%s");
    if (!dev_queries) return fail(CODD_KNN_EINVAL, "null queries%s");
    if (B < 1 || B > CODD_KNN_MAX_BATCH) return fail(CODD_KNN_EINVAL, "B out of range [1,1024]%s");
    if (k < 1 || k > CODD_KNN_MAX_K) return fail(CODD_KNN_EINVAL, "k out of range [1,128]%s");
    DeviceGuard guard(ix->device);
    ix->stat_searches++;
    int rc;
    HIP_TRY(ix->qn.ensure((int64_t)B * ix->dpad));
    HIP_TRY(ix->keys_tmp.ensure((int64_t)B * k));
    if ((rc = wait_rows(ix, st)) != 0) return rc;

    poll_read_backs(ix);
    const bool cooling = ix->watch.cooldown_left > 0;
    const IndexShape shape = shape_of(ix);
    SearchPlan plan = plan_search(ix->knobs, shape, B, k, cooling, ix->eps_r_known, ix->wide_blocks_known);
    if (cooling && plan.filters() && !masked) ix->watch.cooldown_left--;

    // the shadow the plan names (the space filter's route makes sure of its own)
    if (plan.filters() && !plan.use8) {
        // the 2-byte filter: its shadow is allocated by the first search that needs it.  When HBM cannot hold it the plan is
        // downgraded (SearchPlan::without_shadow16) and the failed allocation is not retried until rows change.
        if ((rc = ensure_filter_workspace(ix)) != 0) return rc;
        rc = ensure_shadow(ix, st);
        if (rc == CODD_KNN_ENOMEM) plan.without_shadow16();
        else if (rc != 0) return rc;
    }
    if (plan.filters() && plan.use8) {
        if ((rc = ensure_filter_workspace(ix)) != 0) return rc;
        if ((rc = ensure_shadow8(ix, st)) != 0) return rc;
    }

    // the filter passes write what the caller asked for — packed keys (the shard-local half of a sharded search) and / or
    // (distance, row) — straight from finalize: no unpack launch behind them
    const int dpad8 = dpad8_of(shape);
    switch (plan.route) {
        case SearchPlan::SPACE_FILTER:  // (ceil(B / 256) passes, each with its own preparation)
            return space_filter_search(ix, dev_queries, B, k, row_base, out_keys, out_dist, out_rows, st, deny);
        case SearchPlan::EMPTY: {
            // nothing stored: all-empty result (chromadb returns {"ids": [[]], ...})
            if ((rc = prep_exact_queries(ix, dev_queries, B, st)) != 0) return rc;
            u64* keys_dst = out_keys ? out_keys : ix->keys_tmp;
            HIP_TRY(hipMemsetAsync(keys_dst, 0, (size_t)B * k * sizeof(u64), st));
            if (!out_dist && !out_rows) return CODD_KNN_OK;
            return launch_merge(keys_dst, B, k, k, k, nullptr, out_dist, out_rows, st);
        }
        case SearchPlan::EXACT_SCAN:  // small batches: the per-block partials merge straight into the caller's buffers
            if ((rc = prep_exact_queries(ix, dev_queries, B, st)) != 0) return rc;
            return exact_scan(ix, ix->qn, B, k, row_base, out_keys, out_dist, out_rows, st, deny);
        case SearchPlan::SMALL_BATCH:
            // a handful of queries: ONE launch streams the int8 shadow, keeps the best approximate scores per wave and re-scores the
            // survivors exactly in its last workgroup (small_batch_kernel) instead of the six-launch filter chain
            HIP_TRY(ix->qn.ensure((int64_t)B * ix->dpad));
            if ((rc = small_batch_search(ix, dev_queries, B, k, row_base, out_keys, out_dist, out_rows, st, deny)) != 0) return rc;
            return masked ? CODD_KNN_OK : after_filter_search(ix, B, true, st);
        case SearchPlan::FILTER:
            break;
    }
    if (plan.use8) {
        HIP_TRY(ix->qfrag8.ensure((int64_t)kTileQ * (dpad8 / 16)));
        if (!ix->qmeta) HIP_TRY(ix->qmeta.reset(1024));
    } else if (plan.fused_prep) {
        hipLaunchKernelGGL(prep_queries_kernel, dim3(kTileQ / 4), dim3(256), 0, st, dev_queries, B, ix->dim, ix->dpad, ix->qn,
                           reinterpret_cast<uint2*>(ix->qfrag.get()), reinterpret_cast<unsigned*>(ix->ctl.get()), (int)(sizeof(FilterCtl) / 4));
        HIP_TRY(hipGetLastError());
    } else if ((rc = prep_exact_queries(ix, dev_queries, B, st)) != 0) {
        return rc;
    }
    if ((rc = ensure_filter_workspace(ix)) != 0) return rc;
    for (int q0 = 0; q0 < B; q0 += kTileQ) {
        const int nq = B - q0 < kTileQ ? B - q0 : kTileQ;
        if (plan.use8) {  // the int8 filter: every pass of <= 256 queries prepares its own block
            hipLaunchKernelGGL(prep_queries8_kernel, dim3(kTileQ / 4), dim3(256), 0, st, dev_queries + (int64_t)q0 * ix->dim, nq, ix->dim, ix->dpad, dpad8,
                               ix->qn + (int64_t)q0 * ix->dpad, reinterpret_cast<uint32_t*>(ix->qfrag8.get()), ix->qmeta, ix->eps_r_bits,
                               reinterpret_cast<unsigned*>(ix->ctl.get()), (int)(sizeof(FilterCtl) / 4), ix->exp_slack_scale);
            HIP_TRY(hipGetLastError());
        }
        if ((rc = filter_pass(ix, ix->qn + (int64_t)q0 * ix->dpad, nq, k, row_base, out_keys ? out_keys + (int64_t)q0 * k : nullptr,
                              out_dist ? out_dist + (int64_t)q0 * k : nullptr, out_rows ? out_rows + (int64_t)q0 * k : nullptr, st, deny,
                              plan.fused_prep || plan.use8, plan.use8)) != 0)
            return rc;
    }
    return masked ? CODD_KNN_OK : after_filter_search(ix, B, plan.use8, st);
}

// ---- scopes ----------------------------------------------------------------------------------

// the label array, as long as the row store, zero (= no label) until codd_knn_set_scopes_host writes it.  Only ever called with
// scope_of == nullptr or from an exclusive call: a live array is regrown by grow_rows alone.
int ensure_scope_labels(codd_knn_index* ix, hipStream_t st) {
    if (ix->scope_of && ix->scope_of.cap() >= ix->count) return CODD_KNN_OK;
    if (ix->scope_of) return fail(CODD_KNN_EDEVICE, "scope labels shorter than the row store%s");
    const int64_t cap = ix->capacity > ix->count ? ix->capacity : ix->count;
    if (cap < 1) return CODD_KNN_OK;
    HIP_TRY(ix->scope_of.reset(cap));
    HIP_TRY(hipMemsetAsync(ix->scope_of, 0, (size_t)cap * sizeof(uint32_t), st));
    return CODD_KNN_OK;
}

// The scope lists are derived data like the shadows: (re)built from the labels on the searching stream by the first scoped search
// after the labels or the row count changed.  Searches on other streams wait for the build on the device; the build waits for
// what they have already enqueued (their scans may still read the lists it overwrites).
int ensure_scope_lists(codd_knn_index* ix, hipStream_t st) {
    const int64_t n = ix->count;
    if (ix->scope_perm && ix->scope_built_gen == ix->scope_gen && ix->scope_built_count == n) {
        if (ix->scope_stream != st) HIP_TRY(hipStreamWaitEvent(st, ix->scope_ready, 0));
        return CODD_KNN_OK;
    }
    int rc;
    if ((rc = ensure_scope_labels(ix, st)) != 0) return rc;
    const int64_t nlist = (int64_t)ix->max_scope + 1;
    if (n > ix->scope_perm.cap() || 2 * nlist + 1 > ix->scope_offsets.cap()) {
        if ((rc = wait_searching_streams(ix)) != 0) return rc;   // (growth is the one place where a search call blocks)
        if (n > ix->scope_perm.cap()) HIP_TRY(ix->scope_perm.reset(ix->capacity > n ? ix->capacity : n));
        if (2 * nlist + 1 > ix->scope_offsets.cap()) {
            int64_t cap = 2049;
            while (cap < 2 * nlist + 1) cap = 2 * cap - 1;
            HIP_TRY(ix->scope_offsets.reset(cap));
        }
    }
    for (WorkSlot& w : ix->slots) {
        if (!w.used || w.stream == st) continue;
        HIP_TRY(w.handover.ensure());
        if (hipEventRecord(w.handover, w.stream) == hipSuccess) HIP_TRY(hipStreamWaitEvent(st, w.handover, 0));
        else (void)hipGetLastError();  // (a stream that no longer exists has nothing in flight)
    }
    if (ix->scope_ready && ix->scope_stream != st && ix->scope_built_gen >= 0) HIP_TRY(hipStreamWaitEvent(st, ix->scope_ready, 0));
    unsigned* start = ix->scope_offsets;
    unsigned* fill = start + nlist + 1;
    HIP_TRY(hipMemsetAsync(fill, 0, (size_t)nlist * sizeof(unsigned), st));
    const unsigned rb = (unsigned)((n + 255) / 256);
    hipLaunchKernelGGL(scope_count_kernel, dim3(rb), dim3(256), 0, st, ix->scope_of, n, (int)nlist, fill, ix->dead_bits);
    hipLaunchKernelGGL(scope_offsets_kernel, dim3(1), dim3(1024), 0, st, fill, (int)nlist, start);
    hipLaunchKernelGGL(scope_scatter_kernel, dim3(rb), dim3(256), 0, st, ix->scope_of, n, (int)nlist, start, fill, ix->scope_perm, ix->dead_bits);
    HIP_TRY(hipGetLastError());
    HIP_TRY(ix->scope_ready.ensure());
    HIP_TRY(hipEventRecord(ix->scope_ready, st));
    ix->scope_stream = st;
    ix->scope_built_gen = ix->scope_gen;
    ix->scope_built_count = n;
    ix->stat_scope_builds++;
    return CODD_KNN_OK;
}

// the IVF layout and its coarse index go (a new install, a failed one)
void drop_ivf(codd_knn_index* ix) {
    (void)ix->rows_ivf.reset();
    (void)ix->ivf_ids.reset();
    (void)ix->ivf_offsets.reset();
    (void)codd_knn_destroy(ix->coarse);
    ix->coarse = nullptr;
    ix->ivf_epoch = -1;
    ix->pend.clear();   // (the device bits are cleared by the install that follows; no search reads them without a layout)
    ix->list_of_valid = false;
}

// ---- an IVF layout that follows writes ----------------------------------------

bool ivf_layout_fresh(const codd_knn_index* ix) { return ix->coarse && ix->ivf_epoch == ix->epoch; }

// The slots a write made newly pending (`fresh`, the tail of the host's view of the list: positions [at, at + fresh.size())) go to
// the device on `st`, the write's stream: appended to pend_list through the pinned staging buffer, their bits set in pend_bits.
// Exclusive callers (a write); the searching streams are ordered behind `st` by the write itself.
int pend_mark_device(codd_knn_index* ix, const std::vector<uint32_t>& fresh, int64_t at, hipStream_t st) {
    const int64_t n = (int64_t)fresh.size();
    if (n == 0) return CODD_KNN_OK;
    if (!ix->pend_bits) {
        const int64_t words = (ix->capacity + 31) / 32;
        HIP_TRY(ix->pend_bits.reset(words));
        HIP_TRY(hipMemsetAsync(ix->pend_bits, 0, (size_t)words * sizeof(uint32_t), st));
    }
    if (at + n > ix->pend_list.cap()) {  // (growth blocks, as every growth here does: searches in flight may read the old list)
        DevBuf<uint32_t> grown;
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(grown.reset(pending_list_capacity(ix->pend_list.cap(), at + n)));
        if (at > 0) HIP_TRY(hipMemcpy(grown, ix->pend_list, (size_t)at * sizeof(uint32_t), hipMemcpyDeviceToDevice));
        HIP_TRY(hipDeviceSynchronize());
        ix->pend_list = std::move(grown);
    }
    if (ix->pend_stage_pending) HIP_TRY(hipEventSynchronize(ix->pend_staged));   // the staging buffer's previous copy
    ix->pend_stage_pending = false;
    if (n > ix->pend_stage.cap()) HIP_TRY(ix->pend_stage.reset(n + n / 2 + 64));
    HIP_TRY(ix->pend_staged.ensure());
    memcpy(ix->pend_stage.get(), fresh.data(), (size_t)n * sizeof(uint32_t));
    HIP_TRY(hipMemcpyAsync(ix->pend_list + at, ix->pend_stage, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipEventRecord(ix->pend_staged, st));
    ix->pend_stage_pending = true;
    hipLaunchKernelGGL(pend_set_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, ix->pend_list + at, n, ix->pend_bits);
    HIP_TRY(hipGetLastError());
    return CODD_KNN_OK;
}

// The end of every write of row slots through the C ABI: slots_written, and for a layout that follows writes the pending marks —
// the slots the write names (`slots`, n of them; null: the range [lo, hi)) and the gap below it — on `st`, the stream the rows
// were written on.  A failure here leaves the rows written and the layout stale.
int finish_write(codd_knn_index* ix, const int64_t* slots, int64_t n, int64_t lo, int64_t hi, hipStream_t st) {
    const bool following = ix->ivf_follow && ivf_layout_fresh(ix);
    const int64_t count_before = ix->count;
    slots_written(ix, lo, hi);
    if (!following) return CODD_KNN_OK;
    const int64_t at = ix->pend.count;
    std::vector<uint32_t> fresh;
    int rc;
    try {
        mark_written(ix->pend, count_before, slots, n, lo, hi, fresh);
        rc = pend_mark_device(ix, fresh, at, st);
    } catch (const std::bad_alloc&) {
        rc = fail(CODD_KNN_ENOMEM, "host allocation failed%s");
    }
    if (rc != 0) return rc;   // (ivf_epoch stays behind: the layout is stale)
    ix->ivf_epoch = ix->epoch;
    return CODD_KNN_OK;
}

// The fold: every pending slot is assigned its list — the top-1 of the coarse index's exact scan with the STORED row, widened to
// fp32, as the query — and the layout is rebuilt on the device from list_of: count, 64-bit prefix sums, scatter, then
// gather_rows_kernel from the main row store.  All sizes are known on the host: nothing is read back.  Ordered like an upsert on
// `st`: behind what the searching streams have enqueued, and later searches on other streams wait for rows_ready.
int ivf_fold_body(codd_knn_index* ix, hipStream_t st) {
    const int64_t n = ix->count, m = ix->pend.count;
    const int nlist = ix->ivf_nlist;
    const size_t row_bytes = (size_t)ix->dpad * elem_size(ix->dtype);
    WorkScope work(ix, st), work_coarse(ix->coarse, st);
    int rc;
    for (WorkSlot& w : ix->slots) {
        if (!w.used || w.stream == st) continue;
        HIP_TRY(w.handover.ensure());
        if (hipEventRecord(w.handover, w.stream) == hipSuccess) HIP_TRY(hipStreamWaitEvent(st, w.handover, 0));
        else (void)hipGetLastError();  // (a stream that no longer exists has nothing in flight)
    }
    if (ix->rows_event_set && ix->rows_stream != st) HIP_TRY(hipStreamWaitEvent(st, ix->rows_ready, 0));
    if (ix->reader_event_set && ix->reader_stream != st) HIP_TRY(hipStreamWaitEvent(st, ix->reader_done, 0));
    // appended rows: the layout's buffers and list_of grow.  (Growth is the one place where the fold blocks: what the searching
    // streams have enqueued may still read the old allocations.)
    const bool grows = n * (int64_t)row_bytes > ix->rows_ivf.cap() || n > ix->ivf_ids.cap() || (ix->list_of_valid && n > ix->list_of.cap());
    if (grows) {
        if ((rc = wait_searching_streams(ix)) != 0) return rc;
        HIP_TRY(hipStreamSynchronize(st));
    }
    const int64_t labels = ix->capacity > n ? ix->capacity : n;
    if (!ix->list_of_valid) {
        if (ix->list_of.cap() < n) HIP_TRY(ix->list_of.ensure(labels));
        HIP_TRY(hipMemsetAsync(ix->list_of, 0, (size_t)ix->list_of.bytes(), st));
        hipLaunchKernelGGL(list_of_build_kernel, dim3((unsigned)((ix->ivf_count + 255) / 256)), dim3(256), 0, st, ix->ivf_ids, ix->ivf_offsets, nlist,
                           ix->ivf_count, ix->list_of);
        HIP_TRY(hipGetLastError());
        ix->list_of_valid = true;
    } else if (ix->list_of.cap() < n) {
        DevBuf<uint32_t> grown;
        HIP_TRY(grown.reset(labels));
        HIP_TRY(hipMemsetAsync(grown, 0, (size_t)grown.bytes(), st));
        HIP_TRY(hipMemcpyAsync(grown, ix->list_of, (size_t)ix->ivf_count * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
        HIP_TRY(hipStreamSynchronize(st));
        ix->list_of = std::move(grown);
    }
    // 1. the pending rows' lists, in chunks of at most CODD_KNN_MAX_BATCH queries
    const int64_t chunk = m < CODD_KNN_MAX_BATCH ? m : CODD_KNN_MAX_BATCH;
    HIP_TRY(ix->fold_q.ensure(chunk * ix->dim));
    HIP_TRY(ix->qn.ensure(chunk * ix->dpad));
    HIP_TRY(ix->keys_tmp.ensure(chunk));
    for (int64_t c0 = 0; c0 < m; c0 += chunk) {
        const int nb = (int)(m - c0 < chunk ? m - c0 : chunk);
        const uint32_t* slots = ix->pend_list + c0;
        rc = with_dtype(ix->dtype, [&](auto dt) {
            return launch_kernel<widen_listed_rows_kernel<dt>>(dim3((unsigned)((nb + 3) / 4)), dim3(256), 0, st, ix->rows, slots, (int64_t)nb, ix->dim, ix->dpad,
                                                               ix->fold_q);
        });
        if (rc != 0) return rc;
        HIP_TRY(hipGetLastError());
        if ((rc = prep_exact_queries(ix, ix->fold_q, nb, st)) != 0) return rc;
        if ((rc = exact_scan(ix->coarse, ix->qn, nb, 1, 0u, ix->keys_tmp, nullptr, nullptr, st, ix->coarse->dead_bits)) != 0) return rc;
        hipLaunchKernelGGL(list_assign_kernel, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, st, ix->keys_tmp, slots, (int64_t)nb, nlist, ix->list_of);
        HIP_TRY(hipGetLastError());
    }
    // 2. the layout from list_of
    HIP_TRY(ix->fold_cnt.ensure(nlist));
    HIP_TRY(ix->fold_perm.ensure(n));
    if (n * (int64_t)row_bytes > ix->rows_ivf.cap()) HIP_TRY(ix->rows_ivf.reset(n * (int64_t)row_bytes));
    if (n > ix->ivf_ids.cap()) HIP_TRY(ix->ivf_ids.reset(n));
    HIP_TRY(hipMemsetAsync(ix->fold_cnt, 0, (size_t)nlist * sizeof(unsigned), st));
    const unsigned rb = (unsigned)((n + 255) / 256);
    hipLaunchKernelGGL(ivf_list_count_kernel, dim3(rb), dim3(256), 0, st, ix->list_of, n, nlist, ix->fold_cnt);
    hipLaunchKernelGGL(ivf_list_offsets_kernel, dim3(1), dim3(1024), 0, st, ix->fold_cnt, nlist, ix->ivf_offsets);
    hipLaunchKernelGGL(ivf_list_scatter_kernel, dim3(rb), dim3(256), 0, st, ix->list_of, n, nlist, ix->ivf_offsets, ix->fold_cnt, ix->fold_perm);
    hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, reinterpret_cast<const uint4*>(ix->rows.get()), ix->fold_perm, n,
                       (int)(row_bytes / 16), reinterpret_cast<uint4*>(ix->rows_ivf.get()), ix->ivf_ids);
    HIP_TRY(hipGetLastError());
    // 3. nothing is pending
    HIP_TRY(hipMemsetAsync(ix->pend_bits, 0, (size_t)ix->pend_bits.bytes(), st));
    ix->pend.clear();
    ix->ivf_count = n;
    ix->stat_ivf_refreshes++;
    HIP_TRY(ix->rows_ready.ensure());
    HIP_TRY(hipEventRecord(ix->rows_ready, st));
    ix->rows_stream = st;
    ix->rows_event_set = true;
    return CODD_KNN_OK;
}
// (a fold that fails half way leaves no layout to search: it is stale, and codd_knn_ivf_install is the remedy)
int ivf_fold(codd_knn_index* ix, hipStream_t st) {
    const int rc = ivf_fold_body(ix, st);
    if (rc != 0) ix->ivf_epoch = -1;
    return rc;
}

// what a write does last: fold when more rows are pending than "ivf_fold_rows" allows
int fold_if_due(codd_knn_index* ix, hipStream_t st) {
    if (!ix->ivf_follow || !ivf_layout_fresh(ix)) return CODD_KNN_OK;
    if (!fold_due(ix->pend.count, fold_threshold(ix->ivf_fold_rows, ix->ivf_count, ix->ivf_nlist))) return CODD_KNN_OK;
    return ivf_fold(ix, st);
}

// the end of a synchronous write (upsert_host, load_rows: the rows are on the device): finish_write and the fold when it is due on
// the null stream, complete on return like the rows themselves
int finish_sync_write(codd_knn_index* ix, const int64_t* slots, int64_t n, int64_t lo, int64_t hi) {
    const bool following = ix->ivf_follow && ivf_layout_fresh(ix);
    int rc = finish_write(ix, slots, n, lo, hi, nullptr);
    if (rc == 0) rc = fold_if_due(ix, nullptr);
    if (following && hipDeviceSynchronize() != hipSuccess && rc == 0) rc = fail(CODD_KNN_EDEVICE, "marking the written rows pending failed%s");
    ix->rows_event_set = false;  // (everything is complete on the device)
    return rc;
}

}  // namespace

extern "C" {

const char* codd_knn_version(void) {
    return "codd_knn 0.7.0 gfx950"
#if CODD_SHADOW_F16
           " shadow=f16"
#else
           " shadow=bf16"
#endif
#if CODD_MFMA16
           " mfma=16x16x32 int8=16x16x64";
#else
           " mfma=32x32x16";
#endif
}
const char* codd_knn_last_error(void) { return g_err; }

int codd_knn_create(codd_knn_index** out, int device, int dim, int dtype, int metric) {
    if (!out) return fail(CODD_KNN_EINVAL, "null out pointer%s");
    *out = nullptr;
    if (dim < 1 || dim > 4096) return fail(CODD_KNN_EINVAL, "dim out of range [1,4096]%s");
    if (dtype != DT_F32 && dtype != DT_BF16 && dtype != DT_F16) return fail(CODD_KNN_EINVAL, "unknown dtype%s");
    if (metric != CODD_KNN_METRIC_COSINE && metric != CODD_KNN_METRIC_IP && metric != CODD_KNN_METRIC_L2)
        return fail(CODD_KNN_ENOTSUP, "unknown metric (cosine 0, ip 1, l2 2)%s");
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail(CODD_KNN_EINVAL, "no such device%s");
    const int dpad = (dim + 63) / 64 * 64;
    codd_knn_index* ix = new (std::nothrow) codd_knn_index();
    if (!ix) return fail(CODD_KNN_ENOMEM, "host allocation failed%s");
    ix->device = device;
    ix->dim = dim;
    ix->dpad = dpad;
    ix->dtype = dtype;
    ix->metric = metric;
    // ip and l2 rows are no unit vectors, which both MFMA filters assume: such an index takes no filter leg, every batch the exact scan
    if (metric != CODD_KNN_METRIC_COSINE) ix->all_normalized = false;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) ix->num_cus = prop.multiProcessorCount;
    *out = ix;
    return CODD_KNN_OK;
}

int codd_knn_destroy(codd_knn_index* ix) {
    if (!ix) return CODD_KNN_OK;
    DeviceGuard guard(ix->device);
    (void)hipDeviceSynchronize();
    // (every buffer and event is a member that frees itself; the device is current and idle, as their destructors need)
    delete ix;
    return CODD_KNN_OK;
}

int codd_knn_reserve(codd_knn_index* ix, int64_t rows) {
    if (!ix || rows < 0) return fail(CODD_KNN_EINVAL, "bad reserve arguments%s");
    if (rows >= 0xffffffffll) return fail(CODD_KNN_EINVAL, "row slots must fit 32 bits%s");
    DeviceGuard guard(ix->device);
    if (rows <= ix->capacity) return CODD_KNN_OK;
    HIP_TRY(hipDeviceSynchronize());
    return grow_rows(ix, rows, /*exact=*/true);  // the caller states the final size (288 GB of HBM is the only limit)
}

int codd_knn_upsert_host(codd_knn_index* ix, const int64_t* host_slots, const float* host_vecs, int64_t n, int normalize) {
    if (!ix || (n > 0 && (!host_slots || !host_vecs)) || n < 0) return fail(CODD_KNN_EINVAL, "bad upsert arguments%s");
    if (n == 0) return CODD_KNN_OK;
    int64_t max_slot = -1, min_slot = INT64_MAX;
    for (int64_t i = 0; i < n; ++i) {
        if (host_slots[i] < 0 || host_slots[i] >= 0xfffffffell) return fail(CODD_KNN_EINVAL, "row slot out of range%s");
        if (slot_dead(ix, host_slots[i])) return fail(CODD_KNN_EINVAL, "upsert into a deleted row slot (it stays dead until codd_knn_compact)%s");
        if (host_slots[i] > max_slot) max_slot = host_slots[i];
        if (host_slots[i] < min_slot) min_slot = host_slots[i];
    }
    DeviceGuard guard(ix->device);
    HIP_TRY(hipDeviceSynchronize());
    int rc = grow_rows(ix, max_slot + 1, /*exact=*/false);
    if (rc != 0) return rc;
    // stage in bounded pieces (<= 64 MiB of vectors per piece) through buffers the index keeps between calls (the indexer job
    // upserts one small batch at a time: an allocation and a release per call used to dominate them)
    const int64_t piece = (int64_t)(64ll << 20) / ((int64_t)ix->dim * 4) + 1;
    const int64_t pn = n < piece ? n : piece;
    if (pn * ix->dim > ix->stage_vec.cap()) HIP_TRY(ix->stage_vec.reset(pn * ix->dim < 65536 ? 65536 : pn * ix->dim));
    if (pn > ix->stage_slot.cap()) HIP_TRY(ix->stage_slot.reset(pn < 4096 ? 4096 : pn));
    float* dvec = ix->stage_vec;
    int64_t* dslot = ix->stage_slot;
    rc = CODD_KNN_OK;
    for (int64_t i0 = 0; i0 < n && rc == 0; i0 += pn) {
        const int64_t m = n - i0 < pn ? n - i0 : pn;
        hipError_t e = hipMemcpy(dvec, host_vecs + i0 * ix->dim, (size_t)m * ix->dim * sizeof(float), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(dslot, host_slots + i0, (size_t)m * sizeof(int64_t), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            rc = fail(CODD_KNN_EDEVICE, "staging copy failed: %s", hipGetErrorString(e));
            break;
        }
        rc = launch_ingest(ix, dvec, m, normalize, dslot, 0, nullptr);
        // (one synchronisation per piece: the staging buffers are reused by the next piece, and the call is synchronous by contract)
        if (rc == 0 && hipDeviceSynchronize() != hipSuccess) rc = fail(CODD_KNN_EDEVICE, "ingest kernel failed%s");
    }
    ix->rows_event_set = false;  // (everything is complete on the device)
    ix->reader_event_set = false;
    if (rc == 0) {
        if (!normalize) ix->all_normalized = false;
        rc = finish_sync_write(ix, host_slots, n, min_slot, max_slot + 1);
    }
    return rc;
}

int codd_knn_upsert_device(codd_knn_index* ix, int64_t first_slot, const float* dev_vecs, int64_t n, int normalize, void* stream) {
    if (!ix || n < 0 || first_slot < 0 || (n > 0 && !dev_vecs)) return fail(CODD_KNN_EINVAL, "bad upsert arguments%s");
    if (n == 0) return CODD_KNN_OK;
    if (first_slot + n >= 0xffffffffll) return fail(CODD_KNN_EINVAL, "row slots must fit 32 bits%s");
    if (range_has_dead(ix, first_slot, first_slot + n)) return fail(CODD_KNN_EINVAL, "upsert into a deleted row slot (it stays dead until codd_knn_compact)%s");
    DeviceGuard guard(ix->device);
    if (first_slot + n > ix->capacity) {
        HIP_TRY(hipDeviceSynchronize());
        int rc = grow_rows(ix, first_slot + n, /*exact=*/false);
        if (rc != 0) return rc;
    }
    hipStream_t wst = (hipStream_t)stream;
    // device-side ordering against searches still in flight on OTHER streams (the call is exclusive on the host, but their
    // kernels may still be reading the rows this launch overwrites): the writing stream waits for every searching stream
    for (WorkSlot& w : ix->slots) {
        if (!w.used || w.stream == wst) continue;
        HIP_TRY(w.handover.ensure());
        if (hipEventRecord(w.handover, w.stream) == hipSuccess) HIP_TRY(hipStreamWaitEvent(wst, w.handover, 0));
        else (void)hipGetLastError();  // (a stream that no longer exists has nothing in flight)
    }
    // ... and for the previous writer, when that was another stream: rows_ready is ONE event, re-recorded by every write, so
    // chaining the writers makes the last record cover every earlier write (a reader only ever waits for the last one)
    if (ix->rows_event_set && ix->rows_stream != wst) HIP_TRY(hipStreamWaitEvent(wst, ix->rows_ready, 0));
    // ... and for streams that only READ rows outside a search (codd_knn_copy_rows_f32)
    if (ix->reader_event_set && ix->reader_stream != wst) HIP_TRY(hipStreamWaitEvent(wst, ix->reader_done, 0));
    int rc = launch_ingest(ix, dev_vecs, n, normalize, nullptr, first_slot, wst);
    if (rc != 0) return rc;
    if (!normalize) ix->all_normalized = false;
    // (a layout that follows writes: the pending marks go onto the writing stream behind the rows, in front of rows_ready)
    const int mark_rc = finish_write(ix, nullptr, n, first_slot, first_slot + n, wst);
    // ... and searches on other streams wait for this write (wait_rows)
    HIP_TRY(ix->rows_ready.ensure());
    HIP_TRY(hipEventRecord(ix->rows_ready, wst));
    ix->rows_stream = wst;
    ix->rows_event_set = true;
    if (mark_rc != 0) return mark_rc;
    return fold_if_due(ix, wst);
}

int codd_knn_load_rows(codd_knn_index* ix, int64_t first_slot, const void* host_rows, int64_t n) {
    if (!ix || first_slot < 0 || n < 0 || (n > 0 && !host_rows)) return fail(CODD_KNN_EINVAL, "bad load_rows arguments%s");
    if (n == 0) return CODD_KNN_OK;
    if (first_slot + n >= 0xffffffffll) return fail(CODD_KNN_EINVAL, "row slots must fit 32 bits%s");
    if (range_has_dead(ix, first_slot, first_slot + n)) return fail(CODD_KNN_EINVAL, "load_rows into a deleted row slot (it stays dead until codd_knn_compact)%s");
    DeviceGuard guard(ix->device);
    HIP_TRY(hipDeviceSynchronize());
    for (auto& col : ix->columns) {  // the metadata columns described other rows: the caller builds them again (derived data)
        (void)col.tags.reset();
        (void)col.cells.reset();
    }
    int rc = grow_rows(ix, first_slot + n, /*exact=*/false);
    if (rc != 0) return rc;
    const size_t row_bytes = (size_t)ix->dpad * elem_size(ix->dtype);
    HIP_TRY(hipMemcpy(ix->rows + (size_t)first_slot * row_bytes, host_rows, (size_t)n * row_bytes, hipMemcpyHostToDevice));
    if (!metric_is_cosine(ix)) {   // (ip, l2: rows of any norm, and no filter to keep on)
        return finish_sync_write(ix, nullptr, n, first_slot, first_slot + n);
    }
    // the loaded rows are taken as they are, so their norms are checked: the filters stay on only for unit rows
    // (tolerance = the storage type's rounding of a unit vector)
    DevBuf<unsigned> dev_bits;
    HIP_TRY(dev_bits.reset(1));
    hipError_t e = hipMemset(dev_bits, 0, sizeof(unsigned));
    const dim3 grid((unsigned)((n + 3) / 4)), block(256);
    if (e == hipSuccess) {
        (void)with_dtype(ix->dtype, [&](auto dt) {
            return launch_kernel<row_norm_check_kernel<dt>>(grid, block, 0, nullptr, ix->rows, first_slot, n, ix->dpad, dev_bits);
        });
        e = hipGetLastError();
    }
    float worst = 0.0f;
    if (e == hipSuccess) e = hipMemcpy(&worst, dev_bits, sizeof(float), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(CODD_KNN_EDEVICE, "norm check of the loaded rows failed: %s", hipGetErrorString(e));
    const float tol = ix->dtype == DT_F32 ? 1e-4f : (ix->dtype == DT_BF16 ? 4e-3f : 6e-4f);
    if (!(worst <= tol)) ix->all_normalized = false;
    return finish_sync_write(ix, nullptr, n, first_slot, first_slot + n);
}

int codd_knn_count(const codd_knn_index* ix, int64_t* out) {
    if (!ix || !out) return fail(CODD_KNN_EINVAL, "bad count arguments%s");
    *out = ix->count;
    return CODD_KNN_OK;
}

int codd_knn_dim(const codd_knn_index* ix, int* dim, int* padded_dim, int* dtype) {
    if (!ix) return fail(CODD_KNN_EINVAL, "null index%s");
    if (dim) *dim = ix->dim;
    if (padded_dim) *padded_dim = ix->dpad;
    if (dtype) *dtype = ix->dtype;
    return CODD_KNN_OK;
}

int codd_knn_read_rows(const codd_knn_index* ix, int64_t first, int64_t n, void* host_out) {
    if (!ix || first < 0 || n < 0 || first + n > ix->count || (n > 0 && !host_out)) return fail(CODD_KNN_EINVAL, "bad read_rows range%s");
    if (n == 0) return CODD_KNN_OK;
    DeviceGuard guard(ix->device);
    const size_t row_bytes = (size_t)ix->dpad * elem_size(ix->dtype);
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(host_out, ix->rows + (size_t)first * row_bytes, (size_t)n * row_bytes, hipMemcpyDeviceToHost));
    return CODD_KNN_OK;
}

int codd_knn_search(codd_knn_index* ix, const float* dev_queries, int B, int k, float* dev_dist, int64_t* dev_rows, void* stream) {
    if (!dev_dist || !dev_rows) return fail(CODD_KNN_EINVAL, "null output%s");
    if (!ix) return fail(CODD_KNN_EINVAL, "null index%s");
    WorkScope work(ix, (hipStream_t)stream);
    return search_impl(ix, dev_queries, B, k, 0u, nullptr, dev_dist, dev_rows, (hipStream_t)stream, ix->dead_bits);
}

int codd_knn_search_keys(codd_knn_index* ix, const float* dev_queries, int B, int k, uint32_t row_base, uint64_t* dev_keys, void* stream) {
    if (!dev_keys) return fail(CODD_KNN_EINVAL, "null output%s");
    if (!ix) return fail(CODD_KNN_EINVAL, "null index%s");
    if ((int64_t)row_base + ix->count >= 0xffffffffll) return fail(CODD_KNN_EINVAL, "global row ids must fit 32 bits%s");
    WorkScope work(ix, (hipStream_t)stream);
    return search_impl(ix, dev_queries, B, k, row_base, (u64*)dev_keys, nullptr, nullptr, (hipStream_t)stream, ix->dead_bits);
}

int codd_knn_merge_keys(int device, const uint64_t* dev_keys_in, int B, int m, int k, uint64_t* dev_keys_out, float* dev_dist,
                        int64_t* dev_rows, void* stream) {
    if (!dev_keys_in || B < 1 || m < 1 || k < 1 || k > CODD_KNN_MAX_K) return fail(CODD_KNN_EINVAL, "bad merge arguments%s");
    DeviceGuard guard(device);
    return launch_merge((const u64*)dev_keys_in, B, m, m, k, (u64*)dev_keys_out, dev_dist, dev_rows, (hipStream_t)stream);
}

int codd_knn_merge_shards(int device, const uint64_t* dev_keys_in, int G, int B, int k_in, int k, uint64_t* dev_keys_out, float* dev_dist,
                          int64_t* dev_rows, void* stream) {
    if (!dev_keys_in || G < 1 || B < 1 || k_in < 1 || k < 1 || k > CODD_KNN_MAX_K) return fail(CODD_KNN_EINVAL, "bad merge arguments%s");
    DeviceGuard guard(device);
    return launch_merge((const u64*)dev_keys_in, B, (int64_t)G * k_in, k_in, k, (u64*)dev_keys_out, dev_dist, dev_rows, (hipStream_t)stream, nullptr,
                        nullptr, nullptr, k_in, (int64_t)B * k_in);
}

int codd_knn_merge_keys_metric(int device, const uint64_t* dev_keys_in, int B, int m, int k, int metric, uint64_t* dev_keys_out, float* dev_dist,
                               int64_t* dev_rows, void* stream) {
    if (!dev_keys_in || B < 1 || m < 1 || k < 1 || k > CODD_KNN_MAX_K) return fail(CODD_KNN_EINVAL, "bad merge arguments%s");
    if (metric != CODD_KNN_METRIC_COSINE && metric != CODD_KNN_METRIC_IP && metric != CODD_KNN_METRIC_L2) return fail(CODD_KNN_ENOTSUP, "unknown metric (cosine 0, ip 1, l2 2)%s");
    DeviceGuard guard(device);
    return launch_merge((const u64*)dev_keys_in, B, m, m, k, (u64*)dev_keys_out, dev_dist, dev_rows, (hipStream_t)stream, nullptr, nullptr, nullptr, 0, 0,
                        kernel_metric(metric));
}

int codd_knn_merge_shards_metric(int device, const uint64_t* dev_keys_in, int G, int B, int k_in, int k, int metric, uint64_t* dev_keys_out,
                                 float* dev_dist, int64_t* dev_rows, void* stream) {
    if (!dev_keys_in || G < 1 || B < 1 || k_in < 1 || k < 1 || k > CODD_KNN_MAX_K) return fail(CODD_KNN_EINVAL, "bad merge arguments%s");
    if (metric != CODD_KNN_METRIC_COSINE && metric != CODD_KNN_METRIC_IP && metric != CODD_KNN_METRIC_L2) return fail(CODD_KNN_ENOTSUP, "unknown metric (cosine 0, ip 1, l2 2)%s");
    DeviceGuard guard(device);
    return launch_merge((const u64*)dev_keys_in, B, (int64_t)G * k_in, k_in, k, (u64*)dev_keys_out, dev_dist, dev_rows, (hipStream_t)stream, nullptr,
                        nullptr, nullptr, k_in, (int64_t)B * k_in, kernel_metric(metric));
}

int codd_knn_approx_scores(codd_knn_index* ix, const float* dev_queries, int B, float* dev_scores, void* stream) {
    if (!ix || !dev_queries || !dev_scores || B < 1 || B > kTileQ) return fail(CODD_KNN_EINVAL, "bad debug arguments%s");
    // an ip or l2 index: the values of its int8 filter leg, where that leg exists
    const bool space = !metric_is_cosine(ix);
    const bool space_ok = space && ix->knobs.space_filter && ix->knobs.shadow8_enabled && CODD_MFMA16 && B <= 32 && !(ix->metric == CODD_KNN_METRIC_L2 && niter_of(shape_of(ix)) > 4);
    if (space && !space_ok)
        return fail(CODD_KNN_ENOTSUP, "approx_scores: the MFMA filters' scores exist for the cosine metric only (ip, l2: with \"space_filter\" on, B <= 32)%s");
    if (ix->count < 1) return fail(CODD_KNN_EINVAL, "empty index%s");
    DeviceGuard guard(ix->device);
    hipStream_t st = (hipStream_t)stream;
    WorkScope work(ix, st);
    int rc;
    if ((rc = wait_rows(ix, st)) != 0) return rc;
    HIP_TRY(ix->qn.ensure((int64_t)B * ix->dpad));
    if (space) {
        if ((rc = ensure_space_filter(ix, st)) != 0) return rc;
        if ((rc = launch_prep_raw(ix, dev_queries, B, ix->qn, st)) != 0) return rc;
        const int dpad8 = dpad8_of(shape_of(ix));
        const int64_t ntiles8 = tiles_of(ix->count);
        const dim3 g8((unsigned)(ntiles8 < ix->num_cus ? ntiles8 : ix->num_cus));
        if (ix->metric == CODD_KNN_METRIC_L2)
            rc = launch_kernel<sqd_filter_kernel<MODE_DUMP, 1>>(g8, dim3(kFilterThreads), filter_lds_bytes(MODE_DUMP), st, ix->shadow8, ix->qfrag8, ix->count, dpad8 / 128,
                                                                ntiles8, (int64_t)1, nullptr, nullptr, nullptr, nullptr, 0, nullptr, dev_scores, ix->rscale, ix->qmeta,
                                                                ix->rnorm2, ix->qmeta + 512);
        else
            rc = launch_kernel<gemm_filter_kernel<MODE_DUMP, 1, 1>>(g8, dim3(kFilterThreads), filter_lds_bytes(MODE_DUMP), st, ix->shadow8, ix->qfrag8, ix->count,
                                                                    dpad8 / 128, ntiles8, (int64_t)1, nullptr, nullptr, nullptr, nullptr, 0, nullptr, dev_scores, ix->rscale,
                                                                    ix->qmeta);
        if (rc != 0) return rc;
        HIP_TRY(hipGetLastError());
        return CODD_KNN_OK;
    }
    if ((rc = ensure_filter_workspace(ix)) != 0) return rc;
    if (ix->knobs.shadow8_enabled && B <= 32 && CODD_MFMA16) {
        // the int8 filter's scores (what a batch of <= 32 queries is filtered with when "shadow8" is on)
        if ((rc = ensure_shadow8(ix, st)) != 0) return rc;
        const int dpad8 = dpad8_of(shape_of(ix));
        HIP_TRY(ix->qfrag8.ensure((int64_t)kTileQ * (dpad8 / 16)));
        if (!ix->qmeta) HIP_TRY(ix->qmeta.reset(1024));
        hipLaunchKernelGGL(prep_queries8_kernel, dim3(kTileQ / 4), dim3(256), 0, st, dev_queries, B, ix->dim, ix->dpad, dpad8, ix->qn,
                           reinterpret_cast<uint32_t*>(ix->qfrag8.get()), ix->qmeta, ix->eps_r_bits, reinterpret_cast<unsigned*>(ix->ctl.get()),
                           (int)(sizeof(FilterCtl) / 4), 1.0f);
        const int64_t ntiles8 = tiles_of(ix->count);
        const int64_t g8 = ntiles8 < ix->num_cus ? ntiles8 : ix->num_cus;
        if ((rc = launch_kernel<gemm_filter_kernel<MODE_DUMP, 1, 1>>(dim3((unsigned)g8), dim3(kFilterThreads), filter_lds_bytes(MODE_DUMP), st,
                                                                     ix->shadow8, ix->qfrag8, ix->count, dpad8 / 128, ntiles8, (int64_t)1, nullptr, nullptr,
                                                                     nullptr, nullptr, 0, nullptr, dev_scores, ix->rscale, ix->qmeta)) != 0)
            return rc;
        HIP_TRY(hipGetLastError());
        return CODD_KNN_OK;
    }
    if ((rc = ensure_shadow(ix, st)) != 0) return rc;
    if ((rc = launch_normalize(DT_F32, dev_queries, B, ix->dim, ix->dpad, 1, nullptr, 0, ix->qn, nullptr, st)) != 0) return rc;
    hipLaunchKernelGGL(qfrag_kernel, dim3((kTileQ * (ix->dpad / 8) + 255) / 256), dim3(256), 0, st, ix->qn, B, ix->dpad, ix->qfrag,
                       (unsigned*)nullptr, 0);
    const int64_t ntiles = tiles_of(ix->count);
    const int64_t g = ntiles < ix->num_cus ? ntiles : ix->num_cus;
    if ((rc = launch_kernel<gemm_filter_kernel<MODE_DUMP, 8>>(dim3((unsigned)g), dim3(kFilterThreads), filter_lds_bytes(MODE_DUMP), st, ix->shadow,
                                                              ix->qfrag, ix->count, ix->dpad / 64, ntiles, (int64_t)1, nullptr, nullptr, nullptr, nullptr, 0,
                                                              nullptr, dev_scores, nullptr, nullptr)) != 0)
        return rc;
    HIP_TRY(hipGetLastError());
    return CODD_KNN_OK;
}

int codd_knn_filter_slack(codd_knn_index* ix, const float* dev_queries, int B, float* dev_slack, void* stream) {
    if (!ix || !dev_queries || !dev_slack || B < 1 || B > kTileQ) return fail(CODD_KNN_EINVAL, "bad debug arguments%s");
    const bool space = !metric_is_cosine(ix);
    if (!ix->knobs.shadow8_enabled || !CODD_MFMA16 || (space && !ix->knobs.space_filter) || (space && ix->metric == CODD_KNN_METRIC_L2 && niter_of(shape_of(ix)) > 4))
        return fail(CODD_KNN_ENOTSUP, "filter_slack: this index has no int8 filter leg (\"shadow8\"; ip, l2: \"space_filter\")%s");
    if (ix->count < 1) return fail(CODD_KNN_EINVAL, "empty index%s");
    DeviceGuard guard(ix->device);
    hipStream_t st = (hipStream_t)stream;
    WorkScope work(ix, st);
    int rc;
    if ((rc = wait_rows(ix, st)) != 0) return rc;
    HIP_TRY(ix->qn.ensure((int64_t)B * ix->dpad));
    if ((rc = ensure_space_filter(ix, st)) != 0) return rc;
    if (space) {
        if ((rc = launch_prep_raw(ix, dev_queries, B, ix->qn, st)) != 0) return rc;
    } else {
        hipLaunchKernelGGL(prep_queries8_kernel, dim3(kTileQ / 4), dim3(256), 0, st, dev_queries, B, ix->dim, ix->dpad, dpad8_of(shape_of(ix)), ix->qn,
                           reinterpret_cast<uint32_t*>(ix->qfrag8.get()), ix->qmeta, ix->eps_r_bits, reinterpret_cast<unsigned*>(ix->ctl.get()),
                           (int)(sizeof(FilterCtl) / 4), ix->exp_slack_scale);
    }
    hipLaunchKernelGGL(filter_slack_kernel, dim3(1), dim3(kTileQ), 0, st, ix->qmeta + 256, B, dev_slack);
    HIP_TRY(hipGetLastError());
    return CODD_KNN_OK;
}

int codd_knn_copy_rows_f32(codd_knn_index* ix, int64_t first, int64_t n, float* dev_out, void* stream) {
    if (!ix || first < 0 || n < 0 || first + n > ix->count || (n > 0 && !dev_out)) return fail(CODD_KNN_EINVAL, "bad copy_rows range%s");
    if (n == 0) return CODD_KNN_OK;
    DeviceGuard guard(ix->device);
    const dim3 grid((unsigned)((n + 3) / 4)), block(256);
    hipStream_t st = (hipStream_t)stream;
    std::lock_guard<std::mutex> lock(ix->mu);
    // a read of the stored rows on the caller's stream: behind the last asynchronous write (as a search is), and the next
    // writer on another stream is ordered behind it (reader_done)
    int rc;
    if ((rc = wait_rows(ix, st)) != 0) return rc;
    rc = with_dtype(ix->dtype, [&](auto dt) {
        return launch_kernel<widen_rows_kernel<dt>>(grid, block, 0, st, ix->rows, first, n, ix->dim, ix->dpad, dev_out);
    });
    if (rc != 0) return rc;
    HIP_TRY(hipGetLastError());
    HIP_TRY(ix->reader_done.ensure());
    if (ix->reader_event_set && ix->reader_stream != st) HIP_TRY(hipStreamWaitEvent(st, ix->reader_done, 0));  // (one event: chain the readers too)
    HIP_TRY(hipEventRecord(ix->reader_done, st));
    ix->reader_stream = st;
    ix->reader_event_set = true;
    return CODD_KNN_OK;
}

int codd_knn_ivf_install(codd_knn_index* ix, const float* dev_centroids, int nlist, const int64_t* dev_perm,
                         const int64_t* dev_offsets, void* stream) {
    if (!ix || !dev_centroids || !dev_perm || !dev_offsets || nlist < 1 || nlist > (1 << 20)) return fail(CODD_KNN_EINVAL, "bad ivf_install arguments%s");
    if (!ivf_allowed(ix)) return fail(CODD_KNN_ENOTSUP, "ivf_install: IVF exists for the cosine metric only (spherical k-means, bf16 assignment)%s");
    if (ix->count < 1) return fail(CODD_KNN_EINVAL, "empty index%s");
    DeviceGuard guard(ix->device);
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipDeviceSynchronize());
    drop_ivf(ix);  // a previous layout
    if (ix->pend_bits) HIP_TRY(hipMemsetAsync(ix->pend_bits, 0, (size_t)ix->pend_bits.bytes(), st));  // ... and what was pending under it

    const size_t row_bytes = (size_t)ix->dpad * elem_size(ix->dtype);
    const int64_t n = ix->count;
    // validate the caller's tables before anything indexes memory with them: offsets on the host (nlist + 1 values),
    // the permutation on the device
    {
        std::vector<int64_t> off((size_t)nlist + 1);
        HIP_TRY(hipMemcpyAsync(off.data(), dev_offsets, off.size() * sizeof(int64_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        bool ok = off[0] == 0 && off[(size_t)nlist] == n;
        for (int l = 0; ok && l < nlist; ++l) ok = off[(size_t)l] <= off[(size_t)l + 1];
        if (!ok) return fail(CODD_KNN_EINVAL, "ivf_install: offsets must start at 0, never decrease and end at the row count%s");
        DevBuf<unsigned> bad;
        HIP_TRY(bad.reset(1));
        hipError_t e = hipMemsetAsync(bad, 0, sizeof(unsigned), st);
        unsigned host_bad = 1;
        if (e == hipSuccess) {
            hipLaunchKernelGGL(perm_check_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, dev_perm, n, bad);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipMemcpyAsync(&host_bad, bad, sizeof(unsigned), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) return fail(CODD_KNN_EDEVICE, "ivf_install: permutation check failed: %s", hipGetErrorString(e));
        if (host_bad) return fail(CODD_KNN_EINVAL, "ivf_install: permutation entries must lie in [0, count)%s");
    }
    // (a failed install leaves no half-built layout behind: drop_ivf)
    int rc = CODD_KNN_OK;
    hipError_t he = ix->rows_ivf.reset(n * (int64_t)row_bytes);
    if (he == hipSuccess) he = ix->ivf_ids.reset(n);
    if (he == hipSuccess) he = ix->ivf_offsets.reset((int64_t)nlist + 1);
    if (he == hipSuccess) he = hipMemcpyAsync(ix->ivf_offsets, dev_offsets, (size_t)(nlist + 1) * sizeof(int64_t), hipMemcpyDeviceToDevice, st);
    if (he == hipSuccess) {
        hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, reinterpret_cast<const uint4*>(ix->rows.get()), dev_perm, n,
                           (int)(row_bytes / 16), reinterpret_cast<uint4*>(ix->rows_ivf.get()), ix->ivf_ids);
        he = hipGetLastError();
    }
    if (he != hipSuccess) {
        drop_ivf(ix);
        return fail(he == hipErrorOutOfMemory ? CODD_KNN_ENOMEM : CODD_KNN_EDEVICE, "ivf_install: building the list layout failed: %s", hipGetErrorString(he));
    }
    // the coarse index lives in the index's own space: unit centroids for cosine, the centroids as given for ip and l2 (§22)
    rc = codd_knn_create(&ix->coarse, ix->device, ix->dim, DT_F32, ix->metric);
    if (rc == 0) rc = codd_knn_upsert_device(ix->coarse, 0, dev_centroids, nlist, metric_is_cosine(ix) ? 1 : 0, stream);
    if (rc == 0 && hipStreamSynchronize(st) != hipSuccess) rc = fail(CODD_KNN_EDEVICE, "ivf_install: device work failed%s");
    if (rc != 0) {
        drop_ivf(ix);
        return rc;
    }
    ix->ivf_nlist = nlist;
    ix->ivf_count = n;
    ix->ivf_epoch = ix->epoch;
    return CODD_KNN_OK;
}

}  // extern "C"

namespace {

// what the scoped, the masked and the IVF entry points check before they take a workspace
int search_check_args(const codd_knn_index* ix, const float* dev_queries, int B, int k, uint32_t row_base) {
    if (!ix || !dev_queries) return fail(CODD_KNN_EINVAL, "null index or queries%s");
    if (B < 1 || B > CODD_KNN_MAX_BATCH) return fail(CODD_KNN_EINVAL, "B out of range [1,1024]%s");
    if (k < 1 || k > CODD_KNN_MAX_K) return fail(CODD_KNN_EINVAL, "k out of range [1,128]%s");
    if ((int64_t)row_base + ix->count >= 0xffffffffll) return fail(CODD_KNN_EINVAL, "global row ids must fit 32 bits%s");
    return CODD_KNN_OK;
}

// nothing visible (or nothing stored): all-empty result, no scan
int empty_result(codd_knn_index* ix, int B, int k, uint64_t* dev_keys, float* dev_dist, int64_t* dev_rows, hipStream_t st) {
    HIP_TRY(ix->keys_tmp.ensure((int64_t)B * k));
    u64* keys_dst = dev_keys ? (u64*)dev_keys : ix->keys_tmp.get();
    HIP_TRY(hipMemsetAsync(keys_dst, 0, (size_t)B * k * sizeof(u64), st));
    if (!dev_dist && !dev_rows) return CODD_KNN_OK;
    return launch_merge(keys_dst, B, k, k, k, nullptr, dev_dist, dev_rows, st);
}

// what every IVF entry point checks before it takes a workspace; clamps nprobe to the number of lists
int ivf_check_args(const codd_knn_index* ix, const float* dev_queries, int B, int k, uint32_t row_base, int* nprobe) {
    int rc;
    if ((rc = search_check_args(ix, dev_queries, B, k, row_base)) != 0) return rc;
    if (!ivf_allowed(ix)) return fail(CODD_KNN_ENOTSUP, "IVF search exists for the cosine metric only%s");
    // (a layout that follows writes keeps ivf_epoch at the epoch; rows left pending when "ivf_follow" was switched off make it stale)
    if (!ivf_layout_fresh(ix) || (ix->pend.count > 0 && !ix->ivf_follow))
        return fail(CODD_KNN_EINVAL, "no IVF layout, or rows changed since codd_knn_ivf_install%s");
    if (*nprobe < 1) return fail(CODD_KNN_EINVAL, "nprobe must be >= 1%s");
    if (*nprobe > ix->ivf_nlist) *nprobe = ix->ivf_nlist;
    if (*nprobe > CODD_KNN_MAX_K) return fail(CODD_KNN_ENOTSUP, "nprobe above 128 is not supported (probe the whole index with codd_knn_search)%s");
    return CODD_KNN_OK;
}

// The body of every IVF search; the caller has checked the arguments, made the device current and holds the workspaces of the
// index and of its coarse index for `st`.  deny: the ORIGINAL row slots no answer may hold — ix->dead_bits, or the ~allow | dead
// of a masked search, which the list scans test where they test the tombstones.  Probe selection never sees it.
int ivf_search_body(codd_knn_index* ix, const float* dev_queries, int B, int k, int nprobe, uint32_t row_base, uint64_t* dev_keys, float* dev_dist,
                    int64_t* dev_rows, hipStream_t st, const uint32_t* deny) {
    int rc;
    if ((rc = wait_rows(ix, st)) != 0) return rc;
    HIP_TRY(ix->qn.ensure((int64_t)B * ix->dpad));
    HIP_TRY(ix->probe_keys.ensure((int64_t)B * nprobe));
    if ((rc = prep_exact_queries(ix, dev_queries, B, st)) != 0) return rc;
    const bool sq = ix->metric == CODD_KNN_METRIC_L2;  // the squared-distance list scans (§22); ip runs the dot-product ones on the raw query
    // 1. coarse: the nprobe best lists per query (exact scan of the centroids in the index's space, tiny)
    if ((rc = exact_scan(ix->coarse, ix->qn, B, nprobe, 0u, ix->probe_keys, nullptr, nullptr, st, ix->coarse->dead_bits)) != 0) return rc;
    // Rows pending (a layout that follows writes): the layout's copy of them is stale, so the list scans run under
    // deny | pending, and the delta scan scores every pending slot from the row store under the call's own deny.  Its partial keys go
    // behind the lists' — query b's at [B * m1 + b * m1, ...), m1 the lists' keys per query — and ONE merge reads both runs.
    // Nothing pending: a host branch, and the launches below are what they always were.
    const int64_t npend = ix->pend.count;
    const uint32_t* deny_lists = deny;
    if (npend > 0) {
        const int64_t nwords = (ix->count + 31) / 32;
        HIP_TRY(ix->ivf_deny.ensure(nwords));
        hipLaunchKernelGGL(pend_or_kernel, dim3((unsigned)((nwords + 255) / 256)), dim3(256), 0, st, deny, ix->pend_bits, nwords, ix->ivf_deny);
        HIP_TRY(hipGetLastError());
        deny_lists = ix->ivf_deny;
        ix->stat_ivf_delta++;
    }
    // m1: the lists' partial keys per query, list_parts = m1 / k of them; the caller has made room for 2 * B * m1 keys
    auto delta_then_merge = [&](int64_t m1, int64_t list_parts) -> int {
        if (npend == 0) return launch_merge_of(ix, ix->ivf_partial, B, m1, k, (u64*)dev_keys, dev_dist, dev_rows, st);
        const int dsplit = delta_split(ix->num_cus, B, npend, list_parts);
        u64* delta = ix->ivf_partial + (int64_t)B * m1;
        int drc;
        {
            EvScope ev(ix, EV_SCAN, st);
            drc = with_row_form(ix, k, "row too wide for the IVF scan%s", [&](auto dt, auto ni, auto sl) {
                constexpr int NB = scope_nb(decltype(dt)::value, decltype(ni)::value);
                return launch_by_metric<ivf_delta_sq<dt, ni, sl>, ivf_delta_kernel<dt, ni, sl>>(kernel_metric(ix->metric), dim3((unsigned)((B + NB - 1) / NB), (unsigned)dsplit),
                                                                                                dim3(256), 0, st, ix->rows, ix->pend_list, npend, B, dsplit, ix->dpad, ix->qn, k,
                                                                                                row_base, deny, delta, m1);
            });
        }
        if (drc != 0) return drc;
        HIP_TRY(hipGetLastError());
        return launch_merge(ix->ivf_partial, B, m1 + (int64_t)dsplit * k, m1, k, (u64*)dev_keys, dev_dist, dev_rows, st, nullptr, nullptr, nullptr, m1, (int64_t)B * m1,
                            kernel_metric(ix->metric));
    };
    const int niter = niter_of(shape_of(ix));
    // 2a. a batch with enough (query, list) pairs to fill the chip without splitting lists: group the pairs by list on the
    //     device and scan every probed list once per kIvfNB of its queries (ivf_scan_shared_kernel)
    const int64_t npairs = (int64_t)B * nprobe;
    //     (worth it once a list is probed by two queries or more on average: below that every work item holds one pair and the
    //     grouping launches are pure overhead — 12.5M x 1024 fp16, 2,048 lists, B = 256: nprobe 8 5.98 ms per pair vs 7.22 shared)
    if (ix->knobs.ivf_share && npairs >= 1024 && npairs >= 2 * (int64_t)ix->ivf_nlist && !(ix->dtype != DT_F32 && niter == 4)) {
        const int nlist = ix->ivf_nlist;
        ix->stat_ivf_shared++;
        HIP_TRY(ix->ivf_group.ensure(3 * (int64_t)nlist + 2 + npairs));
        HIP_TRY(ix->ivf_partial.ensure((npend > 0 ? 2 : 1) * npairs * k));
        unsigned* cnt = ix->ivf_group;
        unsigned* pair_start = cnt + nlist;
        unsigned* item_start = pair_start + nlist + 1;
        unsigned* sorted_pairs = item_start + nlist + 1;
        {
        EvScope ev(ix, EV_SCAN, st);
        HIP_TRY(hipMemsetAsync(cnt, 0, (size_t)nlist * sizeof(unsigned), st));
        HIP_TRY(hipMemsetAsync(ix->ivf_partial, 0, (size_t)(npairs * k) * sizeof(u64), st));  // (an empty probe slot stays an empty list)
        const unsigned pb = (unsigned)((npairs + 255) / 256);
        hipLaunchKernelGGL(ivf_pair_count_kernel, dim3(pb), dim3(256), 0, st, ix->probe_keys, (int)npairs, cnt);
        hipLaunchKernelGGL(ivf_pair_offsets_kernel, dim3(1), dim3(1024), 0, st, cnt, nlist, pair_start, item_start);
        hipLaunchKernelGGL(ivf_pair_scatter_kernel, dim3(pb), dim3(256), 0, st, ix->probe_keys, (int)npairs, pair_start, cnt, sorted_pairs);
        // work items <= sum over lists of ceil(pairs / kIvfNB) <= min(pairs, lists + pairs / kIvfNB): the grid covers the bound, surplus workgroups leave at once
        const int64_t bound = std::min<int64_t>(npairs, (int64_t)nlist + npairs / kIvfNB);
        rc = with_row_form(ix, k, "row too wide for the IVF scan%s", [&](auto dt, auto ni, auto sl) {
            if (sq) {
                // (2-byte rows of 4 chunks per lane never come here, see the condition above: that form is not built)
                if constexpr (decltype(dt)::value != DT_F32 && decltype(ni)::value == 4) {
                    return fail(CODD_KNN_EINVAL, "the shared squared-distance scan takes no 2-byte rows of 4 chunks per lane%s");
                } else {
                    return launch_kernel<ivf_shared_sq<dt, ni, sl>>(dim3((unsigned)bound), dim3(256), 0, st, ix->rows_ivf, ix->ivf_ids, ix->ivf_offsets, pair_start,
                                                                    item_start, sorted_pairs, nlist, nprobe, ix->dpad, ix->qn, k, row_base, ix->ivf_partial, deny_lists);
                }
            }
            return launch_kernel<ivf_scan_shared_kernel<dt, ni, sl>>(dim3((unsigned)bound), dim3(256), 0, st, ix->rows_ivf, ix->ivf_ids, ix->ivf_offsets,
                                                                     pair_start, item_start, sorted_pairs, nlist, nprobe, ix->dpad, ix->qn, k, row_base,
                                                                     ix->ivf_partial, deny_lists);
        });
        if (rc != 0) return rc;
        HIP_TRY(hipGetLastError());
        }
        const int64_t ms = (int64_t)nprobe * k;
        return delta_then_merge(ms, nprobe);
    }
    // 2. scan the probed lists; split each list over several blocks when the batch alone cannot fill the chip
    int split = (int)((4 * (int64_t)ix->num_cus + (int64_t)B * nprobe - 1) / ((int64_t)B * nprobe));
    split = split < 1 ? 1 : (split > 16 ? 16 : split);
    const int64_t m = (int64_t)nprobe * split * k;
    HIP_TRY(ix->ivf_partial.ensure((npend > 0 ? 2 : 1) * (int64_t)B * m));
    const dim3 grid((unsigned)(nprobe * split), (unsigned)B), block(256);
    {
        EvScope ev(ix, EV_SCAN, st);
        rc = with_row_form(ix, k, "row too wide for the IVF scan%s", [&](auto dt, auto ni, auto sl) {
            return launch_by_metric<ivf_scan_sq<dt, ni, sl>, ivf_scan_kernel<dt, ni, sl>>(sq ? kMetricL2 : kMetricDot, grid, block, 0, st, ix->rows_ivf, ix->ivf_ids,
                                                                                          ix->ivf_offsets, ix->probe_keys, nprobe, split, ix->dpad, ix->qn, k, row_base,
                                                                                          ix->ivf_partial, deny_lists);
        });
    }
    if (rc != 0) return rc;
    HIP_TRY(hipGetLastError());
    // 3. top-k of the nprobe*split partial lists
    return delta_then_merge(m, (int64_t)nprobe * split);
}

}  // namespace

extern "C" {

int codd_knn_ivf_search(codd_knn_index* ix, const float* dev_queries, int B, int k, int nprobe, uint32_t row_base,
                        uint64_t* dev_keys, float* dev_dist, int64_t* dev_rows, void* stream) {
    int rc;
    if ((rc = ivf_check_args(ix, dev_queries, B, k, row_base, &nprobe)) != 0) return rc;
    DeviceGuard guard(ix->device);
    hipStream_t st = (hipStream_t)stream;
    WorkScope work(ix, st), work_coarse(ix->coarse, st);
    return ivf_search_body(ix, dev_queries, B, k, nprobe, row_base, dev_keys, dev_dist, dev_rows, st, ix->dead_bits);
}

int codd_knn_ivf_refresh(codd_knn_index* ix, void* stream) {
    if (!ix) return fail(CODD_KNN_EINVAL, "null index%s");
    if (!ix->ivf_follow) return fail(CODD_KNN_EINVAL, "ivf_refresh: option \"ivf_follow\" is off%s");
    if (!ivf_layout_fresh(ix)) return fail(CODD_KNN_EINVAL, "ivf_refresh: no IVF layout, or rows changed since codd_knn_ivf_install%s");
    if (ix->pend.count == 0) return CODD_KNN_OK;   // nothing pending: nothing enqueued
    DeviceGuard guard(ix->device);
    return ivf_fold(ix, (hipStream_t)stream);
}

int codd_knn_set_scopes_host(codd_knn_index* ix, const int64_t* host_slots, const uint32_t* host_scopes, int64_t n) {
    if (!ix || n < 0 || (n > 0 && (!host_slots || !host_scopes))) return fail(CODD_KNN_EINVAL, "bad set_scopes arguments%s");
    if (n == 0) return CODD_KNN_OK;
    uint32_t top = 0;
    bool increasing = true;
    for (int64_t i = 0; i < n; ++i) {
        if (host_slots[i] < 0 || host_slots[i] >= ix->count) return fail(CODD_KNN_EINVAL, "set_scopes: row slot outside [0, count)%s");
        if (slot_dead(ix, host_slots[i])) return fail(CODD_KNN_EINVAL, "set_scopes: deleted row slot (it stays dead until codd_knn_compact)%s");
        if (host_scopes[i] > CODD_KNN_MAX_SCOPE) return fail(CODD_KNN_EINVAL, "set_scopes: scope above CODD_KNN_MAX_SCOPE%s");
        if (host_scopes[i] > top) top = host_scopes[i];
        if (i > 0 && host_slots[i] <= host_slots[i - 1]) increasing = false;
    }
    // (slot, scope) packed into one word each; a slot listed more than once keeps its LAST label (the device writes in no order)
    std::vector<int64_t> packed;
    try {
        packed.resize((size_t)n);
        for (int64_t i = 0; i < n; ++i) packed[(size_t)i] = (int64_t)(((u64)host_scopes[i] << 32) | (u64)host_slots[i]);
        if (!increasing) {
            std::vector<int64_t> order((size_t)n);
            for (int64_t i = 0; i < n; ++i) order[(size_t)i] = i;
            std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return host_slots[a] < host_slots[b]; });
            size_t m = 0;
            for (int64_t i = 0; i < n; ++i)
                if (i + 1 == n || host_slots[order[(size_t)i]] != host_slots[order[(size_t)i + 1]])
                    packed[m++] = (int64_t)(((u64)host_scopes[order[(size_t)i]] << 32) | (u64)host_slots[order[(size_t)i]]);
            packed.resize(m);
        }
    } catch (const std::bad_alloc&) {
        return fail(CODD_KNN_ENOMEM, "host allocation failed%s");
    }
    DeviceGuard guard(ix->device);
    HIP_TRY(hipDeviceSynchronize());
    int rc;
    if ((rc = ensure_scope_labels(ix, nullptr)) != 0) return rc;
    if (ix->stage_slot.cap() < 4096) HIP_TRY(ix->stage_slot.reset(4096));  // (the staging buffer codd_knn_upsert_host keeps between calls)
    const int64_t total = (int64_t)packed.size(), pn = ix->stage_slot.cap();
    for (int64_t i0 = 0; i0 < total; i0 += pn) {
        const int64_t m = total - i0 < pn ? total - i0 : pn;
        HIP_TRY(hipMemcpy(ix->stage_slot, packed.data() + i0, (size_t)m * sizeof(int64_t), hipMemcpyHostToDevice));
        hipLaunchKernelGGL(scope_set_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, nullptr, ix->stage_slot, m, ix->scope_of);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipDeviceSynchronize());  // (the staging buffer is reused by the next piece, and the call is synchronous by contract)
    }
    if (top > ix->max_scope) ix->max_scope = top;
    ix->scope_gen++;
    return CODD_KNN_OK;
}

int codd_knn_search_scoped(codd_knn_index* ix, const float* dev_queries, const uint32_t* dev_scopes, int B, int k, uint32_t row_base,
                           uint64_t* dev_keys, float* dev_dist, int64_t* dev_rows, void* stream) {
    if (!ix || !dev_queries) return fail(CODD_KNN_EINVAL, "null index or queries%s");
    if (!dev_scopes) return fail(CODD_KNN_EINVAL, "null scopes%s");
    int rc;
    if ((rc = search_check_args(ix, dev_queries, B, k, row_base)) != 0) return rc;
    DeviceGuard guard(ix->device);
    hipStream_t st = (hipStream_t)stream;
    WorkScope work(ix, st);
    ix->stat_scoped_searches++;
    const int64_t n = ix->count;
    if ((rc = wait_rows(ix, st)) != 0) return rc;
    if (n == 0) return empty_result(ix, B, k, dev_keys, dev_dist, dev_rows, st);  // nothing stored: all-empty result, as codd_knn_search gives
    // enough work items to fill the chip whatever the batch: a scope's list is cut into `split` parts.  The batch has between
    // ceil(B / 4) (one scope) and B (all different) groups of queries; the lower bound sizes the split, surplus workgroups are cheap.
    const int64_t groups = (B + 3) / 4;
    int split = (int)((4 * (int64_t)ix->num_cus + groups - 1) / groups);
    split = split < 1 ? 1 : (split > 256 ? 256 : split);
    const int64_t m = (int64_t)split * k;
    HIP_TRY(ix->qn.ensure((int64_t)B * ix->dpad));
    HIP_TRY(ix->partial.ensure((int64_t)B * m));
    HIP_TRY(ix->scope_group.ensure((int64_t)2 * CODD_KNN_MAX_BATCH));
    if ((rc = ensure_scope_lists(ix, st)) != 0) return rc;
    if ((rc = prep_exact_queries(ix, dev_queries, B, st)) != 0) return rc;
    unsigned* sorted_q = ix->scope_group;
    unsigned* rank = sorted_q + CODD_KNN_MAX_BATCH;
    hipLaunchKernelGGL(scope_group_kernel, dim3(1), dim3(1024), 0, st, dev_scopes, B, sorted_q, rank);
    HIP_TRY(hipGetLastError());
    {
        EvScope ev(ix, EV_SCAN, st);
        rc = with_row_form(ix, k, "row too wide for the scope scan%s", [&](auto dt, auto ni, auto sl) {
            return launch_by_metric<scope_scan_l2<dt, ni, sl>, scope_scan_kernel<dt, ni, sl>>(
                kernel_metric(ix->metric), dim3((unsigned)B, (unsigned)split), dim3(256), 0, st, ix->rows, ix->scope_perm, ix->scope_offsets,
                n - ix->dead_count, ix->max_scope, dev_scopes, sorted_q, rank, B, split, ix->dpad, ix->qn, k, row_base, ix->partial);
        });
    }
    if (rc != 0) return rc;
    HIP_TRY(hipGetLastError());
    return launch_merge_of(ix, ix->partial, B, m, k, (u64*)dev_keys, dev_dist, dev_rows, st);
}

}  // extern "C"

namespace {

// The body both masked entry points run: the clipped allow words are in ix->mask_allow (written on `st`, or enqueued there) and m > 0,
// the number of allowed live rows, is known on the host.  Chooses the route and enqueues it.
int masked_search_body(codd_knn_index* ix, const float* dev_queries, int B, int k, int64_t nwords, int64_t m, uint32_t row_base,
                       uint64_t* dev_keys, float* dev_dist, int64_t* dev_rows, hipStream_t st) {
    const int64_t n = ix->count;
    int rc;
    if (mask_takes_dense(ix->knobs, shape_of(ix), B, k, m)) {
        ix->stat_mask_dense++;
        const int64_t total_words = (ix->capacity + 31) / 32;   // (as long as the tombstone bits: every kernel that reads those reads these)
        HIP_TRY(ix->mask_deny.ensure(total_words));
        hipLaunchKernelGGL(mask_deny_kernel, dim3((unsigned)((total_words + 255) / 256)), dim3(256), 0, st, ix->mask_allow, ix->dead_bits, n, nwords,
                           total_words, ix->mask_deny);
        HIP_TRY(hipGetLastError());
        std::swap(ix->dstats, ix->mask_dstats);   // (the passes below count into the masked searches' own counters)
        rc = search_impl(ix, dev_queries, B, k, row_base, (u64*)dev_keys, dev_dist, dev_rows, st, ix->mask_deny, true);
        std::swap(ix->dstats, ix->mask_dstats);
        return rc;
    }

    ix->stat_mask_list++;
    const int64_t nblocks = (nwords + 255) / 256;
    HIP_TRY(ix->mask_prefix.ensure(nwords + 2 * nblocks + 1));
    HIP_TRY(ix->mask_list.ensure(m));
    unsigned* prefix = ix->mask_prefix;
    unsigned* block_total = prefix + nwords;
    unsigned* block_base = block_total + nblocks;
    hipLaunchKernelGGL(mask_prefix_kernel, dim3((unsigned)nblocks), dim3(256), 0, st, ix->mask_allow, ix->dead_bits, n, nwords, prefix, block_total);
    hipLaunchKernelGGL(scope_offsets_kernel, dim3(1), dim3(1024), 0, st, block_total, (int)nblocks, block_base);
    hipLaunchKernelGGL(mask_scatter_kernel, dim3((unsigned)nblocks), dim3(256), 0, st, ix->mask_allow, ix->dead_bits, n, nwords, prefix, block_base, m,
                       ix->mask_list);
    HIP_TRY(hipGetLastError());
    // the split of codd_knn_search_scoped, and no more parts than the list has workgroup steps (16 rows)
    const int64_t groups = (B + 3) / 4;
    int split = (int)((4 * (int64_t)ix->num_cus + groups - 1) / groups);
    split = split < 1 ? 1 : (split > 256 ? 256 : split);
    if ((int64_t)split > (m + 15) / 16) split = (int)((m + 15) / 16);
    const int64_t pm = (int64_t)split * k;
    HIP_TRY(ix->qn.ensure((int64_t)B * ix->dpad));
    HIP_TRY(ix->partial.ensure((int64_t)B * pm));
    if ((rc = prep_exact_queries(ix, dev_queries, B, st)) != 0) return rc;
    {
        EvScope ev(ix, EV_SCAN, st);
        rc = with_row_form(ix, k, "row too wide for the mask scan%s", [&](auto dt, auto ni, auto sl) {
            constexpr int NB = scope_nb(decltype(dt)::value, decltype(ni)::value);
            return launch_by_metric<mask_scan_l2<dt, ni, sl>, mask_scan_kernel<dt, ni, sl>>(kernel_metric(ix->metric), dim3((unsigned)((B + NB - 1) / NB), (unsigned)split),
                                                                                            dim3(256), 0, st, ix->rows, ix->mask_list, m, B, split, ix->dpad, ix->qn, k,
                                                                                            row_base, ix->partial);
        });
    }
    if (rc != 0) return rc;
    HIP_TRY(hipGetLastError());
    return launch_merge_of(ix, ix->partial, B, pm, k, (u64*)dev_keys, dev_dist, dev_rows, st);
}

// The host words of a masked search (nwords > 0 of them): clipped to [0, n) into the workspace's pinned staging buffer and counted
// against the tombstone mirror on the way (*m: the rows the call may see, exact, nothing read back).  The caller's words are not
// touched again; the staging buffer's previous copy (the stream's last masked search) is waited for first.
int stage_host_mask(codd_knn_index* ix, const uint32_t* host_allow_bits, int64_t nwords, int64_t n, int64_t* m) {
    if (ix->mask_upload_pending) HIP_TRY(hipEventSynchronize(ix->mask_uploaded));
    ix->mask_upload_pending = false;
    if (nwords > ix->mask_host.cap()) HIP_TRY(ix->mask_host.reset(nwords + nwords / 2 + 64));
    HIP_TRY(ix->mask_uploaded.ensure());
    const bool any_dead = ix->dead_count > 0;
    int64_t seen = 0;
    for (int64_t w = 0; w < nwords; ++w) {
        const int64_t left = n - w * 32;
        const uint32_t a = host_allow_bits[w] & (left >= 32 ? 0xffffffffu : (1u << (uint32_t)left) - 1u);
        ix->mask_host[w] = a;
        seen += __builtin_popcount(any_dead && (size_t)w < ix->dead_host.size() ? a & ~ix->dead_host[(size_t)w] : a);
    }
    *m = seen;
    return CODD_KNN_OK;
}

// ... and one asynchronous copy on `st` takes the staged words to the workspace's allow buffer
int upload_staged_mask(codd_knn_index* ix, int64_t nwords, hipStream_t st) {
    HIP_TRY(ix->mask_allow.ensure(nwords));
    HIP_TRY(hipMemcpyAsync(ix->mask_allow, ix->mask_host, (size_t)nwords * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipEventRecord(ix->mask_uploaded, st));
    ix->mask_upload_pending = true;
    return CODD_KNN_OK;
}

// A masked IVF search behind its mask: `allow` are nwords device words, valid on `st` (the workspace's copy of the
// host words, or the caller's own); deny = ~allow | dead over the nwords words that cover every row slot of the layout goes into the
// workspace's deny buffer and takes the tombstones' place in the list scans.  Nothing depends on how many rows the mask leaves.
int ivf_masked_body(codd_knn_index* ix, const float* dev_queries, int B, int k, int nprobe, const uint32_t* allow, int64_t nwords, uint32_t row_base,
                    uint64_t* dev_keys, float* dev_dist, int64_t* dev_rows, hipStream_t st) {
    HIP_TRY(ix->mask_deny.ensure(nwords));
    hipLaunchKernelGGL(mask_deny_kernel, dim3((unsigned)((nwords + 255) / 256)), dim3(256), 0, st, allow, ix->dead_bits, ix->count, nwords, nwords,
                       ix->mask_deny);
    HIP_TRY(hipGetLastError());
    return ivf_search_body(ix, dev_queries, B, k, nprobe, row_base, dev_keys, dev_dist, dev_rows, st, ix->mask_deny);
}

bool docs_valid(const codd_knn_index* ix) { return ix->doc_arena && ix->doc_epoch == ix->epoch && ix->doc_count == ix->count; }

}  // namespace

extern "C" {

int codd_knn_search_masked(codd_knn_index* ix, const float* dev_queries, int B, int k, const uint32_t* host_allow_bits, int64_t nwords,
                           uint32_t row_base, uint64_t* dev_keys, float* dev_dist, int64_t* dev_rows, void* stream) {
    int rc;
    if ((rc = search_check_args(ix, dev_queries, B, k, row_base)) != 0) return rc;
    DeviceGuard guard(ix->device);
    hipStream_t st = (hipStream_t)stream;
    WorkScope work(ix, st);
    const int64_t n = ix->count;
    if (nwords != (n + 31) / 32) return fail(CODD_KNN_EINVAL, "search_masked: nwords must be ceil(count / 32)%s");
    if (nwords > 0 && !host_allow_bits) return fail(CODD_KNN_EINVAL, "null allow bits%s");
    ix->stat_masked_searches++;
    if ((rc = wait_rows(ix, st)) != 0) return rc;
    // The host words: clipped to [0, count) into the workspace's pinned staging buffer, counted against the tombstone mirror on
    // the way (m: the rows this call may see, exact, nothing read back), then one asynchronous copy from the staging buffer.  The
    // caller's words are not touched again; the staging buffer's previous copy (the stream's last masked search) is waited for first.
    int64_t m = 0;
    if (nwords > 0 && (rc = stage_host_mask(ix, host_allow_bits, nwords, n, &m)) != 0) return rc;
    ix->stat_last_mask_rows = m;
    if (m == 0) return empty_result(ix, B, k, dev_keys, dev_dist, dev_rows, st);
    if ((rc = upload_staged_mask(ix, nwords, st)) != 0) return rc;
    return masked_search_body(ix, dev_queries, B, k, nwords, m, row_base, dev_keys, dev_dist, dev_rows, st);
}

int codd_knn_search_masked_dev(codd_knn_index* ix, const float* dev_queries, int B, int k, const uint32_t* dev_allow_bits, int64_t nwords,
                               uint32_t row_base, uint64_t* dev_keys, float* dev_dist, int64_t* dev_rows, void* stream) {
    int rc;
    if ((rc = search_check_args(ix, dev_queries, B, k, row_base)) != 0) return rc;
    DeviceGuard guard(ix->device);
    hipStream_t st = (hipStream_t)stream;
    WorkScope work(ix, st);
    const int64_t n = ix->count;
    if (nwords != (n + 31) / 32) return fail(CODD_KNN_EINVAL, "search_masked_dev: nwords must be ceil(count / 32)%s");
    if (nwords > 0 && !dev_allow_bits) return fail(CODD_KNN_EINVAL, "null allow bits%s");
    ix->stat_masked_searches++;
    ix->stat_masked_dev++;
    if ((rc = wait_rows(ix, st)) != 0) return rc;
    // The device words: clipped to [0, count) into the workspace's allow buffer and counted against the tombstone bits by one small
    // kernel behind whatever wrote them on `st`; the count comes back through pinned memory — the one host synchronisation of the call
    // (m chooses the route and sizes the list).
    int64_t m = 0;
    if (nwords > 0) {
        if (!ix->mask_m_dev) HIP_TRY(ix->mask_m_dev.reset(1));
        if (!ix->mask_m_host) HIP_TRY(ix->mask_m_host.reset(1));
        HIP_TRY(ix->mask_allow.ensure(nwords));
        HIP_TRY(hipMemsetAsync(ix->mask_m_dev, 0, sizeof(unsigned long long), st));
        hipLaunchKernelGGL(mask_clip_count_kernel, dim3((unsigned)((nwords + 255) / 256)), dim3(256), 0, st, dev_allow_bits, ix->dead_bits, n, nwords,
                           ix->mask_allow, ix->mask_m_dev);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(ix->mask_m_host, ix->mask_m_dev, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        m = (int64_t)*ix->mask_m_host;
    }
    ix->stat_last_mask_rows = m;
    if (m == 0) return empty_result(ix, B, k, dev_keys, dev_dist, dev_rows, st);
    return masked_search_body(ix, dev_queries, B, k, nwords, m, row_base, dev_keys, dev_dist, dev_rows, st);
}

int codd_knn_ivf_search_masked(codd_knn_index* ix, const float* dev_queries, int B, int k, int nprobe, const uint32_t* host_allow_bits, int64_t nwords,
                               uint32_t row_base, uint64_t* dev_keys, float* dev_dist, int64_t* dev_rows, void* stream) {
    int rc;
    if ((rc = ivf_check_args(ix, dev_queries, B, k, row_base, &nprobe)) != 0) return rc;
    DeviceGuard guard(ix->device);
    hipStream_t st = (hipStream_t)stream;
    WorkScope work(ix, st), work_coarse(ix->coarse, st);
    const int64_t n = ix->count;   // (>= 1: a layout exists)
    if (nwords != (n + 31) / 32) return fail(CODD_KNN_EINVAL, "ivf_search_masked: nwords must be ceil(count / 32)%s");
    if (!host_allow_bits) return fail(CODD_KNN_EINVAL, "null allow bits%s");
    ix->stat_ivf_masked++;
    int64_t m = 0;   // (counted by the staging pass, not needed: nothing here depends on it)
    if ((rc = stage_host_mask(ix, host_allow_bits, nwords, n, &m)) != 0) return rc;
    if ((rc = upload_staged_mask(ix, nwords, st)) != 0) return rc;
    return ivf_masked_body(ix, dev_queries, B, k, nprobe, ix->mask_allow, nwords, row_base, dev_keys, dev_dist, dev_rows, st);
}

int codd_knn_ivf_search_masked_dev(codd_knn_index* ix, const float* dev_queries, int B, int k, int nprobe, const uint32_t* dev_allow_bits, int64_t nwords,
                                   uint32_t row_base, uint64_t* dev_keys, float* dev_dist, int64_t* dev_rows, void* stream) {
    int rc;
    if ((rc = ivf_check_args(ix, dev_queries, B, k, row_base, &nprobe)) != 0) return rc;
    DeviceGuard guard(ix->device);
    hipStream_t st = (hipStream_t)stream;
    WorkScope work(ix, st), work_coarse(ix->coarse, st);
    if (nwords != (ix->count + 31) / 32) return fail(CODD_KNN_EINVAL, "ivf_search_masked_dev: nwords must be ceil(count / 32)%s");
    if (!dev_allow_bits) return fail(CODD_KNN_EINVAL, "null allow bits%s");
    ix->stat_ivf_masked++;
    // the caller's words are read once, by mask_deny_kernel on `st` (which clips them to [0, count) itself): no count, no read-back
    return ivf_masked_body(ix, dev_queries, B, k, nprobe, dev_allow_bits, nwords, row_base, dev_keys, dev_dist, dev_rows, st);
}

int codd_knn_slice_mask(int device, const uint32_t* dev_global_bits, int64_t global_rows, int64_t row_base, int64_t count, uint32_t* dev_out,
                        int64_t nwords, void* stream) {
    if (global_rows < 0 || row_base < 0 || count < 0) return fail(CODD_KNN_EINVAL, "slice_mask: negative global_rows, row_base or count%s");
    if (nwords != (count + 31) / 32) return fail(CODD_KNN_EINVAL, "slice_mask: nwords must be ceil(count / 32)%s");
    if (nwords == 0) return CODD_KNN_OK;
    if (!dev_out || (global_rows > 0 && !dev_global_bits)) return fail(CODD_KNN_EINVAL, "slice_mask: null words%s");
    DeviceGuard guard(device);
    const int rc = launch_kernel<mask_slice_kernel>(dim3((unsigned)((nwords + 255) / 256)), dim3(256), 0, (hipStream_t)stream, dev_global_bits, global_rows,
                                                    row_base, count, dev_out, nwords);
    if (rc != 0) return rc;
    HIP_TRY(hipGetLastError());
    return CODD_KNN_OK;
}

int codd_knn_set_documents_host(codd_knn_index* ix, const uint8_t* host_bytes, const int64_t* host_offsets, int64_t n) {
    if (!ix || !host_offsets || n < 0) return fail(CODD_KNN_EINVAL, "set_documents: null index or offsets%s");
    if (n != ix->count) return fail(CODD_KNN_EINVAL, "set_documents: n must equal the count (one document per row slot)%s");
    if (host_offsets[0] != 0) return fail(CODD_KNN_EINVAL, "set_documents: offsets must start at 0%s");
    for (int64_t r = 0; r < n; ++r)
        if (host_offsets[r + 1] < host_offsets[r]) return fail(CODD_KNN_EINVAL, "set_documents: offsets must be non-decreasing%s");
    const int64_t total = host_offsets[n];
    if (total > 0 && !host_bytes) return fail(CODD_KNN_EINVAL, "set_documents: null bytes%s");
    if (total > 0 && memchr(host_bytes, 0, (size_t)total)) return fail(CODD_KNN_EINVAL, "set_documents: a document holds a 0x00 byte%s");
    DeviceGuard guard(ix->device);
    HIP_TRY(hipDeviceSynchronize());
    // the arena on the host first: document r at host_offsets[r] + r, its separator behind it, zeros to the end of the allocation
    const int64_t bytes = total + n, alloc = doc_arena_alloc_bytes(bytes);
    std::vector<uint8_t> arena;
    std::vector<int64_t> offsets;
    try {
        arena.assign((size_t)alloc, (uint8_t)0);
        offsets.resize((size_t)n + 1);
    } catch (const std::bad_alloc&) {
        return fail(CODD_KNN_ENOMEM, "host allocation failed%s");
    }
    for (int64_t r = 0; r < n; ++r) {
        offsets[(size_t)r] = host_offsets[r] + r;
        const int64_t len = host_offsets[r + 1] - host_offsets[r];
        if (len > 0) memcpy(arena.data() + offsets[(size_t)r], host_bytes + host_offsets[r], (size_t)len);
    }
    offsets[(size_t)n] = bytes;
    DevBuf<uint8_t> dev_arena;
    DevBuf<int64_t> dev_offsets;
    hipError_t e = dev_arena.reset(alloc);
    if (e == hipSuccess) e = dev_offsets.reset(n + 1);
    if (e == hipSuccess) e = hipMemcpy(dev_arena, arena.data(), (size_t)alloc, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dev_offsets, offsets.data(), ((size_t)n + 1) * sizeof(int64_t), hipMemcpyHostToDevice);
    // (on failure the previous snapshot stays as it was)
    if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? CODD_KNN_ENOMEM : CODD_KNN_EDEVICE, "set_documents: upload failed: %s", hipGetErrorString(e));
    ix->doc_arena = std::move(dev_arena);
    ix->doc_offsets = std::move(dev_offsets);
    ix->doc_bytes = bytes;
    ix->doc_count = n;
    ix->doc_epoch = ix->epoch;
    return CODD_KNN_OK;
}

int codd_knn_match_documents(codd_knn_index* ix, const uint8_t* host_needle, int needle_len, uint32_t* dev_bits, int64_t nwords, void* stream) {
    if (!ix || !host_needle) return fail(CODD_KNN_EINVAL, "match_documents: null index or needle%s");
    if (needle_len < 1 || needle_len > CODD_KNN_MAX_NEEDLE) return fail(CODD_KNN_EINVAL, "match_documents: needle_len out of range [1,256]%s");
    if (memchr(host_needle, 0, (size_t)needle_len)) return fail(CODD_KNN_EINVAL, "match_documents: the needle holds a 0x00 byte%s");
    static_assert(kDocMaxNeedle == CODD_KNN_MAX_NEEDLE, "doc_match.h and codd_knn.h disagree");
    DeviceGuard guard(ix->device);
    hipStream_t st = (hipStream_t)stream;
    std::lock_guard<std::mutex> lock(ix->mu);   // (no workspace: the kernel reads the snapshot and writes the caller's words)
    if (!docs_valid(ix)) return fail(CODD_KNN_EINVAL, "match_documents: no document snapshot, or a stale one (rows changed since codd_knn_set_documents_host)%s");
    if (nwords != (ix->count + 31) / 32) return fail(CODD_KNN_EINVAL, "match_documents: nwords must be ceil(count / 32)%s");
    if (nwords == 0) return CODD_KNN_OK;
    if (!dev_bits) return fail(CODD_KNN_EINVAL, "match_documents: null bits%s");
    DocNeedle needle;
    memset(&needle, 0, sizeof(needle));
    memcpy(needle.w, host_needle, (size_t)needle_len);
    HIP_TRY(hipMemsetAsync(dev_bits, 0, (size_t)nwords * sizeof(uint32_t), st));
    const int64_t tiles = (ix->doc_bytes + kDocTile - 1) / kDocTile;
    const int64_t most = (int64_t)ix->num_cus * 8;   // (grid-stride beyond eight workgroups per compute unit)
    const int rc = launch_kernel<doc_match_kernel>(dim3((unsigned)(tiles < most ? tiles : most)), dim3(kDocThreads), 0, st,
                                                   reinterpret_cast<const uint4*>(ix->doc_arena.get()), ix->doc_bytes, tiles, ix->doc_offsets, ix->count, needle,
                                                   needle_len, dev_bits);
    if (rc != 0) return rc;
    HIP_TRY(hipGetLastError());
    ix->stat_doc_matches++;
    return CODD_KNN_OK;
}

int codd_knn_match_documents_dfa(codd_knn_index* ix, const uint8_t* host_class_of, const uint8_t* host_next, int nstates, int nclasses, int start, int accept,
                                 uint32_t* dev_bits, int64_t nwords, void* stream) {
    if (!ix || !host_class_of || !host_next) return fail(CODD_KNN_EINVAL, "match_documents_dfa: null index, class map or table%s");
    static_assert(kRegexMaxStates == CODD_KNN_MAX_DFA_STATES && kRegexMaxTable == CODD_KNN_MAX_DFA_TABLE, "doc_regex.h and codd_knn.h disagree");
    // the table is checked here, entry by entry, before anything is enqueued: on the device no entry leads outside it
    if (nstates < 1 || nstates > CODD_KNN_MAX_DFA_STATES) return fail(CODD_KNN_EINVAL, "match_documents_dfa: nstates out of range [1,255]%s");
    if (nclasses < 1 || nclasses > 256) return fail(CODD_KNN_EINVAL, "match_documents_dfa: nclasses out of range [1,256]%s");
    const int entries = nstates * nclasses;
    if (entries > CODD_KNN_MAX_DFA_TABLE) return fail(CODD_KNN_EINVAL, "match_documents_dfa: the table exceeds CODD_KNN_MAX_DFA_TABLE bytes%s");
    if (start < 0 || start >= nstates || accept < 0 || accept >= nstates) return fail(CODD_KNN_EINVAL, "match_documents_dfa: start or accept is not a state%s");
    for (int b = 0; b < 256; ++b)
        if (host_class_of[b] >= nclasses) return fail(CODD_KNN_EINVAL, "match_documents_dfa: a byte's class is not below nclasses%s");
    for (int i = 0; i < entries; ++i)
        if (host_next[i] >= nstates) return fail(CODD_KNN_EINVAL, "match_documents_dfa: a table entry is not a state%s");
    for (int c = 0; c < nclasses; ++c)
        if (host_next[accept * nclasses + c] != accept) return fail(CODD_KNN_EINVAL, "match_documents_dfa: the accepting state must be absorbing%s");
    int reject = -1;   // an absorbing state other than accept, if the table has one: a lane stops reading there too
    for (int s = 0; s < nstates && reject < 0; ++s) {
        bool absorbing = s != accept;
        for (int c = 0; c < nclasses && absorbing; ++c) absorbing = host_next[s * nclasses + c] == s;
        if (absorbing) reject = s;
    }
    DeviceGuard guard(ix->device);
    hipStream_t st = (hipStream_t)stream;
    WorkScope work(ix, st);   // (holds the index's enqueue lock from the checks below to the launch: the snapshot checked is the snapshot read)
    if (!docs_valid(ix)) return fail(CODD_KNN_EINVAL, "match_documents_dfa: no document snapshot, or a stale one (rows changed since codd_knn_set_documents_host)%s");
    if (nwords != (ix->count + 31) / 32) return fail(CODD_KNN_EINVAL, "match_documents_dfa: nwords must be ceil(count / 32)%s");
    if (nwords == 0) return CODD_KNN_OK;
    if (!dev_bits) return fail(CODD_KNN_EINVAL, "match_documents_dfa: null bits%s");
    // the class map and the table: into the stream's pinned staging buffer (its previous copy is waited for first), one copy on `st`
    if (ix->dfa_upload_pending) HIP_TRY(hipEventSynchronize(ix->dfa_uploaded));
    ix->dfa_upload_pending = false;
    HIP_TRY(ix->dfa_host.ensure(kRegexTableWords));
    HIP_TRY(ix->dfa_dev.ensure(kRegexTableWords));
    HIP_TRY(ix->dfa_uploaded.ensure());
    const int table_words = (entries + 3) / 4, words = kRegexClassWords + table_words;
    memset(ix->dfa_host.get(), 0, (size_t)words * sizeof(uint32_t));
    memcpy(ix->dfa_host.get(), host_class_of, 256);
    memcpy(ix->dfa_host.get() + kRegexClassWords, host_next, (size_t)entries);
    HIP_TRY(hipMemcpyAsync(ix->dfa_dev, ix->dfa_host, (size_t)words * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipEventRecord(ix->dfa_uploaded, st));
    ix->dfa_upload_pending = true;
    const int64_t runs = (ix->count + kRegexDocs - 1) / kRegexDocs;
    const int rc = launch_kernel<doc_regex_kernel>(dim3((unsigned)runs), dim3(kRegexDocs), 0, st, reinterpret_cast<const uint4*>(ix->doc_arena.get()), ix->doc_offsets,
                                                   ix->count, ix->dfa_dev, table_words, nclasses, start, accept, reject, dev_bits, nwords);
    if (rc != 0) return rc;
    HIP_TRY(hipGetLastError());
    ix->stat_doc_regex_matches++;
    return CODD_KNN_OK;
}

int codd_knn_embedder_create(codd_knn_embedder** out, int device, int dim, float trigram_weight) {
    if (!out) return fail(CODD_KNN_EINVAL, "embedder_create: null out pointer%s");
    *out = nullptr;
    static_assert(kEmbedMaxDim == 4096 && kEmbedMinDim == 8, "text_embed.h and codd_knn.h disagree");
    if (dim < kEmbedMinDim || dim > kEmbedMaxDim) return fail(CODD_KNN_EINVAL, "embedder_create: dim out of range [8,4096]%s");
    if (!(trigram_weight - trigram_weight == 0.0f)) return fail(CODD_KNN_EINVAL, "embedder_create: trigram_weight must be finite%s");
    if (device < 0) return fail(CODD_KNN_EINVAL, "embedder_create: no such device%s");
    codd_knn_embedder* e = new (std::nothrow) codd_knn_embedder();
    if (!e) return fail(CODD_KNN_ENOMEM, "host allocation failed%s");
    e->device = device;
    e->dim = dim;
    e->trigram_weight = trigram_weight;
    *out = e;
    return CODD_KNN_OK;
}

int codd_knn_embedder_destroy(codd_knn_embedder* e) {
    if (!e) return CODD_KNN_OK;
    if (e->device_seen) {   // (its buffers and events free themselves: the device is current and idle, as their destructors need)
        DeviceGuard guard(e->device);
        (void)hipDeviceSynchronize();
        delete e;
    } else {
        delete e;
    }
    return CODD_KNN_OK;
}

int codd_knn_embed_texts_host(codd_knn_embedder* e, const uint8_t* host_bytes, const int64_t* host_offsets, int64_t n, float* dev_out, void* stream) {
    if (!e || !host_offsets || n < 0) return fail(CODD_KNN_EINVAL, "embed_texts: null embedder or offsets, or negative n%s");
    if (n > CODD_KNN_MAX_EMBED_TEXTS) return fail(CODD_KNN_EINVAL, "embed_texts: more than CODD_KNN_MAX_EMBED_TEXTS texts%s");
    if (host_offsets[0] != 0) return fail(CODD_KNN_EINVAL, "embed_texts: offsets must start at 0%s");
    for (int64_t r = 0; r < n; ++r)
        if (host_offsets[r + 1] < host_offsets[r]) return fail(CODD_KNN_EINVAL, "embed_texts: offsets must be non-decreasing%s");
    const int64_t total = host_offsets[n];
    if (total > CODD_KNN_MAX_EMBED_BYTES) return fail(CODD_KNN_EINVAL, "embed_texts: more than CODD_KNN_MAX_EMBED_BYTES bytes of text%s");
    if (total > 0 && !host_bytes) return fail(CODD_KNN_EINVAL, "embed_texts: null bytes%s");
    unsigned char seen = 0;
    for (int64_t i = 0; i < total; ++i) seen |= host_bytes[i];
    if (seen & 0x80) return fail(CODD_KNN_EINVAL, "embed_texts: a byte at or above 0x80 (ASCII only: other texts are embedded on the host)%s");
    if (n == 0) return CODD_KNN_OK;
    if (!dev_out) return fail(CODD_KNN_EINVAL, "embed_texts: null output%s");
    std::lock_guard<std::mutex> lock(e->mu);
    if (!e->device_seen) {
        int ndev = 0;
        HIP_TRY(hipGetDeviceCount(&ndev));
        if (e->device >= ndev) return fail(CODD_KNN_EINVAL, "embed_texts: no such device%s");
        e->device_seen = true;
    }
    DeviceGuard guard(e->device);
    hipStream_t st = (hipStream_t)stream;
    // the staging buffer: the previous call's copy has to have left it — the only wait on the host; its kernel is not waited for
    if (e->upload_pending) HIP_TRY(hipEventSynchronize(e->uploaded));
    e->upload_pending = false;
    const int64_t off_bytes = (n + 1) * (int64_t)sizeof(int64_t), need = off_bytes + total;
    if (need > e->stage_host.cap()) HIP_TRY(e->stage_host.reset(need + need / 2 + 4096));
    HIP_TRY(e->stage_dev.ensure(e->stage_host.cap()));
    HIP_TRY(e->uploaded.ensure());
    HIP_TRY(e->embedded.ensure());
    memcpy(e->stage_host.get(), host_offsets, (size_t)off_bytes);
    if (total > 0) memcpy(e->stage_host.get() + off_bytes, host_bytes, (size_t)total);
    // the device copy may still be read by the previous call's kernel on another stream: this stream waits for it on the device
    if (e->embedded_set && e->last_stream != st) HIP_TRY(hipStreamWaitEvent(st, e->embedded, 0));
    HIP_TRY(hipMemcpyAsync(e->stage_dev, e->stage_host, (size_t)need, hipMemcpyHostToDevice, st));
    HIP_TRY(hipEventRecord(e->uploaded, st));
    e->upload_pending = true;
    const int64_t most = (int64_t)1 << 20;   // (grid-stride beyond that many texts)
    const int rc = launch_kernel<text_embed_kernel>(dim3((unsigned)(n < most ? n : most)), dim3(kEmbedThreads), (size_t)e->dim * sizeof(float), st,
                                                    (const uint8_t*)(e->stage_dev.get() + off_bytes), reinterpret_cast<const int64_t*>(e->stage_dev.get()), n,
                                                    e->dim, e->trigram_weight, dev_out);
    if (rc != 0) return rc;
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(e->embedded, st));
    e->embedded_set = true;
    e->last_stream = st;
    return CODD_KNN_OK;
}

int codd_knn_delete_host(codd_knn_index* ix, const int64_t* host_slots, int64_t n) {
    if (!ix || n < 0 || (n > 0 && !host_slots)) return fail(CODD_KNN_EINVAL, "bad delete arguments%s");
    for (int64_t i = 0; i < n; ++i)
        if (host_slots[i] < 0 || host_slots[i] >= ix->count) return fail(CODD_KNN_EINVAL, "delete: row slot outside [0, count)%s");
    if (n == 0) return CODD_KNN_OK;
    DeviceGuard guard(ix->device);
    HIP_TRY(hipDeviceSynchronize());
    int rc;
    if ((rc = grow_dead_bits(ix, ix->capacity)) != 0) return rc;
    // the slots that are not dead yet, each once (an already-dead or repeated slot is a no-op): marked in the host mirror first,
    // taken back if the device cannot follow
    std::vector<int64_t> fresh;
    try {
        for (int64_t i = 0; i < n; ++i) {
            uint32_t& word = ix->dead_host[(size_t)(host_slots[i] >> 5)];
            const uint32_t bit = 1u << (uint32_t)(host_slots[i] & 31);
            if (word & bit) continue;
            fresh.push_back(host_slots[i]);
            word |= bit;
        }
    } catch (const std::bad_alloc&) {
        for (int64_t slot : fresh) ix->dead_host[(size_t)(slot >> 5)] &= ~(1u << (uint32_t)(slot & 31));
        return fail(CODD_KNN_ENOMEM, "host allocation failed%s");
    }
    auto undo = [&]() {
        for (int64_t slot : fresh) ix->dead_host[(size_t)(slot >> 5)] &= ~(1u << (uint32_t)(slot & 31));
        if (ix->dead_bits) (void)hipMemcpy(ix->dead_bits, ix->dead_host.data(), (size_t)ix->dead_bits.bytes(), hipMemcpyHostToDevice);
    };
    // the staging buffer codd_knn_upsert_host keeps between calls, grown once to hold the call's slots (at most 1M of them, 8 MiB:
    // a piece costs a copy, a launch and a synchronisation — 5M slots through 4,096-slot pieces were 1,221 such round trips)
    const int64_t total = (int64_t)fresh.size();
    const int64_t want = total < 4096 ? 4096 : (total < (1ll << 20) ? total : (1ll << 20));
    if (ix->stage_slot.cap() < want && ix->stage_slot.reset(want) != hipSuccess) {
        (void)hipGetLastError();
        undo();
        return fail(CODD_KNN_ENOMEM, "delete: staging buffer%s");
    }
    const int64_t pn = ix->stage_slot.cap();
    for (int64_t i0 = 0; i0 < total; i0 += pn) {
        const int64_t m = total - i0 < pn ? total - i0 : pn;
        hipError_t e = hipMemcpy(ix->stage_slot, fresh.data() + i0, (size_t)m * sizeof(int64_t), hipMemcpyHostToDevice);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(dead_set_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, nullptr, ix->stage_slot, m, ix->dead_bits);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipDeviceSynchronize();  // (the staging buffer is reused by the next piece, and the call is synchronous by contract)
        if (e != hipSuccess) {
            undo();
            return fail(CODD_KNN_EDEVICE, "delete: setting the tombstone bits failed: %s", hipGetErrorString(e));
        }
    }
    ix->stat_delete_calls++;
    if (total == 0) return CODD_KNN_OK;
    ix->dead_count += total;
    for (int64_t slot : fresh)
        if (slot < ix->first_dead) ix->first_dead = slot;
    ix->scope_gen++;  // the scope lists leave dead rows out: rebuilt by the next scoped search, like after a label change
    // (no epoch bump: the stored rows and both shadows are what they were, and an installed IVF layout stays valid — its scans
    //  mask by the original row slot)
    return CODD_KNN_OK;
}

int codd_knn_live_count(const codd_knn_index* ix, int64_t* out) {
    if (!ix || !out) return fail(CODD_KNN_EINVAL, "bad live_count arguments%s");
    *out = ix->count - ix->dead_count;
    return CODD_KNN_OK;
}

int codd_knn_compact(codd_knn_index* ix, int64_t* new_count) {
    if (!ix) return fail(CODD_KNN_EINVAL, "null index%s");
    if (ix->dead_count == 0) {
        if (new_count) *new_count = ix->count;
        return CODD_KNN_OK;
    }
    DeviceGuard guard(ix->device);
    HIP_TRY(hipDeviceSynchronize());
    const int64_t n = ix->count, live = n - ix->dead_count, first = ix->first_dead;
    const size_t row_bytes = (size_t)ix->dpad * elem_size(ix->dtype);
    const int cpr = (int)(row_bytes / 16);
    // source rows per chunk: what the bounce buffer (the staging buffer of codd_knn_upsert_host, at most 64 MiB) holds
    int64_t chunk = ix->compact_chunk_rows > 0 ? ix->compact_chunk_rows : (int64_t)((64ull << 20) / row_bytes);
    if (chunk > n - first) chunk = n - first;
    if (chunk < 1) chunk = 1;
    const int64_t bounce_floats = (chunk * (int64_t)row_bytes + 3) / 4;
    if (bounce_floats > ix->stage_vec.cap()) HIP_TRY(ix->stage_vec.reset(bounce_floats < 65536 ? 65536 : bounce_floats));
    if ((chunk + 1) / 2 > ix->stage_slot.cap())  // the chunk's scope labels, 4 bytes each
        HIP_TRY(ix->stage_slot.reset((chunk + 1) / 2 < 4096 ? 4096 : (chunk + 1) / 2));
    // new slot of a live row = its rank among the live rows: prefix sums over the bitmap, on the device
    const int64_t nwords = (n + 31) / 32, nblocks = (nwords + 255) / 256;
    DevBuf<unsigned> sums;   // [nwords] per-word prefix, [nblocks] block totals, [nblocks + 1] block bases
    HIP_TRY(sums.reset(nwords + 2 * nblocks + 1));
    // the metadata columns move out of place, into zero-filled copies allocated before any row moves (nothing has changed if HBM is short)
    codd_knn_index::WhereColumn moved_columns[CODD_KNN_MAX_COLUMNS];
    for (int c = 0; c < CODD_KNN_MAX_COLUMNS; ++c) {
        if (!ix->columns[c].tags) continue;
        HIP_TRY(moved_columns[c].tags.reset(ix->capacity));
        HIP_TRY(moved_columns[c].cells.reset(ix->capacity));
        HIP_TRY(hipMemsetAsync(moved_columns[c].tags, 0, (size_t)ix->capacity, nullptr));
        HIP_TRY(hipMemsetAsync(moved_columns[c].cells, 0, (size_t)ix->capacity * sizeof(uint64_t), nullptr));
    }
    unsigned* prefix = sums;
    unsigned* block_total = prefix + nwords;
    unsigned* block_base = block_total + nblocks;
    hipLaunchKernelGGL(live_prefix_kernel, dim3((unsigned)nblocks), dim3(256), 0, nullptr, ix->dead_bits, n, nwords, prefix, block_total);
    hipLaunchKernelGGL(scope_offsets_kernel, dim3(1), dim3(1024), 0, nullptr, block_total, (int)nblocks, block_base);
    hipError_t e = hipGetLastError();
    // ascending chunks of source rows from the first dead slot on (the rows below it stay where they are), ordered on one stream
    uint4* rows4 = reinterpret_cast<uint4*>(ix->rows.get());
    uint4* bounce = reinterpret_cast<uint4*>(ix->stage_vec.get());
    uint32_t* bounce_scope = reinterpret_cast<uint32_t*>(ix->stage_slot.get());
    int64_t dbase = first;  // every slot below the first dead one is live
    for (int64_t s0 = first; s0 < n && e == hipSuccess; s0 += chunk) {
        const int64_t s1 = s0 + chunk < n ? s0 + chunk : n;
        const int64_t moved = live_in_range(ix, s0, s1);
        if (moved == 0) continue;
        hipLaunchKernelGGL(compact_gather_kernel, dim3((unsigned)((s1 - s0 + 3) / 4)), dim3(256), 0, nullptr, rows4, ix->dead_bits, n, prefix, block_base,
                           ix->scope_of, s0, s1, dbase, chunk, cpr, bounce, bounce_scope);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(ix->rows + (size_t)dbase * row_bytes, bounce, (size_t)moved * row_bytes, hipMemcpyDeviceToDevice, nullptr);
        if (e == hipSuccess && ix->scope_of)
            e = hipMemcpyAsync(ix->scope_of + dbase, bounce_scope, (size_t)moved * sizeof(uint32_t), hipMemcpyDeviceToDevice, nullptr);
        dbase += moved;
    }
    // the columns by the same mapping, while the tombstone bits still stand: slots below the first dead one stay, the rest go to their ranks
    for (int c = 0; c < CODD_KNN_MAX_COLUMNS && e == hipSuccess; ++c) {
        codd_knn_index::WhereColumn& from = ix->columns[c];
        codd_knn_index::WhereColumn& to = moved_columns[c];
        if (!from.tags) continue;
        if (first > 0) {
            e = hipMemcpyAsync(to.tags, from.tags, (size_t)first, hipMemcpyDeviceToDevice, nullptr);
            if (e == hipSuccess) e = hipMemcpyAsync(to.cells, from.cells, (size_t)first * sizeof(uint64_t), hipMemcpyDeviceToDevice, nullptr);
        }
        if (e == hipSuccess) {
            hipLaunchKernelGGL(column_compact_kernel, dim3((unsigned)((n - first + 255) / 256)), dim3(256), 0, nullptr, ix->dead_bits, n, prefix, block_base,
                               first, from.tags, from.cells, to.tags, to.cells);
            e = hipGetLastError();
        }
    }
    // the slots past the live rows are new slots again: no label, no tombstone; the int8 shadow's scales there read "no such row"
    // ... and zero rows: a later write past the new count that does not regrow the store brings them back below the count
    if (e == hipSuccess) e = hipMemsetAsync(ix->rows + (size_t)live * row_bytes, 0, (size_t)(n - live) * row_bytes, nullptr);
    if (e == hipSuccess && ix->scope_of) e = hipMemsetAsync(ix->scope_of + live, 0, (size_t)(n - live) * sizeof(uint32_t), nullptr);
    if (e == hipSuccess) e = hipMemsetAsync(ix->dead_bits, 0, (size_t)ix->dead_bits.bytes(), nullptr);
    if (e == hipSuccess && ix->rscale) {
        const int64_t hi = n < ix->shadow8_rows ? n : ix->shadow8_rows;
        if (hi > live) e = hipMemsetD32Async((hipDeviceptr_t)(ix->rscale + live), (int)0x7fc00000, (size_t)(hi - live), nullptr);
        const int64_t b0 = (live + 31) / 32, b1 = (hi + 31) / 32;
        if (e == hipSuccess && b1 > b0) e = hipMemsetD32Async((hipDeviceptr_t)(ix->bmeta + b0), (int)0x7fc00000, (size_t)(b1 - b0) * 2, nullptr);
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    // A device failure in the middle leaves rows partly moved under an unchanged bitmap and count: the index is unusable from
    // then on (destroy it and rebuild the collection), as the header says.  Nothing short of a device error gets here.
    if (e != hipSuccess) return fail(CODD_KNN_EDEVICE, "compaction failed, the index is unusable: %s", hipGetErrorString(e));
    if (dbase != live) return fail(CODD_KNN_EDEVICE, "compaction: the host's row mapping disagrees with its dead count%s");
    for (int c = 0; c < CODD_KNN_MAX_COLUMNS; ++c)
        if (ix->columns[c].tags) ix->columns[c] = std::move(moved_columns[c]);
    std::fill(ix->dead_host.begin(), ix->dead_host.end(), 0u);
    ix->count = live;
    ix->dead_count = 0;
    ix->first_dead = INT64_MAX;
    ix->rows_event_set = false;  // (everything is complete on the device)
    ix->reader_event_set = false;
    // both shadows are dirty from the first dead slot on (and the last live row's 32-row block is quantised again: its scale
    // spanned rows that are gone); the epoch bump makes an installed IVF layout stale, as after an upsert
    // A dirty range still pending from earlier upserts may reach past the new count (the count never shrank before compaction
    // existed): cut it back first — a shadow build over rows past the count would write past a shadow sized for the count.
    // Every pending dirty row at or behind `first` has moved to a slot in [first, live): the widened range below covers it.
    auto cut = [&](int64_t& dlo, int64_t& dhi) {
        if (dhi > live) dhi = live;
        if (dlo > dhi) dlo = dhi;
    };
    cut(ix->dirty_lo, ix->dirty_hi);
    cut(ix->dirty16_lo, ix->dirty16_hi);
    const int64_t lo = live > 0 ? (first < live - 1 ? first : live - 1) : 0;
    rows_written(ix, lo, live);
    ix->scope_gen++;
    ix->stat_compactions++;
    if (new_count) *new_count = live;
    return CODD_KNN_OK;
}

int codd_knn_set_column_host(codd_knn_index* ix, int column, const int64_t* host_slots, const uint8_t* host_tags, const uint64_t* host_cells, int64_t n) {
    if (!ix || n < 0 || (n > 0 && (!host_tags || !host_cells))) return fail(CODD_KNN_EINVAL, "bad set_column arguments%s");
    if (column < 0 || column >= CODD_KNN_MAX_COLUMNS) return fail(CODD_KNN_EINVAL, "set_column: column outside [0, CODD_KNN_MAX_COLUMNS)%s");
    if (ix->capacity <= 0 || ix->count <= 0) return fail(CODD_KNN_EINVAL, "set_column: the index holds no row slot%s");
    if (!host_slots && n > ix->count) return fail(CODD_KNN_EINVAL, "set_column: a full upload holds at most count rows%s");
    bool increasing = true;
    for (int64_t i = 0; i < n; ++i) {
        if (host_tags[i] > CODD_KNN_WHERE_TAG_STR) return fail(CODD_KNN_EINVAL, "set_column: a tag is none of absent, bool, number, str%s");
        if (!host_slots) continue;
        if (host_slots[i] < 0 || host_slots[i] >= ix->count) return fail(CODD_KNN_EINVAL, "set_column: row slot outside [0, count)%s");
        if (slot_dead(ix, host_slots[i])) return fail(CODD_KNN_EINVAL, "set_column: deleted row slot (it stays dead until codd_knn_compact)%s");
        if (i > 0 && host_slots[i] <= host_slots[i - 1]) increasing = false;
    }
    // a slot listed more than once keeps its LAST value (the device writes in no order): the triples are made distinct here
    std::vector<int64_t> slots;
    std::vector<uint8_t> tags;
    std::vector<uint64_t> cells;
    if (host_slots && !increasing) {
        try {
            std::vector<int64_t> order((size_t)n);
            for (int64_t i = 0; i < n; ++i) order[(size_t)i] = i;
            std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return host_slots[a] < host_slots[b]; });
            for (int64_t i = 0; i < n; ++i) {
                const int64_t at = order[(size_t)i];
                if (i + 1 < n && host_slots[at] == host_slots[order[(size_t)i + 1]]) continue;
                slots.push_back(host_slots[at]);
                tags.push_back(host_tags[at]);
                cells.push_back(host_cells[at]);
            }
        } catch (const std::bad_alloc&) {
            return fail(CODD_KNN_ENOMEM, "host allocation failed%s");
        }
        host_slots = slots.data(); host_tags = tags.data(); host_cells = cells.data();
        n = (int64_t)slots.size();
    }
    DeviceGuard guard(ix->device);
    HIP_TRY(hipDeviceSynchronize());
    codd_knn_index::WhereColumn& col = ix->columns[column];
    if (!col.tags) {   // as long as the row store, absent everywhere; on failure the column stays unset
        DevBuf<uint8_t> fresh_tags;
        DevBuf<uint64_t> fresh_cells;
        HIP_TRY(fresh_tags.reset(ix->capacity));
        HIP_TRY(fresh_cells.reset(ix->capacity));
        HIP_TRY(hipMemset(fresh_tags, 0, (size_t)ix->capacity));
        HIP_TRY(hipMemset(fresh_cells, 0, (size_t)ix->capacity * sizeof(uint64_t)));
        col.tags = std::move(fresh_tags);
        col.cells = std::move(fresh_cells);
    }
    if (n == 0) return CODD_KNN_OK;
    if (!host_slots) {
        HIP_TRY(hipMemcpy(col.tags, host_tags, (size_t)n, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(col.cells, host_cells, (size_t)n * sizeof(uint64_t), hipMemcpyHostToDevice));
        return CODD_KNN_OK;
    }
    DevBuf<int64_t> dev_slots;
    DevBuf<uint8_t> dev_tags;
    DevBuf<uint64_t> dev_cells;
    HIP_TRY(dev_slots.reset(n));
    HIP_TRY(dev_tags.reset(n));
    HIP_TRY(dev_cells.reset(n));
    HIP_TRY(hipMemcpy(dev_slots, host_slots, (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dev_tags, host_tags, (size_t)n, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dev_cells, host_cells, (size_t)n * sizeof(uint64_t), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(column_set_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, nullptr, dev_slots, dev_tags, dev_cells, n, col.tags, col.cells);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());  // (the staging buffers go out of scope, and the call is synchronous by contract)
    return CODD_KNN_OK;
}

int codd_knn_drop_columns(codd_knn_index* ix) {
    if (!ix) return fail(CODD_KNN_EINVAL, "null index%s");
    DeviceGuard guard(ix->device);
    HIP_TRY(hipDeviceSynchronize());
    for (auto& col : ix->columns) {
        (void)col.tags.reset();
        (void)col.cells.reset();
    }
    return CODD_KNN_OK;
}

int codd_knn_eval_where(codd_knn_index* ix, const codd_knn_where_program* prog, uint32_t* dev_out_bits, int64_t nwords, void* stream) {
    if (!ix) return fail(CODD_KNN_EINVAL, "eval_where: null index%s");
    // the program is checked here, index by index, before anything is enqueued: on the device nothing leads outside it
    if (const char* why = where_program_error(prog)) return fail(CODD_KNN_EINVAL, why);
    DeviceGuard guard(ix->device);
    hipStream_t st = (hipStream_t)stream;
    std::lock_guard<std::mutex> lock(ix->mu);   // (no workspace: the kernel reads the columns and writes the caller's words)
    WhereArgs args;
    memset(&args, 0, sizeof(args));
    args.prog = *prog;
    for (int i = 0; i < prog->nleaves; ++i) {
        const int c = prog->leaves[i].column;
        if (!ix->columns[c].tags || ix->columns[c].tags.cap() < ix->count) return fail(CODD_KNN_EINVAL, "eval_where: a leaf names a column that has not been set%s");
        args.tags[c] = ix->columns[c].tags;
        args.cells[c] = ix->columns[c].cells;
    }
    const int64_t n = ix->count;
    if (nwords != (n + 31) / 32) return fail(CODD_KNN_EINVAL, "eval_where: nwords must be ceil(count / 32)%s");
    if (nwords == 0) return CODD_KNN_OK;
    if (!dev_out_bits) return fail(CODD_KNN_EINVAL, "eval_where: null bits%s");
    int rc;
    if ((rc = wait_rows(ix, st)) != 0) return rc;
    const int64_t steps = (n + kWhereBlockRows - 1) / kWhereBlockRows;
    const int64_t most = ix->where_max_blocks > 0 ? ix->where_max_blocks : (int64_t)ix->num_cus * 8;   // (grid-stride beyond that)
    rc = launch_kernel<where_eval_kernel>(dim3((unsigned)(steps < most ? steps : most)), dim3(kWhereThreads), 0, st, args, ix->dead_bits, n, nwords, dev_out_bits);
    if (rc != 0) return rc;
    HIP_TRY(hipGetLastError());
    ix->stat_where_evals++;
    return CODD_KNN_OK;
}

#ifdef CODD_I8_EXP_STAMPS
// diagnostic builds only (not in include/codd_knn.h): the per-wave phase stamps of the last i8_tile_kernel<FILTER> launch on `stream`'s
// workspace — [workgroup][wave][8] u64: issue, corpus wait, MFMA phase, end-of-interval sync, epilogue, intervals, total, tiles
int codd_knn_exp_read_stamps(codd_knn_index* ix, unsigned long long* host_out, int n_u64, void* stream) {
    if (!ix || !host_out) return CODD_KNN_EINVAL;
    WorkScope work(ix, (hipStream_t)stream);
    if (!ix->bucket_max || (int64_t)n_u64 > ix->bucket_max.cap()) return CODD_KNN_EINVAL;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(host_out, ix->bucket_max, (size_t)n_u64 * 8, hipMemcpyDeviceToHost));
    return CODD_KNN_OK;
}
#endif

int codd_knn_debug_last_pass(codd_knn_index* ix, void* stream, codd_knn_last_pass* info, float* thr, float* qmeta, uint32_t* hit_counts,
                             uint32_t* fb_list, uint64_t* keys, int64_t keys_per_query, uint64_t* bucket_max, int64_t bucket_max_cap,
                             float* bmeta, int64_t bmeta_blocks) {
    if (keys_per_query < 0 || bucket_max_cap < 0 || bmeta_blocks < 0) return fail(CODD_KNN_EINVAL, "negative buffer size%s");
    if (!ix) return fail(CODD_KNN_EINVAL, "null index%s");
    hipStream_t st = (hipStream_t)stream;
    std::lock_guard<std::mutex> lock(ix->mu);
    // the stream's workspace where it rests between calls (no WorkScope: a stream that never searched must not take a slot)
    const WorkBufs* w = nullptr;
    for (const WorkSlot& s : ix->slots)
        if (s.used && s.stream == st) w = &s.bufs;
    if (!w || !w->last.valid) return fail(CODD_KNN_EINVAL, "no filter pass has run on this stream's workspace%s");
    const LastPass& lp = w->last;
    if (bucket_max && bucket_max_cap < (int64_t)kTileQ * lp.sample_tiles) return fail(CODD_KNN_EINVAL, "bucket_max buffer below 256 x sampled tiles%s");
    DeviceGuard guard(ix->device);
    HIP_TRY(hipStreamSynchronize(st));
    FilterCtl ctl;
    HIP_TRY(hipMemcpy(&ctl, w->ctl.get(), sizeof(FilterCtl), hipMemcpyDeviceToHost));
    if (info) {
        info->family = lp.family; info->nbq = lp.nbq; info->ts = lp.ts; info->res = lp.res; info->el = lp.el; info->sqd = lp.sqd;
        info->nq = lp.nq; info->k = lp.k; info->hit_cap = lp.hit_cap;
        info->per_block_filter = lp.per_block_filter; info->per_block_finalize = lp.per_block_finalize;
        info->eps = lp.eps;
        info->n = lp.n; info->sample_tiles = lp.sample_tiles; info->sample_stride = lp.sample_stride;
        info->cascade_d = (uint32_t)lp.cascade_d;
        for (int i = 0; i < 4; ++i) info->flags[i] = i < FLAG_WORDS ? ctl.flags[i] : 0u;
        info->fb_count = ctl.fb_count;
    }
    if (thr) HIP_TRY(hipMemcpy(thr, w->thr.get(), 2 * kTileQ * sizeof(float), hipMemcpyDeviceToHost));
    if (qmeta && lp.el && w->qmeta) HIP_TRY(hipMemcpy(qmeta, w->qmeta.get(), 1024 * sizeof(float), hipMemcpyDeviceToHost));
    if (hit_counts)
        for (int q = 0; q < kTileQ; ++q) hit_counts[q] = ctl.hit_cnt[q * kHitCntStride];
    if (fb_list) memcpy(fb_list, ctl.fb_list, sizeof(ctl.fb_list));
    if (keys && keys_per_query > 0) {
        for (int q = 0; q < kTileQ; ++q) {
            int64_t m = ctl.hit_cnt[q * kHitCntStride];
            if (m > lp.hit_cap) m = lp.hit_cap;
            if (m > keys_per_query) m = keys_per_query;
            if (m > 0) HIP_TRY(hipMemcpy(keys + (int64_t)q * keys_per_query, w->hits.get() + (int64_t)q * lp.hit_cap, (size_t)m * sizeof(u64), hipMemcpyDeviceToHost));
        }
    }
    if (bucket_max) HIP_TRY(hipMemcpy(bucket_max, w->bucket_max.get(), (size_t)kTileQ * lp.sample_tiles * sizeof(u64), hipMemcpyDeviceToHost));
    if (bmeta && lp.el && ix->bmeta) {
        int64_t nb = (lp.n + 31) / 32;
        if (nb > bmeta_blocks) nb = bmeta_blocks;
        if (nb > 0) HIP_TRY(hipMemcpy(bmeta, ix->bmeta.get(), (size_t)nb * sizeof(float2), hipMemcpyDeviceToHost));
    }
    return CODD_KNN_OK;
}

int codd_knn_set_option(codd_knn_index* ix, const char* key, int64_t value) {
    if (!ix || !key) return fail(CODD_KNN_EINVAL, "bad option arguments%s");
    // an integer in [lo, hi] stored into one knob: kKnobTable (search_plan.h)
    if (const KnobRow* row = find_knob(key)) {
        if (const char* message = set_knob(ix->knobs, *row, value)) return fail(CODD_KNN_EINVAL, message);
        if (row->knob == &FilterKnobs::shadow8_cooldown) ix->watch.cooldown_left = 0;
        return CODD_KNN_OK;
    }
    // ... and the options that clamp, are no plain int or do more than store
    if (strcmp(key, "filter") == 0) { ix->knobs.filter_enabled = value != 0; return CODD_KNN_OK; }
    if (strcmp(key, "filter_min_rows") == 0) { ix->knobs.filter_min_rows = value < 1 ? 1 : value; return CODD_KNN_OK; }
    if (strcmp(key, "filter_min_rows_small") == 0) { ix->knobs.filter_min_rows_small = value < 1 ? 1 : value; return CODD_KNN_OK; }
    if (strcmp(key, "filter_min_batch") == 0) { ix->knobs.filter_min_batch = value < 1 ? 1 : (int)value; return CODD_KNN_OK; }
    // an IVF layout that follows writes (plain integers in a range, checked here like the cascade's: kKnobTable's length is pinned)
    if (strcmp(key, "ivf_follow") == 0) {
        if (value < 0 || value > 1) return fail(CODD_KNN_EINVAL, "ivf_follow must be 0 or 1%s");
        ix->ivf_follow = (int)value;
        return CODD_KNN_OK;
    }
    if (strcmp(key, "ivf_fold_rows") == 0) {
        if (value < 0 || value > (1ll << 32)) return fail(CODD_KNN_EINVAL, "ivf_fold_rows must be in [0,2^32]%s");
        ix->ivf_fold_rows = value;
        return CODD_KNN_OK;
    }
    // the sample cascade (search_plan.h: cascade_plan)
    if (strcmp(key, "sample_cascade") == 0) {
        if (value < 0 || value > 2) return fail(CODD_KNN_EINVAL, "sample_cascade must be 0, 1 or 2%s");
        ix->knobs.sample_cascade = (int)value;
        return CODD_KNN_OK;
    }
    if (strcmp(key, "cascade_d") == 0) {
        if (value < kCascadeDMin || value > kCascadeDMax) return fail(CODD_KNN_EINVAL, "cascade_d must be in [16,64]%s");
        ix->knobs.cascade_d = (int)value;
        return CODD_KNN_OK;
    }
    if (strcmp(key, "i8_sweep") == 0) {  // the sweep form of the static int8 tile program (search_plan.h: filter_program)
        if (value < 0 || value > 1) return fail(CODD_KNN_EINVAL, "i8_sweep must be 0 or 1%s");
        ix->knobs.i8_sweep = (int)value;
        return CODD_KNN_OK;
    }
    if (strcmp(key, "cascade_min_rounds") == 0) {
        if (value < 1 || value > 64) return fail(CODD_KNN_EINVAL, "cascade_min_rounds must be in [1,64]%s");
        ix->knobs.cascade_min_rounds = (int)value;
        return CODD_KNN_OK;
    }
#if CODD_EXPERIMENTS
    if (strcmp(key, "exp_slack_pct") == 0) {  // what-if timing only, experiment builds only: < 100 makes the int8 filter UNSOUND
        if (value < 1 || value > 100) return fail(CODD_KNN_EINVAL, "exp_slack_pct must be in [1,100]%s");
        ix->exp_slack_scale = (float)value / 100.0f;
        return CODD_KNN_OK;
    }
#endif
    if (strcmp(key, "debug_fail_shadow_alloc") == 0) {  // test hook: the 2-byte shadow's allocation fails as if HBM were full
        ix->debug_fail_shadow_alloc = value != 0;
        if (!value) ix->shadow_nomem_epoch = -1;
        return CODD_KNN_OK;
    }
    if (strcmp(key, "debug_num_cus") == 0) {  // test hook: the filter passes count this many compute units (0: the device's)
        if (value < 0 || value > ix->num_cus) return fail(CODD_KNN_EINVAL, "debug_num_cus must be 0 or in [1, the device's compute units]%s");
        ix->debug_num_cus = (int)value;
        return CODD_KNN_OK;
    }
    if (strcmp(key, "all_normalized") == 0) {
        // 0: the caller knows of rows that are not unit vectors (a persisted index written with normalize = 0): both filters
        // off, every search takes the exact scan.  The flag cannot be switched back on from outside.
        if (value != 0) return fail(CODD_KNN_EINVAL, "all_normalized can only be cleared (0)%s");
        ix->all_normalized = false;
        return CODD_KNN_OK;
    }
    if (strcmp(key, "where_max_blocks") == 0) {
        if (value < 0 || value > (1ll << 20)) return fail(CODD_KNN_EINVAL, "where_max_blocks must be in [0,2^20]%s");
        ix->where_max_blocks = value;
        return CODD_KNN_OK;
    }
    if (strcmp(key, "compact_chunk_rows") == 0) {
        if (value < 0 || value > (1ll << 32)) return fail(CODD_KNN_EINVAL, "compact_chunk_rows must be in [0,2^32]%s");
        ix->compact_chunk_rows = value;
        return CODD_KNN_OK;
    }
    if (strcmp(key, "profile") == 0) {
        // value = number of (start, stop) event pairs to keep (0 switches timing off); resets the log
        if (value < 0 || value > 65536) return fail(CODD_KNN_EINVAL, "profile pairs must be in [0,65536]%s");
        DeviceGuard guard(ix->device);
        while ((int64_t)ix->ev.size() < 2 * value) {
            Event e;
            HIP_TRY(e.ensure(hipEventDefault));
            ix->ev.push_back(std::move(e));
        }
        ix->ev_kind.assign(ix->ev.size() / 2, 0);
        ix->profile = value > 0;
        ix->ev_used = 0;
        return CODD_KNN_OK;
    }
    return fail(CODD_KNN_EINVAL, "unknown option: %s", key);
}

int codd_knn_debug_live_allocations(int64_t* buffers, int64_t* bytes, int64_t* events) {
    if (!buffers || !bytes || !events) return fail(CODD_KNN_EINVAL, "debug_live_allocations: null output%s");
    *buffers = g_live_buffers.load();
    *bytes = g_live_bytes.load();
    *events = g_live_events.load();
    return CODD_KNN_OK;
}

int codd_knn_get_stat(const codd_knn_index* ix, const char* key, int64_t* out) {
    if (!ix || !key || !out) return fail(CODD_KNN_EINVAL, "bad stat arguments%s");
    // "time_ns:<kernel>" / "events:<kernel>" with kernel in {scan, filter, sample, finalize}
    const bool want_time = strncmp(key, "time_ns:", 8) == 0, want_events = strncmp(key, "events:", 7) == 0;
    if (want_time || want_events) {
        const char* name = key + (want_time ? 8 : 7);
        int kind = -1;
        for (int i = 0; i < EV_KINDS; ++i)
            if (strcmp(name, kEvNames[i]) == 0) kind = i;
        if (kind < 0) return fail(CODD_KNN_EINVAL, "unknown kernel name in stat: %s", key);
        double total_ms = 0.0;
        int64_t events = 0;
        if (ix->ev_used > 0) {
            DeviceGuard guard(ix->device);
            HIP_TRY(hipEventSynchronize(ix->ev[2 * ix->ev_used - 1]));
            for (int i = 0; i < ix->ev_used; ++i) {
                if (ix->ev_kind[i] != kind) continue;
                float ms = 0.0f;
                HIP_TRY(hipEventElapsedTime(&ms, ix->ev[2 * i], ix->ev[2 * i + 1]));
                total_ms += ms;
                events++;
            }
        }
        *out = want_time ? (int64_t)(total_ms * 1e6) : events;
        return CODD_KNN_OK;
    }
    // the stats that read one int64 member
    static const struct { const char* name; int64_t codd_knn_index::*member; } kStatTable[] = {
        {"searches", &codd_knn_index::stat_searches},
        {"scan_launches", &codd_knn_index::stat_scan_launches},
        {"last_scan_blocks", &codd_knn_index::stat_last_scan_blocks},
        {"last_scan_group", &codd_knn_index::stat_last_scan_group},
        {"last_finalize_parts", &codd_knn_index::stat_last_finalize_parts},
        {"ivf_shared_searches", &codd_knn_index::stat_ivf_shared},
        {"ivf_masked_searches", &codd_knn_index::stat_ivf_masked},
        {"ivf_refreshes", &codd_knn_index::stat_ivf_refreshes},
        {"ivf_delta_searches", &codd_knn_index::stat_ivf_delta},
        {"ivf_fold_rows", &codd_knn_index::ivf_fold_rows},
        {"ivf_rows", &codd_knn_index::ivf_count},
        {"scoped_searches", &codd_knn_index::stat_scoped_searches},
        {"scope_builds", &codd_knn_index::stat_scope_builds},
        {"masked_searches", &codd_knn_index::stat_masked_searches},
        {"mask_list_searches", &codd_knn_index::stat_mask_list},
        {"mask_dense_searches", &codd_knn_index::stat_mask_dense},
        {"last_mask_rows", &codd_knn_index::stat_last_mask_rows},
        {"masked_dev_searches", &codd_knn_index::stat_masked_dev},
        {"doc_matches", &codd_knn_index::stat_doc_matches},
        {"doc_regex_matches", &codd_knn_index::stat_doc_regex_matches},
        {"where_evals", &codd_knn_index::stat_where_evals},
        {"dead_rows", &codd_knn_index::dead_count},
        {"delete_calls", &codd_knn_index::stat_delete_calls},
        {"compactions", &codd_knn_index::stat_compactions},
        {"filter_passes", &codd_knn_index::stat_filter_passes},
        {"cascade_passes", &codd_knn_index::stat_cascade_passes},
        {"last_cascade_d", &codd_knn_index::stat_last_cascade_d},
        {"sweep_passes", &codd_knn_index::stat_sweep_passes},
        {"last_sweep", &codd_knn_index::stat_last_sweep},
        {"shadow8_builds", &codd_knn_index::stat_shadow8_builds},
        {"shadow16_builds", &codd_knn_index::stat_shadow_builds},
        {"shadow16_alloc_failures", &codd_knn_index::stat_shadow_nomem},
        {"shadow8_passes", &codd_knn_index::stat_shadow8_passes},
        {"i8v2_passes", &codd_knn_index::stat_i8v2_passes},
        {"f16_tile_passes", &codd_knn_index::stat_f16_tile_passes},
        {"small_batch_passes", &codd_knn_index::stat_small_batch},
        {"capacity_rows", &codd_knn_index::capacity},
    };
    for (const auto& row : kStatTable)
        if (strcmp(key, row.name) == 0) {
            *out = ix->*row.member;
            return CODD_KNN_OK;
        }
    if (strcmp(key, "scopes") == 0) *out = (int64_t)ix->max_scope;
    else if (strcmp(key, "docs_valid") == 0) *out = docs_valid(ix) ? 1 : 0;
    else if (strcmp(key, "doc_bytes") == 0) *out = ix->doc_arena ? ix->doc_bytes : 0;
    else if (strcmp(key, "doc_tile_bytes") == 0) *out = kDocTile;
    else if (strcmp(key, "doc_regex_tile_bytes") == 0) *out = kRegexTile;
    else if (strcmp(key, "doc_regex_run_docs") == 0) *out = kRegexDocs;
    else if (strcmp(key, "where_columns") == 0) {
        *out = 0;
        for (const auto& col : ix->columns) *out += col.tags ? 1 : 0;
    }
    else if (strcmp(key, "where_column_bytes") == 0) {
        *out = 0;
        for (const auto& col : ix->columns) *out += col.tags.bytes() + col.cells.bytes();
    }
    else if (strcmp(key, "all_normalized") == 0) *out = ix->all_normalized ? 1 : 0;
    else if (strcmp(key, "metric") == 0) *out = ix->metric;
    else if (strcmp(key, "space_filter") == 0) *out = ix->knobs.space_filter;
    else if (strcmp(key, "space_ivf") == 0) *out = ix->knobs.space_ivf;
    else if (strcmp(key, "ivf_follow") == 0) *out = ix->ivf_follow;
    else if (strcmp(key, "ivf_pending_rows") == 0) *out = ix->pend.count;
    else if (strcmp(key, "ivf_fold_threshold") == 0) *out = ix->coarse ? fold_threshold(ix->ivf_fold_rows, ix->ivf_count, ix->ivf_nlist) : 0;
    else if (strcmp(key, "shadow8_cooldowns") == 0) *out = ix->watch.stat_cooldowns;
    else if (strcmp(key, "shadow8_wide_blocks") == 0) {  // blocks whose error norm exceeds shadow8_max_eps, as last read back
        if (ix->eps_r_copied && hipEventQuery(ix->eps_r_copied) == hipSuccess) *out = (int64_t)reinterpret_cast<const unsigned*>(ix->eps_r_host.get())[1];
        else {
            (void)hipGetLastError();
            *out = ix->wide_blocks_known;
        }
    }
    else if (strcmp(key, "shadow8_eps_r_micro") == 0) {  // worst row's quantisation error norm x 1e6, as last read back
        if (ix->eps_r_copied && hipEventQuery(ix->eps_r_copied) == hipSuccess) *out = (int64_t)(ix->eps_r_host[0] * 1e6f);
        else {
            (void)hipGetLastError();
            *out = (int64_t)(ix->eps_r_known * 1e6f);
        }
    }
    else if (strcmp(key, "fallback_queries") == 0 || strcmp(key, "filter_hits") == 0 || strcmp(key, "filter_survivors") == 0) {
        // device-side counters (the search itself never reads them back): synchronises
        unsigned long long h[4] = {0, 0, 0, 0};
        if (ix->dstats) {
            DeviceGuard guard(ix->device);
            HIP_TRY(hipDeviceSynchronize());
            HIP_TRY(hipMemcpy(h, ix->dstats, sizeof(h), hipMemcpyDeviceToHost));
        }
        *out = (int64_t)(key[0] == 'f' && key[1] == 'a' ? h[2] : (strcmp(key, "filter_hits") == 0 ? h[0] : h[1]));
    }
    else if (strcmp(key, "mask_filter_hits") == 0 || strcmp(key, "mask_filter_survivors") == 0 || strcmp(key, "mask_fallback_queries") == 0) {
        // the same device counters, of the dense masked passes alone: synchronises
        unsigned long long h[4] = {0, 0, 0, 0};
        if (ix->mask_dstats) {
            DeviceGuard guard(ix->device);
            HIP_TRY(hipDeviceSynchronize());
            HIP_TRY(hipMemcpy(h, ix->mask_dstats, sizeof(h), hipMemcpyDeviceToHost));
        }
        *out = (int64_t)(key[12] == 'h' ? h[0] : (key[12] == 's' ? h[1] : h[2]));
    }
    else if (strcmp(key, "num_cus") == 0) *out = ix->num_cus;
    else if (strcmp(key, "device_bytes") == 0) {
        int64_t b = ix->capacity * (int64_t)ix->dpad * (int64_t)elem_size(ix->dtype) + ix->shadow_rows * (int64_t)ix->dpad * 2 +
                    ix->shadow8_rows * ((int64_t)dpad8_of(shape_of(ix)) + 4) + ix->scope_of.bytes() + ix->scope_perm.bytes() + ix->scope_offsets.bytes() + ix->dead_bits.bytes() +
                    ix->doc_arena.bytes() + ix->doc_offsets.bytes();
        for (const WorkSlot& w : ix->slots)
            b += w.bufs.qn.bytes() + w.bufs.partial.bytes() + w.bufs.keys_tmp.bytes() + w.bufs.hits.bytes() + w.bufs.bucket_max.bytes() +
                 w.bufs.qfrag.bytes() + w.bufs.fb_partial.bytes() + w.bufs.probe_keys.bytes() + w.bufs.ivf_partial.bytes();
        *out = b;  // (the terms it has always had: DESIGN.md §18 lists what it leaves out)
    } else if (strcmp(key, "workspaces") == 0) {
        int64_t c = 0;
        for (const WorkSlot& w : ix->slots) c += w.used ? 1 : 0;
        *out = c;
    }
    else return fail(CODD_KNN_EINVAL, "unknown stat: %s", key);
    return CODD_KNN_OK;
}

}  // extern "C"
