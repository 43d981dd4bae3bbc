/*
 * codd_knn.h — C ABI of the MI355X-native cosine top-k engine that stands where
 * ChromaDB stands on Codd's `search_relevant_metrics` path.
 *
 * The reference has no FFI of its own: its seam is Python duck typing on the
 * chromadb client object injected into MetricsSemanticMetadataStore
 * (/root/reference/codd_dal/metrics/metrics_semantic_metadata_store.py:43-57).
 * Each entry point below names the chromadb call it takes over; string ids
 * and metadata never cross this boundary, documents only as the bytes that
 * codd_knn_match_documents searches (the Python façade
 * codd_query_engine_amd/knn_client.py keeps id <-> row slot and metadata on the
 * host, exactly the part of chromadb that is not arithmetic).
 *
 * Conventions
 *   - every function returns 0 on success and a negative CODD_KNN_E* code on
 *     failure; it never throws, aborts or exits.  codd_knn_last_error() returns a
 *     thread-local message for the last failure on the calling thread.
 *   - "dev_" pointers are device (HBM) addresses on the index's GPU, "host_"
 *     pointers are ordinary host memory.  The caller owns every buffer it passes;
 *     the index owns its row storage and its workspaces.
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream).  Calls
 *     are asynchronous with respect to the host unless stated otherwise.
 *   - thread-safety: the search entry points (codd_knn_search, _search_keys, _search_scoped,
 *     _search_masked, _search_masked_dev, _match_documents, _match_documents_dfa, _eval_where, _ivf_search, _ivf_search_masked, _ivf_search_masked_dev, _approx_scores) may be called from several host threads and on
 *     several streams of one index: the index keeps one workspace per stream (up to
 *     4; a fifth stream takes over the least recently used one, ordered behind its
 *     previous owner on the device) and serialises only the enqueueing.  Searches on
 *     different streams then overlap on the GPU.  upsert/reserve/load/ivf_install/set_scopes/
 *     delete/compact/set_documents/set_column/drop_columns are exclusive: no other call on the index may be in flight.
 *   - rows are stored L2-normalised, zero padded to a multiple of 64 elements.  Normalisation
 *     (rows and queries alike) holds for every finite non-zero fp32 vector, whatever its scale:
 *     where the fp32 sum of squares leaves [2^-100, 2^100] the vector is first scaled by an exact
 *     power of two.  A vector with a NaN or infinite element, or all zeros, is the
 *     zero vector: score 0, distance 1 against everything.
 *     score = <q/|q|, c/|c|> evaluated in fp32 in the canonical order of
 *     DESIGN.md §3; distance = 1 - score (fp32); ties -> lower row.
 *   - the above is the cosine metric.  An index created with CODD_KNN_METRIC_IP or CODD_KNN_METRIC_L2
 *     (ChromaDB's `hnsw:space` "ip" and "l2") uses rows and queries AS GIVEN: rounded to
 *     the storage dtype and zero padded, never normalised (upsert with normalize = 0; normalize != 0
 *     still normalises, the caller's choice).  A vector with a NaN or infinite element, or without a
 *     non-zero one, is the zero vector here too.
 *       ip: score = <q, c>, the canonical dot product of DESIGN.md §3; distance = 1 - score.
 *       l2: distance = sum (q_i - c_i)^2, the SQUARED distance as hnswlib and ChromaDB report it, by the
 *           direct difference in the same canonical order (per element one fp32 subtraction t, then
 *           fmaf(t, t, a)); the score packed into a key is 0 - distance.  A query equal to a stored row
 *           has distance +0.0 exactly.
 *     Ties -> lower row, padding (row -1, distance +inf, key 0) and "a NaN score ranks as -inf" are as
 *     for cosine.  Inputs whose fp32 sums overflow are outside the contract.  Such an index takes no
 *     MFMA filter leg (both assume unit rows): every batch is answered by the exact scan, in groups of
 *     up to 8 queries per pass over the rows; the "all_normalized" stat reads 0 from the start.  (Opt-in,
 *     option "space_filter": an int8 filter leg with measured norms in its bound; the
 *     answers are the same bits.)  Every
 *     search, delete, compact, load and read entry point keeps its contract word for word under these
 *     metrics, except the IVF ones and codd_knn_approx_scores, which return ENOTSUP by default (spherical
 *     k-means and the bf16 assignment are cosine-specific).  (Opt-in, option "space_ivf": the IVF entry
 *     points accept an ip or l2 index, with a coarse index in the index's own space)
 *   - the count is the highest written slot + 1, and a write may start above it.  A row slot below the count that was never
 *     written (since creation, or since the last codd_knn_compact vacated it) holds the zero vector: it is live, has scope 0,
 *     scores 0 (distance 1) under cosine and ip and lies at distance sum q_i^2 under l2 on every search path, reads back as
 *     zeros from codd_knn_read_rows, and can be deleted.
 *   - every entry point with a `row_base` (codd_knn_search_keys, _search_scoped, _search_masked,
 *     _search_masked_dev, _ivf_search, _ivf_search_masked, _ivf_search_masked_dev) writes global rows
 *     row_base + row, which must fit the low word of a packed key: the highest global row is
 *     0xFFFFFFFD, i.e. row_base + count < 0xFFFFFFFF, else EINVAL and nothing is enqueued or written.
 *   - a row slot can be deleted (codd_knn_delete_host): it becomes a tombstone that no search entry
 *     point returns and no write accepts, until codd_knn_compact moves the live rows down over it
 *     (stable: slot order kept).  An index nobody deleted from behaves, and runs, exactly as before
 *     (DESIGN.md §14).
 */
#ifndef CODD_KNN_H
#define CODD_KNN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CODD_KNN_DTYPE_F32 0
#define CODD_KNN_DTYPE_BF16 1
#define CODD_KNN_DTYPE_F16 2

/* `hnsw:space` of get_or_create_collection (store.py:63-68): "cosine", "ip", "l2" (see the conventions above) */
#define CODD_KNN_METRIC_COSINE 0
#define CODD_KNN_METRIC_IP 1
#define CODD_KNN_METRIC_L2 2

#define CODD_KNN_MAX_K 128        /* reference caps n_results at 100 (store.py:24) */
#define CODD_KNN_MAX_BATCH 1024   /* queries per codd_knn_search call */
#define CODD_KNN_MAX_SCOPE 1048575u /* highest scope label of codd_knn_set_scopes_host */

#define CODD_KNN_OK 0
#define CODD_KNN_EINVAL (-22)     /* bad argument */
#define CODD_KNN_ENOMEM (-12)     /* device allocation failed */
#define CODD_KNN_EDEVICE (-5)     /* HIP runtime error */
#define CODD_KNN_ENOTSUP (-95)    /* shape/dtype outside what the kernels cover */

typedef struct codd_knn_index codd_knn_index;

/* library / build identification: "codd_knn <semver> gfx950 shadow=<bf16|f16> mfma=<shape>" */
const char* codd_knn_version(void);
const char* codd_knn_last_error(void);

/*
 * Replaces: client.get_or_create_collection(name=..., metadata={"hnsw:space":"cosine",...})
 *           (store.py:60-69) — the arithmetic half: an empty device-resident row store.
 * dim: embedding width, 1 <= dim <= 4096 for every dtype (4097 and above: EINVAL).  Rows of up to
 *      1024 (f32) / 2048 (bf16, f16) elements are scored with the query held in registers; wider
 *      rows (1536 / 3072 / 4096-wide embedders) by the wide forms of the exact-score kernels — the
 *      scan, finalize, the threshold anchors and the IVF scans — which stage the query in LDS and
 *      walk the row in segments: the same canonical scores.
 * metric: CODD_KNN_METRIC_COSINE, _IP or _L2; any other value: ENOTSUP.
 */
int codd_knn_create(codd_knn_index** out, int device, int dim, int dtype, int metric);
int codd_knn_destroy(codd_knn_index* index);

/* Grow row storage to hold at least `rows` row slots (contents preserved). Synchronous. */
int codd_knn_reserve(codd_knn_index* index, int64_t rows);

/*
 * Replaces: collection.upsert(documents=[...], metadatas=[...], ids=[...]) (store.py:236-238)
 *           — the vector half.  Writes `n` fp32 vectors (row stride `dim`) into the row
 *           slots chosen by the host id-map; a slot may be new (append) or existing
 *           (overwrite).  normalize != 0 scales each vector to unit L2 norm first
 *           (always what the façade asks for; 0 is for callers that already did).
 *           Storage grows as needed.  The host variant stages through a bounded device
 *           buffer (kept by the index between calls) and is synchronous; the device variant
 *           writes slots [first_slot, first_slot+n) asynchronously on `stream`: it is ordered on
 *           the device behind every search and every earlier upsert already enqueued on other
 *           streams of this index (two writers on two streams run in call order), and every later
 *           search, upsert or codd_knn_copy_rows_f32 on another stream waits for it on the device
 *           (no host synchronisation either way).  The `dev_vecs` buffer must stay valid until
 *           `stream` has run the call.
 */
int codd_knn_upsert_host(codd_knn_index* index, const int64_t* host_slots, const float* host_vecs,
                         int64_t n, int normalize);
int codd_knn_upsert_device(codd_knn_index* index, int64_t first_slot, const float* dev_vecs,
                           int64_t n, int normalize, void* stream);

/*
 * Counterpart of codd_knn_read_rows for loading a persisted index (the role of the Chroma
 * server's docker volume, docker-compose.yml:8-9): `host_rows` are n stored rows exactly as
 * codd_knn_read_rows returned them (storage dtype, padded width, already normalised); they are
 * copied into slots [first_slot, first_slot+n).  Their norms are checked on the device: if any row is
 * not a unit vector (within the storage type's rounding) the index behaves as after an upsert with
 * normalize = 0 — both filters off, every search an exact scan ("all_normalized" stat = 0).  An ip or l2 index
 * holds rows of any norm: nothing is checked, the rows load bit for bit.  Synchronous.
 */
int codd_knn_load_rows(codd_knn_index* index, int64_t first_slot, const void* host_rows, int64_t n);

/* Number of row slots in use (highest written slot + 1) — collection.count(). */
int codd_knn_count(const codd_knn_index* index, int64_t* out);
int codd_knn_dim(const codd_knn_index* index, int* dim, int* padded_dim, int* dtype);

/* Copy stored rows [first, first+n) back to the host, in storage dtype, padded width.
 * (persistence + tests).  Synchronous.  Slot-addressed: a deleted slot's contents are returned as they are. */
int codd_knn_read_rows(const codd_knn_index* index, int64_t first, int64_t n, void* host_out);

/*
 * Replaces: collection.query(query_texts=[q], n_results=n) (store.py:314-316) — the k-NN
 *           half, batched.  dev_queries: B x dim fp32, raw (normalised here).
 *           dev_dist : B x k fp32, ascending distance (1 - score), +inf padded.
 *           dev_rows : B x k int64 row slots, -1 padded (fewer than k rows stored).
 */
int codd_knn_search(codd_knn_index* index, const float* dev_queries, int B, int k,
                    float* dev_dist, int64_t* dev_rows, void* stream);

/*
 * Shard-local half of a row-sharded search: same as codd_knn_search but returns packed
 * keys, key = (orderable_u32(score) << 32) | (0xFFFFFFFF - (row_base + row)), descending,
 * 0 = empty slot — so that the cross-rank merge is an integer top-k (codd_knn_merge_keys).
 */
int codd_knn_search_keys(codd_knn_index* index, const float* dev_queries, int B, int k,
                         uint32_t row_base, uint64_t* dev_keys, void* stream);

/*
 * Top-k of B lists of m packed keys each (the all-gathered [B][G*k] shard partials).
 * Any of dev_keys_out / dev_dist / dev_rows may be NULL.  `device` as in codd_knn_create.
 */
int codd_knn_merge_keys(int device, const uint64_t* dev_keys_in, int B, int m, int k,
                        uint64_t* dev_keys_out, float* dev_dist, int64_t* dev_rows, void* stream);

/*
 * The same merge straight from the buffer an all_gather of the ranks' [B][k_in] partials delivers:
 * dev_keys_in[(g * B + q) * k_in + j], g < G.  No transpose pass in between.
 */
int codd_knn_merge_shards(int device, const uint64_t* dev_keys_in, int G, int B, int k_in, int k,
                          uint64_t* dev_keys_out, float* dev_dist, int64_t* dev_rows, void* stream);

/*
 * The two merges above for keys of any metric.  The keys merge alike (integers); `metric` decides the
 * distance written to dev_dist: 1 - score for CODD_KNN_METRIC_COSINE and _IP, 0 - score for _L2
 * (another value: ENOTSUP).  codd_knn_merge_keys and codd_knn_merge_shards are these with cosine.
 */
int codd_knn_merge_keys_metric(int device, const uint64_t* dev_keys_in, int B, int m, int k, int metric,
                               uint64_t* dev_keys_out, float* dev_dist, int64_t* dev_rows, void* stream);
int codd_knn_merge_shards_metric(int device, const uint64_t* dev_keys_in, int G, int B, int k_in, int k, int metric,
                                 uint64_t* dev_keys_out, float* dev_dist, int64_t* dev_rows, void* stream);

/*
 * The raw approximate (bf16 MFMA) scores of B <= 256 queries against every stored row:
 * dev_scores[q * count + row], q < 256 (rows of padding queries are zero).  Used by the IVF build
 * (row -> nearest centroid) and by tests that check the MFMA operand layouts in isolation.
 * Cosine indexes only: ENOTSUP on an ip or l2 index, nothing enqueued — unless that index has its int8 filter
 * leg switched on (option "space_filter" = 1) and B <= 32: then dev_scores holds the values that
 * leg filters with, the int8 approximation of <q, c> (ip) or of -|q - c|^2 (l2: fma(acc s_row, 2 s_q, -|c|^2) - |q|^2),
 * each within codd_knn_filter_slack's eps(q) of the exact score of (q, row).
 */
int codd_knn_approx_scores(codd_knn_index* index, const float* dev_queries, int B,
                                 float* dev_scores, void* stream);

/*
 * Debug: dev_slack[q] = eps(q), q < B <= 256: the slack between an approximate and an exact score that the next int8
 * filter pass over this index would use for these queries (the device-wide bound: measured |q - q~|, the rows'
 * measured quantisation error and, on an ip or l2 index, the measured norms).  +inf: the bound
 * cannot be evaluated finitely and the pass re-scores every row.  Builds the int8 shadow if rows changed.
 * ENOTSUP where the index has no int8 leg: "shadow8" off, or an ip / l2 index without "space_filter".
 */
int codd_knn_filter_slack(codd_knn_index* index, const float* dev_queries, int B, float* dev_slack, void* stream);

/*
 * Coarse-IVF with exact scores (BASELINE config 5: the small-batch, HBM-bound regime on corpora
 * where even one pass over the shard is too slow).  Not on the reference's path — ChromaDB's own
 * index is HNSW (store.py:63-68) — but the same trade: approximate candidate generation, exact
 * distances.  The caller clusters the rows (codd_query_engine_amd/ivf.py: spherical k-means whose
 * assignment GEMM is codd_knn_approx_scores on a centroid index) and hands over
 *   dev_centroids [nlist][dim] fp32, dev_perm [count] (row slots grouped by list),
 *   dev_offsets [nlist+1] (list l = perm[offsets[l] .. offsets[l+1])).
 * install copies the rows into list order (HBM: one more copy of the rows) and builds the coarse
 * index; any later upsert makes the layout stale (ivf_search then fails with EINVAL) — except on an
 * index whose option "ivf_follow" is 1, see codd_knn_ivf_refresh below.
 * ivf_search: nprobe (<= 128) best lists per query by exact centroid score, canonical exact scores
 * over those lists, top-k with ORIGINAL row slots; with nprobe == nlist the result is bit-identical
 * to codd_knn_search.  Any of dev_keys / dev_dist / dev_rows may be NULL.
 * An ip or l2 index: ENOTSUP from install and from every IVF search, nothing enqueued or allocated, unless
 * option "space_ivf" is 1.  Then the centroids are RAW vectors (stored as given, f32, not
 * normalised: for l2 the means of their lists), the coarse index has the index's own metric, and ivf_search
 * probes the nprobe lists of smallest canonical squared distance to the centroid (l2) or largest canonical
 * dot product with it (ip), ties to the lower list number; the lists are scored with the index's canonical
 * expression on the raw query.  The contract is the cosine one word for word: the exact canonical top-k among
 * the allowed live rows of the probed lists, min(k, rows there) hits, padding (row -1, distance +inf, key 0),
 * and nprobe >= nlist is codd_knn_search bit for bit.  The same holds for the two masked forms below.
 */
/* Stored rows [first, first+n) widened to fp32, device to device, asynchronously on `stream` (the IVF build's
 * input).  Ordered like a search: behind every upsert enqueued before it on any stream, and a later upsert waits
 * for it — which is why the index is not const here (ABI change in round 3). */
int codd_knn_copy_rows_f32(codd_knn_index* index, int64_t first, int64_t n, float* dev_out, void* stream);
int codd_knn_ivf_install(codd_knn_index* index, const float* dev_centroids, int nlist,
                         const int64_t* dev_perm, const int64_t* dev_offsets, void* stream);
int codd_knn_ivf_search(codd_knn_index* index, const float* dev_queries, int B, int k, int nprobe,
                        uint32_t row_base, uint64_t* dev_keys, float* dev_dist, int64_t* dev_rows,
                        void* stream);

/*
 * An IVF layout that follows writes (opt-in, option "ivf_follow" = 1, default 0: nothing changes).
 * With the option on, an installed layout stays searchable across codd_knn_upsert_host, _upsert_device and _load_rows:
 * every slot such a call writes, and every slot that comes into existence below a write that starts above the count,
 * is marked PENDING (a device bitmap with a host mirror, and a device list of the distinct pending slots; a slot
 * written twice is pending once).  The layout's own copy of a pending row is stale from then on.  All four IVF
 * entry points then scan the probed lists under deny | pending and score every pending slot from the main row store
 * with the canonical exact score under the call's own deny bits (tombstones, or ~allow | dead), one merge over both.
 * The contract is the IVF contract word for word with the pending rows counting as a list every query probes: the exact
 * canonical top-k among the allowed live rows of {rows of the probed lists that are not pending} U {pending rows};
 * nprobe >= nlist is codd_knn_search bit for bit.  Probe selection is unchanged, the device-mask form stays free of
 * host synchronisation, and with nothing pending a search enqueues exactly what it enqueues with the option off.
 * codd_knn_delete_host is followed as it always was (tombstones by original slot); codd_knn_compact still makes the
 * layout stale, and so do rows left pending when the option is switched off.
 * ivf_refresh: the FOLD.  Every pending slot is assigned its list — the top-1 of the coarse index's exact scan with the
 *           STORED row, widened to fp32, as the query: largest canonical dot product (cosine, ip), smallest canonical
 *           squared distance (l2), ties to the lower list — rows that are not pending keep theirs, and the layout is rebuilt
 *           on the device from the main row store (count per list, 64-bit prefix sums, scatter, gather); centroids and the
 *           coarse index are untouched.  Appended rows join the layout here; afterwards nothing is pending.  Asynchronous on
 *           `stream` and ordered like an upsert: searches enqueued earlier on any stream finish before the layout is replaced,
 *           later ones wait for it; nothing is read back (it blocks only where appended rows make the layout's buffers grow).
 *           Nothing pending: a no-op, nothing enqueued.  Option "ivf_follow" off, no layout or a stale one: EINVAL, nothing
 *           enqueued.  A search never folds; a write folds before it returns when more rows are pending than option
 *           "ivf_fold_rows" allows (0, the default: one mean list, ceil(rows of the layout / nlist)).
 */
int codd_knn_ivf_refresh(codd_knn_index* index, void* stream);

/*
 * Replaces: the `where={"namespace": ...}` of collection.query(query_texts=..., n_results=..., where=...) — the metadata
 *           filter of ChromaDB's query, for the one key every record of the path carries (store.py:236-238 writes
 *           "namespace" into each metadata).  Strings stay on the host: the façade numbers the namespaces, and the
 *           number is the row slot's SCOPE, a 32-bit label; 0 = no label.
 * set_scopes_host: the scope of n row slots (each < count; scope <= CODD_KNN_MAX_SCOPE, else EINVAL); 0 clears.  A slot listed
 *           more than once keeps the last value.  Exclusive like upsert, synchronous.  A slot keeps its scope when its vector is
 *           overwritten; a new slot starts with scope 0.
 * search_scoped: like codd_knn_search / _search_keys, restricted per query: query q sees only the rows whose scope equals
 *           dev_scopes[q] (device, B values) — the exact cosine top-k among them, the same scores, tie rule and padding.
 *           dev_scopes[q] == 0 means "every row": bit-identical to codd_knn_search (so that one batch can mix scoped and
 *           unscoped queries).  A scope no row carries, or a value above anything ever set, gives an empty result for that
 *           query (all keys 0, rows -1, distances +inf), not an error.  Any of dev_keys / dev_dist / dev_rows may be NULL.
 *           Asynchronous on `stream`, ordered against upserts like the other search entry points.  The rows of a scope are
 *           found through lists (row slots grouped by scope) that the first scoped search after a change of scopes or of the
 *           row count rebuilds on its stream; the scan reads rows_in_scope rows per group of up to four queries of that scope —
 *           the tool for scopes that hold a small share of the index.
 */
int codd_knn_set_scopes_host(codd_knn_index* index, const int64_t* host_slots, const uint32_t* host_scopes, int64_t n);
int codd_knn_search_scoped(codd_knn_index* index, const float* dev_queries, const uint32_t* dev_scopes, int B, int k,
                           uint32_t row_base, uint64_t* dev_keys, float* dev_dist, int64_t* dev_rows, void* stream);

/*
 * Replaces: the general `where` of collection.query(query_texts=..., n_results=..., where=...) — ChromaDB's metadata grammar
 *           ($eq, $ne, $gt, $gte, $lt, $lte, $in, $nin, $and, $or).  Metadata stays on the host: the façade evaluates the filter to
 *           a set of row slots and hands it over as a bitmap, bit (r & 31) of word (r >> 5) set = row slot r may be returned.
 *           One mask per call, shared by the B queries.
 * search_masked: like codd_knn_search / _search_keys, restricted to the rows that are allowed AND live: per query the exact cosine
 *           top-k among them — the same scores, tie rule and padding, min(k, m) hits where m is the number of such rows.  nwords
 *           must equal ceil(count / 32), else EINVAL; bits at or above count in the last word are ignored.  m == 0 gives an
 *           all-empty result (keys 0, rows -1, distances +inf) and launches no scan; an all-ones mask returns the bits of
 *           codd_knn_search.  Any of dev_keys / dev_dist / dev_rows may be NULL.
 *           host_allow_bits is host memory and is consumed before the call returns: the words are copied into a pinned staging
 *           buffer of the stream's workspace (and counted there against the index's own mirror of the tombstones, which gives m
 *           without reading anything back), from where one asynchronous copy on `stream` takes them to the device.  The caller
 *           may reuse or free its words at once.  A second masked search on the same stream waits on the host until the first
 *           one's copy has left the staging buffer — not for its kernels.  Those stay asynchronous on `stream`, ordered against
 *           upserts like the other search entry points, and masked searches on different streams overlap.
 *           Two routes, chosen from m, B and the index size; the choice affects time only, never the answer:
 *           the LIST route expands the mask into the ascending list of visible row slots and walks it as a scoped search walks
 *           a scope's list (m rows per group of up to four queries: small m); the DENSE route runs the ordinary dispatch of
 *           codd_knn_search with ~allow | dead in the place of the tombstone bits (large m: the MFMA filters score every row,
 *           the threshold anchors and the exact re-scoring drop the rows the mask denies).  A dense masked pass neither feeds
 *           the survivor watch of "shadow8" nor starts or uses up a cooldown.  An index stored with normalize = 0 takes no
 *           filter leg here either.
 */
int codd_knn_search_masked(codd_knn_index* index, const float* dev_queries, int B, int k, const uint32_t* host_allow_bits,
                           int64_t nwords, uint32_t row_base, uint64_t* dev_keys, float* dev_dist, int64_t* dev_rows, void* stream);

/*
 * Replaces: collection.delete(ids=..., where=...) — the row half (ChromaDB's own call; the reference never deletes).
 * delete_host: tombstones n row slots.  A slot outside [0, count) gives EINVAL and changes nothing; a slot that is dead already,
 *           or listed twice, is a no-op.  Exclusive like upsert, synchronous.  From then on NO search entry point returns the row:
 *           codd_knn_search, _search_keys, _search_scoped and _ivf_search give each query the exact canonical top-k among the LIVE
 *           rows it may see — same scores, tie rule and padding, min(k, live rows) hits.  An installed IVF layout stays valid (its
 *           scans mask by the original row slot); the scope lists are rebuilt by the next scoped search.  Both MFMA filters keep
 *           scoring dead rows (their shadows are untouched); the threshold anchors and the exact re-scoring drop them.
 *           A dead slot stays dead until codd_knn_compact: upsert_host, upsert_device, load_rows and set_scopes_host return EINVAL
 *           for it (no reuse: "ties -> the row inserted first" would break).  The slot-addressed readers — codd_knn_read_rows,
 *           _copy_rows_f32, _approx_scores — keep returning a dead slot's contents.  codd_knn_count keeps its meaning.
 * live_count: row slots in use minus the dead ones.
 * compact:  moves the live rows to slots 0 .. live-1 IN SLOT ORDER (new slot = live slots below the old one; the caller renumbers
 *           its own tables by the same rule), their scopes with them; clears the tombstones; count shrinks to the live count
 *           (*new_count, may be NULL), capacity is kept.  In place, through the bounded staging buffer of codd_knn_upsert_host —
 *           no second copy of the row store.  Both shadows are brought up to date by the next search that needs them, from the
 *           first moved row on; an installed IVF layout becomes stale, as after an upsert.  No dead row: a no-op that returns the
 *           count.  Exclusive, synchronous.  EDEVICE from compact means a HIP error struck while rows were being moved: the rows
 *           are then partly moved under the old tombstones and count, and the index must be destroyed and rebuilt.
 */
int codd_knn_delete_host(codd_knn_index* index, const int64_t* host_slots, int64_t n);
int codd_knn_live_count(const codd_knn_index* index, int64_t* out);
int codd_knn_compact(codd_knn_index* index, int64_t* new_count);

/*
 * Replaces: the `where_document` of collection.query(query_texts=..., n_results=..., where_document={"$contains": "..."}) — ChromaDB's
 *           substring filter on the stored documents (store.py:146-150 writes one per record).  The grammar ($contains, $not_contains,
 *           $and, $or) stays with the façade; what crosses this boundary is bytes: the documents once, then one needle per call, and
 *           the answer is a row bitmap on the device that codd_knn_search_masked_dev searches under.
 * set_documents_host: the document of row slot r is host_bytes[host_offsets[r] .. host_offsets[r + 1]), possibly empty; host_offsets holds
 *           n + 1 values.  n must equal the count, the offsets must be non-decreasing from 0, and no byte may be 0x00 — a violation of
 *           any of these returns EINVAL and changes nothing.  Replaces the whole snapshot; exclusive and synchronous, like upsert_host.
 *           The engine lays out its own ARENA: the documents back to back in slot order, one 0x00 behind every document (document r
 *           starts at arena offset host_offsets[r] + r; the arena has host_offsets[n] + n bytes, the "doc_bytes" stat), zero bytes
 *           behind the last separator up to the end of the allocation so that every load of the match kernel is unconditional, and the
 *           n + 1 arena offsets as int64 on the device.  The snapshot is derived data, like the shadows and the scope lists: it is never
 *           persisted, and it goes STALE on upsert_host, upsert_device, load_rows and a compact that moves rows, as an IVF layout does;
 *           delete_host leaves it valid.
 * match_documents: sets bit (r & 31) of dev_bits[r >> 5] iff document r contains the needle as a byte substring; every other bit of the
 *           nwords words, the bits at or above the count among them, is zero.  Slot-addressed: a dead slot's document is matched as it
 *           stands (the searches drop dead rows, as everywhere else).  needle_len in [1, CODD_KNN_MAX_NEEDLE], no 0x00 in the needle,
 *           nwords == ceil(count / 32), else EINVAL; a stale or absent snapshot: EINVAL.  host_needle is consumed before the call
 *           returns.  Asynchronous on `stream`: one hipMemsetAsync of dev_bits and one launch of doc_match_kernel (csrc/doc_match.h),
 *           which streams the arena once, "doc_tile_bytes" start positions per workgroup step — its cost is the arena's bytes whatever
 *           the documents' lengths are.  May be called from several host threads and streams, like a search.
 * match_documents_dfa: the `$regex` of the same filter grammar.  What crosses this boundary is a byte DFA, compiled from
 *           the pattern by the façade (codd_query_engine_amd/regex_dfa.py): host_class_of[256] maps a byte to its class, host_next is
 *           next[nstates][nclasses], one uint8 per entry.  Sets bit (r & 31) of dev_bits[r >> 5] iff the walk
 *           state = next[state][class_of[byte]] over document r's bytes and then one 0x00 (the arena's separator), from `start`, ends in
 *           `accept`; every other bit of the nwords words is zero.  The contract of match_documents otherwise: a current snapshot and
 *           nwords == ceil(count / 32), else EINVAL; a dead slot's document is matched as it stands; the host pointers are consumed
 *           before the call returns; callable from several host threads and streams.  THE TABLE IS VALIDATED ON THE HOST before anything
 *           is enqueued, so that no entry leads outside it on the device: nstates in [1, CODD_KNN_MAX_DFA_STATES], nclasses in [1, 256],
 *           nstates * nclasses <= CODD_KNN_MAX_DFA_TABLE, every class < nclasses, every entry < nstates, start and accept states,
 *           accept absorbing (next[accept][c] == accept for every c); a violation is EINVAL and changes nothing.  The table does not
 *           fit a kernel's argument segment: it is staged in pinned memory of the calling stream's workspace and copied on `stream`.
 *           Asynchronous on `stream`: that copy and one launch of doc_regex_kernel (csrc/doc_regex.h) — document-parallel, one lane per
 *           document, "doc_regex_run_docs" consecutive documents per workgroup, their arena range staged "doc_regex_tile_bytes" at a
 *           time; the bitmap is written by wave ballots, every word once: no memset, no atomics.
 * search_masked_dev: codd_knn_search_masked under a mask that is already on the device — the same answer contract, word for word: the
 *           exact canonical top-k among the rows that are allowed AND live, min(k, m) hits, m == 0 an all-empty result with no scan, the
 *           same two routes chosen by the same rule from m, B and the index size, the same "mask_route" / "mask_list_pct" options and
 *           the same masked counters (plus "masked_dev_searches").  dev_allow_bits are nwords == ceil(count / 32) device words, read on
 *           `stream` behind whatever wrote them there (codd_knn_match_documents, a torch bitwise op ...); a small kernel clips them to
 *           [0, count) into the index's own allow buffer, so the caller's words are not needed once `stream` has run the call, and counts
 *           m on the way against the tombstone bits.  m decides the route and sizes the list, so it is READ BACK: THE CALL SYNCHRONISES
 *           `stream` ONCE, before it launches the scan (holding the index's enqueue lock meanwhile).  This entry point is therefore not
 *           asynchronous with respect to the host; the scan, merge and outputs behind the read-back are enqueued as usual.
 */
#define CODD_KNN_MAX_NEEDLE 256
int codd_knn_set_documents_host(codd_knn_index* index, const uint8_t* host_bytes, const int64_t* host_offsets, int64_t n);
int codd_knn_match_documents(codd_knn_index* index, const uint8_t* host_needle, int needle_len,
                             uint32_t* dev_bits, int64_t nwords, void* stream);
#define CODD_KNN_MAX_DFA_STATES 255
#define CODD_KNN_MAX_DFA_TABLE 8192   /* bytes of next[nstates][nclasses] */
int codd_knn_match_documents_dfa(codd_knn_index* index, const uint8_t* host_class_of, const uint8_t* host_next, int nstates, int nclasses,
                                 int start, int accept, uint32_t* dev_bits, int64_t nwords, void* stream);
int codd_knn_search_masked_dev(codd_knn_index* index, const float* dev_queries, int B, int k, const uint32_t* dev_allow_bits,
                               int64_t nwords, uint32_t row_base, uint64_t* dev_keys, float* dev_dist, int64_t* dev_rows, void* stream);

/*
 * Replaces: the `where` / `where_document` of collection.query on the two routes that scale the engine: the coarse-IVF search and
 *           the row-sharded search.  The masks are those of codd_knn_search_masked: bit (r & 31) of word (r >> 5)
 *           set = ORIGINAL row slot r may be returned; one mask per call, shared by the B queries.
 * ivf_search_masked: codd_knn_ivf_search restricted to the rows that are allowed AND live.  Probe selection is unchanged: the nprobe
 *           best lists per query come from the exact centroid score, whatever the mask says — the mask removes rows from the probed
 *           lists, it never sends the search to other lists.  The answer is the exact canonical top-k among the rows that are
 *           allowed, live and in the probed lists: the same scores, tie rule and padding, min(k, such rows) hits — under a mask that
 *           leaves few rows in the probed lists that is fewer than k, and fewer than codd_knn_search_masked finds.  With
 *           nprobe == nlist the result is the bits of codd_knn_search_masked; an all-ones mask returns the bits of
 *           codd_knn_ivf_search; a mask that allows no row (or only dead ones) gives an all-empty result (keys 0, rows -1, distances
 *           +inf).  nwords must equal ceil(count / 32), else EINVAL; bits at or above count are ignored.  No IVF layout, or a stale one
 *           (rows changed since codd_knn_ivf_install): EINVAL, as for codd_knn_ivf_search; B, k, nprobe and the three outputs as there.
 *           host_allow_bits is host memory and is consumed before the call returns, by the staging and copy rules of
 *           codd_knn_search_masked: the words are clipped into the pinned staging buffer of the stream's workspace, from where one
 *           asynchronous copy on `stream` takes them to the device; the caller may reuse or free its words at once; a second
 *           host-mask search on the same stream waits on the host until the first one's copy has left the staging buffer — not for
 *           its kernels.  One small kernel then writes ~allow | dead into the workspace, and the list scans test that bitmap, by
 *           original row slot, where they test the tombstone bits otherwise: the same kernels and launches as codd_knn_ivf_search
 *           (the per-pair scan, or the list-sharing scan from 1,024 pairs on), one launch more.
 * ivf_search_masked_dev: the same under a mask that is already on the device: nwords device words, read on `stream` behind whatever
 *           wrote them there (codd_knn_match_documents, codd_knn_slice_mask, a torch bitwise op ...), once, by that small kernel;
 *           the caller's words are not needed once `stream` has run the call.  THE ROUTE DOES NOT DEPEND ON THE NUMBER OF VISIBLE
 *           ROWS, so nothing is counted and nothing is read back: unlike codd_knn_search_masked_dev this entry point does not
 *           synchronise `stream` and is asynchronous with respect to the host, like codd_knn_ivf_search.
 * slice_mask: a shard's words out of a mask over GLOBAL rows — a `where` mask is compiled once over global row numbers and
 *           replicated; every rank of a row-sharded index cuts its own rows out on its device and searches under the result
 *           (_search_masked_dev, _ivf_search_masked_dev).  Static like codd_knn_merge_keys, `device` as in codd_knn_create.
 *           dev_global_bits: ceil(global_rows / 32) device words, bit g of the mask = global row g.  dev_out: nwords ==
 *           ceil(count / 32) device words (else EINVAL); bit r of the result = global bit row_base + r for r < count and
 *           row_base + r < global_rows, every other bit zero.  row_base is arbitrary — not a multiple of 32 in general: an output word
 *           is a funnel shift of two neighbouring global words — and may lie at or past global_rows (all zero); negative
 *           global_rows, row_base or count: EINVAL.  No word past the last global word is loaded; bits of that word at or above
 *           global_rows are ignored.  Asynchronous on `stream`; one launch of mask_slice_kernel (csrc/doc_match.h).
 */
int codd_knn_ivf_search_masked(codd_knn_index* index, const float* dev_queries, int B, int k, int nprobe, const uint32_t* host_allow_bits,
                               int64_t nwords, uint32_t row_base, uint64_t* dev_keys, float* dev_dist, int64_t* dev_rows, void* stream);
int codd_knn_ivf_search_masked_dev(codd_knn_index* index, const float* dev_queries, int B, int k, int nprobe, const uint32_t* dev_allow_bits,
                                   int64_t nwords, uint32_t row_base, uint64_t* dev_keys, float* dev_dist, int64_t* dev_rows, void* stream);
int codd_knn_slice_mask(int device, const uint32_t* dev_global_bits, int64_t global_rows, int64_t row_base, int64_t count, uint32_t* dev_out,
                        int64_t nwords, void* stream);

/*
 * Replaces: the embedding step inside collection.query(query_texts=[...]) (store.py:314-316) and collection.upsert(documents=[...])
 *           (store.py:236-238) — what chromadb's client does to the texts before the search — for the façade's default embedder,
 *           HashingEmbeddingFunction (codd_query_engine_amd/embedding.py): ASCII text in, its vectors out, on the device, BIT-EQUAL to
 *           the host embedder.  An index does not exist before the first upsert fixes the width, so the embedder is an
 *           object of its own.
 * embedder_create: dim in [8, 4096] and a finite trigram_weight (the fp32 rounding of the host's), else EINVAL; device >= 0.  Touches no
 *           device: that `device` exists is checked by the first call that embeds (EINVAL there).
 * embedder_destroy: frees the embedder's staging buffers and events (codd_knn_debug_live_allocations returns to its earlier values);
 *           NULL: OK.  No call on the embedder may be in flight on the host.
 * embed_texts_host: text r is host_bytes[host_offsets[r] .. host_offsets[r + 1]), possibly empty; host_offsets holds n + 1 values.  The
 *           offsets alone separate the texts — no separator bytes, 0x00 is an ordinary non-word byte.  dev_out: n x dim fp32 on the
 *           embedder's device, EVERY element written (a bucket without a feature is +0.0; the caller clears nothing).  Per text: a word
 *           byte is [0-9A-Za-z_], low() maps A-Z to a-z, a token is a maximal run of word bytes inside the text; for each word byte at
 *           position p, in increasing p: if p starts a token, out[crc32("w:" + low(token)) % dim] += 1.0f; then always
 *           out[crc32("t:" + a + low(b[p]) + c) % dim] += trigram_weight, a = low(b[p - 1]) or '^' at the token's start, c = low(b[p + 1])
 *           or '$' at its end; crc32 is zlib's.  The fp32 additions into one bucket happen in exactly this order, whatever the lanes'
 *           timing: the order is part of the bits.
 *           EINVAL, with nothing enqueued: a null embedder, offsets or output; n < 0 or n > CODD_KNN_MAX_EMBED_TEXTS; offsets that do not
 *           start at 0 or decrease; more than CODD_KNN_MAX_EMBED_BYTES bytes; null host_bytes unless the total is 0; a byte at or above
 *           0x80 (such texts are the host embedder's: Unicode's \w and lower() are not restated here).  n == 0: OK, no launch.
 *           host_bytes and host_offsets are consumed before the call returns: copied into the embedder's pinned staging buffer, from
 *           where one asynchronous copy on `stream` takes them to the device, and one launch of text_embed_kernel (csrc/text_embed.h)
 *           follows.  By the staging rule of codd_knn_search_masked, a second call waits on the host until the first one's copy has left
 *           the staging buffer — not for its kernel; a call on another stream is ordered on the device behind the previous call's
 *           kernel, which reads the same device copy of the texts.  Everything else is asynchronous on `stream`.  Calls from several
 *           host threads are serialised by the embedder's own lock.
 */
#define CODD_KNN_MAX_EMBED_BYTES (1ll << 28)   /* text bytes per codd_knn_embed_texts_host call */
#define CODD_KNN_MAX_EMBED_TEXTS (1ll << 24)   /* texts per call */
typedef struct codd_knn_embedder codd_knn_embedder;
int codd_knn_embedder_create(codd_knn_embedder** out, int device, int dim, float trigram_weight);
int codd_knn_embedder_destroy(codd_knn_embedder* e);
int codd_knn_embed_texts_host(codd_knn_embedder* e, const uint8_t* host_bytes, const int64_t* host_offsets, int64_t n, float* dev_out,
                              void* stream);

/*
 * Replaces: the general `where` of collection.query once more — this time the filter itself runs on the device.
 *           Strings still stay on the host: what crosses this boundary is, per metadata key, a COLUMN — for every row slot a tag
 *           (CODD_KNN_WHERE_TAG_*: absent, bool, number, str) and a 64-bit cell — and, per filter, a PROGRAM over the columns; the
 *           answer is a row bitmap on the device, in the form codd_knn_match_documents produces, that codd_knn_search_masked_dev,
 *           codd_knn_ivf_search_masked_dev and codd_knn_slice_mask take.  A C caller has a metadata filter without building bitmaps.
 *           Cells: bool 0 / 1; number the order-preserving key of the float64 x: the bits of x + 0.0 (so that -0.0 and +0.0 agree),
 *           all of them flipped for a negative x, else the sign bit alone — unsigned comparison of keys is numeric comparison, and
 *           the device performs no floating-point operation; str a code of the caller's own dictionary.  An absent cell is ignored.
 * set_column_host: writes tag and cell of n row slots of column `column` (< CODD_KNN_MAX_COLUMNS).  host_slots == NULL: the rows
 *           0 .. n-1, a full upload (n <= count).  Otherwise each slot must lie in [0, count) and be live, else EINVAL and nothing
 *           changes; a slot listed more than once keeps the last value.  A tag above CODD_KNN_WHERE_TAG_STR: EINVAL.  A column's
 *           storage follows the scope labels': allocated by the first call that names it, as long as the row store and zero (absent)
 *           wherever nothing was written; it grows with the row store, codd_knn_compact moves it with the rows by the same stable
 *           mapping (the vacated slots read absent again), codd_knn_load_rows drops every column, and a slot keeps its cell when its
 *           vector is overwritten.  Derived data: never persisted.  Exclusive like upsert, synchronous.  An index without a row slot:
 *           EINVAL.
 * drop_columns: frees every column.  Exclusive, synchronous.
 * eval_where: sets bit (r & 31) of dev_out_bits[r >> 5] iff r < count, row slot r is not a tombstone and the program accepts it;
 *           every other bit of the nwords == ceil(count / 32) words (else EINVAL) is zero.  The program: leaf i passes for a row iff
 *           the row's tag in column leaves[i].column equals leaves[i].tag AND, kind CODD_KNN_WHERE_IN, the cell equals one of
 *           literals[lit_first .. lit_first + lit_count) (no literal: nothing passes), or, kinds _LT _LE _GT _GE, the cell compares so,
 *           unsigned, with the one literal; with `negate` the leaf passes iff that fails — an absent cell then passes, ChromaDB's $ne
 *           and $nin.  ops[0 .. nops) is a postfix expression: a value below CODD_KNN_WHERE_AND pushes that leaf's result,
 *           CODD_KNN_WHERE_AND and _OR replace the two top entries by their conjunction / disjunction; the one value left is the row's
 *           verdict.  (p pushes need p - 1 operators: a well-formed program has an odd nops, 63 at the most.)
 *           THE PROGRAM IS VALIDATED ON THE HOST before anything is enqueued; a failed check is EINVAL with a message, no launch and
 *           no change: nleaves in [1, CODD_KNN_WHERE_MAX_LEAVES], nliterals in [0, CODD_KNN_WHERE_MAX_LITERALS], nops in
 *           [1, CODD_KNN_WHERE_MAX_OPS]; every leaf's column below CODD_KNN_MAX_COLUMNS and SET on this index, its tag one of bool /
 *           number / str, its kind known, negate 0 or 1, its literal range inside the literals; a comparison leaf on class number with
 *           exactly one literal; every pushed leaf below nleaves; the expression never underflows, needs at most 32 stack entries and
 *           leaves exactly one value.  `prog` is host memory, consumed before the call returns: it travels to the device as a kernel
 *           argument.  Asynchronous on `stream`, ordered against upserts like a search, nothing read back: one launch of
 *           where_eval_kernel (csrc/where_eval.h), a stream of 9 bytes per row and distinct column that writes every output word
 *           once — no memset, no atomics.  May be called from several host threads and streams, like a search.
 */
#define CODD_KNN_MAX_COLUMNS 32            /* columns per index */
#define CODD_KNN_WHERE_MAX_LEAVES 32
#define CODD_KNN_WHERE_MAX_LITERALS 256
#define CODD_KNN_WHERE_MAX_OPS 64
#define CODD_KNN_WHERE_TAG_ABSENT 0
#define CODD_KNN_WHERE_TAG_BOOL 1
#define CODD_KNN_WHERE_TAG_NUMBER 2
#define CODD_KNN_WHERE_TAG_STR 3
#define CODD_KNN_WHERE_IN 0
#define CODD_KNN_WHERE_LT 1
#define CODD_KNN_WHERE_LE 2
#define CODD_KNN_WHERE_GT 3
#define CODD_KNN_WHERE_GE 4
#define CODD_KNN_WHERE_AND 0xFE            /* postfix operators; a value below these pushes that leaf */
#define CODD_KNN_WHERE_OR 0xFF
typedef struct codd_knn_where_leaf {
    uint8_t column, tag, kind, negate;
    uint16_t lit_first, lit_count;
} codd_knn_where_leaf;
typedef struct codd_knn_where_program {
    int32_t nleaves, nliterals, nops, reserved;
    codd_knn_where_leaf leaves[CODD_KNN_WHERE_MAX_LEAVES];
    uint8_t ops[CODD_KNN_WHERE_MAX_OPS];
    uint64_t literals[CODD_KNN_WHERE_MAX_LITERALS];
} codd_knn_where_program;
int codd_knn_set_column_host(codd_knn_index* index, int column, const int64_t* host_slots, const uint8_t* host_tags, const uint64_t* host_cells,
                             int64_t n);
int codd_knn_drop_columns(codd_knn_index* index);
int codd_knn_eval_where(codd_knn_index* index, const codd_knn_where_program* prog, uint32_t* dev_out_bits, int64_t nwords, void* stream);

/*
 * Tuning / introspection (never needed for correctness).
 *   options: "scan_blocks_per_cu" (4; 1..8: workgroups per compute unit of the exact scan, at most); "filter" (0/1: MFMA filter path for large batches);
 *            "filter_min_batch" (9), "filter_min_rows" (1: batches >= filter_min_batch always
 *            filter when the corpus has >= 2k sample tiles), "filter_min_rows_small" (100000:
 *            smaller batches filter when rows * B reaches it): when the filter path is taken;
 *            "sample_div" (40: about 1/40 of the tiles set the per-query thresholds, never
 *            fewer than one tile per CU once the corpus has two rounds of tiles), "sample_tiles"
 *            (4096: upper bound on that number), "hit_cap" (131072: per-query
 *            candidate capacity; overflow falls back to the exact scan);
 *            "all_normalized" (write 0 only: the caller knows of stored rows that are not unit
 *            vectors, e.g. a persisted index whose manifest says so: filters off for good);
 *            "shadow8" (1: batches of <= "shadow8_max_batch" (256) queries are filtered through an
 *            int8 copy of the corpus, 1 byte per element, derived lazily from the stored rows and
 *            kept up to date incrementally; results stay exact; an index whose worst row quantises
 *            badly — error norm above 0.04 — keeps the 2-byte (fp16) filter; so does, for the next
 *            "shadow8_cooldown" (256) searches, an index whose int8 passes leave more than
 *            "shadow8_max_surv" (4000) survivors per query or send queries to the fallback: dense
 *            clusters — unless the 2-byte passes are seen to leave at least half as many), "sample_div8" (28:
 *            the int8 filter's thresholds come from a sample of 1/28 of the row tiles) and
 *            "sample_rounds8" (2: ... of at least that many tiles per compute unit for batches of
 *            more than 32 queries, up to a quarter of the corpus; performance only),
 *            "sample_cascade" (1: a pass of the static int8 tile program — 65..256 queries, rows of 768 int8 elements — whose sample
 *            would take "cascade_min_rounds" (3) rounds of workgroups fixes its thresholds in two steps, a one-round sample and then
 *            the filter program itself over every ("cascade_d" (16) + 1)-th tile, whose candidates are kept and whose tiles the main
 *            launch skips: those tiles are not scanned a second time; 2: wherever that applies, whatever the size; 0: never.  Same ids
 *            and distance bits either way), "cascade_d" (16, in [16,64]: d of that pass is the divisor of the number of
 *            compute units in [16,64] nearest this value; no such divisor: no cascade), "cascade_min_rounds" (3, in [1,64]: the size
 *            rule of "sample_cascade" = 1; both are measured settings, profiles/cascade/README.md; the first sample takes at most
 *            "sample_tiles" tiles like the plain one),
 *            "i8_sweep" (1: a filter pass of 129..256 queries over rows of 768 int8 elements runs the static tile program in its sweep
 *            form — tiles of odd ordinal walk the K-steps the other way round, so a tile stages two query slices instead of six; same
 *            candidates, same ids and distance bits; 0: i8_tile_kernel's static program),
 *            "resident_q" (1: rows of <= 512 int8 elements keep the query block in LDS for the
 *            whole launch), "i8v2" (2: batches of 65..256 queries on rows of 384 or
 *            more elements take the second-generation int8 kernel, csrc/filter_i8.h; 1: only rows of
 *            more than 512 elements; 0: never), "i8v2_half" (1: batches of 65..128 queries take that kernel's
 *            8-query-block instantiation; 0: the first-generation kernel),
 *            "i8_pair" (2: that kernel synchronises once per two K-steps on rows of 768 / 1536 ... elements, and rows of exactly 768 take its static form; 1: without the static form; 0: every
 *            K-step), "per_block" (7, bit mask: the int8 bound uses each 32-row block's own quantisation error instead of
 *            the corpus's worst — bit 0 in the tile kernel, bit 1 in finalize (bit 2 is accepted and ignored: the
 *            tile kernel's filter pass always fetches the block metadata by one LDS-DMA per tile); 0 = the device-wide bound everywhere), "fuse_fallback" (1: every pass of the 2-byte filter and the int8 passes of more than 64 queries, k <= 64,
 *            answer candidate-list overflows inside the finalize launch; 0: a launch of their own), "small_batch_max" (0; 1: a single query,
 *            k <= 64, on an index of 4,096 rows or more whose int8 rows are 384, 512, 768 or 1,024 elements wide is answered by ONE
 *            launch — measured slower than the three-launch chain, see DESIGN.md §12, hence off), "f16_tile" (1: the 2-byte filter of 129..256 queries on rows of 384 / 768 / 1152 ... elements runs
 *            csrc/filter_i8.h's tile program on fp16 operands; 0: the first-generation kernel), "ivf_share" (1: codd_knn_ivf_search scans a probed list once for all queries of the
 *            batch that probe it, from 1,024 (query, list) pairs on; 0: once per pair),
 *            "compact_chunk_rows" (0: codd_knn_compact moves as many source rows per step as 64 MiB hold; N: N rows — tests),
 *            "mask_route" (0: codd_knn_search_masked chooses its route by the rule of DESIGN.md §15; 1: always the list route; 2: always the
 *            dense route), "mask_list_pct" (100: the weight of the dense side in that rule's cost comparison, in percent — above 100 more
 *            searches take the list route, 0 none that the rule decides by cost),
 *            "where_max_blocks" (0: codd_knn_eval_where launches as many workgroups as the rows need, at most eight per compute unit; N: at
 *            most N — tests: the answer never depends on it),
 *            "space_filter" (0; 1: an ip or l2 index filters batches of "filter_min_batch" queries and more over "filter_min_rows" rows
 *            and more through the int8 MFMA filter with measured norms in its bound, then re-scores exactly — same ids and distance
 *            bits as the scan; needs "filter" and "shadow8" on, l2 rows of at most 4 chunks per lane; no effect on a cosine index;
 *            DESIGN.md §21),
 *            "space_ivf" (0; 1: codd_knn_ivf_install and the IVF searches accept an ip or l2 index — raw centroids, a coarse index
 *            and list scans in the index's own space; 0: they return ENOTSUP there; no effect on a cosine index),
 *            "ivf_follow" (0; 1: an installed IVF layout follows upsert_host, upsert_device and load_rows — written rows are pending
 *            until a fold, see codd_knn_ivf_refresh), "ivf_fold_rows" (0; a write folds when more rows than this are
 *            pending; 0 = one mean list of the layout; at most 2^32),
 *            "debug_fail_shadow_alloc" (tests; a switch, not a count: while it is non-zero every allocation of the 2-byte shadow fails as
 *            if HBM were full; 0 switches it off and lets the next search try again),
 *            "debug_num_cus" (tests; 0: off; N in [1, the device's compute units]: the filter passes plan and launch their sample and
 *            filter programs as if the device had N compute units, so that a small corpus gives a workgroup several tiles; the answer
 *            never depends on it);
 *            "profile" = N keeps N (start, stop) HIP-event pairs, one per heavy-kernel launch,
 *            recorded on the launch stream (0 = off; resets the log)
 *   stats  : "searches", "scan_launches", "last_scan_blocks", "last_scan_group" (queries per pass over the rows of the
 *            last exact scan), "last_finalize_parts" (workgroups per query of the last filter pass's finalize),
 *            "ivf_shared_searches" (IVF searches that scanned each probed list once for all its queries), "ivf_masked_searches" (IVF searches
 *            under a row mask, host or device words), "ivf_pending_rows" (distinct row slots pending under a layout that follows
 *            writes), "ivf_refreshes" (folds, by codd_knn_ivf_refresh or by a write), "ivf_delta_searches" (IVF searches that ran a
 *            delta scan over pending rows), "ivf_rows" (rows the layout holds), "ivf_fold_threshold" (pending rows above which a write
 *            folds), "ivf_follow", "ivf_fold_rows" (the options), "scoped_searches",
 *            "scope_builds" (times the scope lists were rebuilt), "scopes" (highest scope label ever set), "dead_rows" (tombstones below count),
 *            "delete_calls", "compactions" (codd_knn_compact calls that moved rows), "masked_searches", "mask_list_searches",
 *            "mask_dense_searches" (masked searches by route), "last_mask_rows" (allowed live rows of the last masked search),
 *            "mask_filter_hits", "mask_filter_survivors", "mask_fallback_queries" (the device counters of the dense masked passes, kept
 *            apart from the three below), "masked_dev_searches" (the masked searches among them that came through
 *            codd_knn_search_masked_dev), "docs_valid" (1: a document snapshot exists and is not stale), "doc_bytes" (its arena: the
 *            documents' bytes plus one separator each), "doc_tile_bytes" (arena bytes per workgroup step of doc_match_kernel),
 *            "doc_matches" (codd_knn_match_documents calls that launched), "doc_regex_matches" (codd_knn_match_documents_dfa calls that
 *            launched), "doc_regex_tile_bytes" (arena bytes per segment of doc_regex_kernel), "doc_regex_run_docs" (documents per
 *            workgroup of it), "where_evals" (codd_knn_eval_where calls that launched), "where_columns" (columns set), "where_column_bytes"
 *            (their device bytes: 9 per row slot of the capacity and column), "filter_passes", "cascade_passes" (the filter passes among them that took the sample cascade), "last_cascade_d"
 *            (the d of the last filter pass's cascade, 0: it took none), "sweep_passes" (the filter passes whose filter launches ran
 *            i8_sweep_kernel), "last_sweep" (1: the last filter pass was one of them; family TILE and ts 3 either way),
 *            "fallback_queries", "filter_hits", "filter_survivors", "capacity_rows",
 *            "device_bytes", "num_cus", "workspaces" (stream workspaces in use), "shadow8_builds", "shadow8_passes", "i8v2_passes",
 *            "shadow16_builds" (the 2-byte (fp16) shadow is built lazily, by the first search that needs it), "all_normalized",
 *            "shadow8_cooldowns", "shadow8_eps_r_micro", "shadow8_wide_blocks" (32-row blocks whose quantisation error is above
 *            0.04: tolerated up to 1 % of the blocks), "shadow16_alloc_failures", "small_batch_passes", "f16_tile_passes", "space_filter", "space_ivf" (the options), and per kernel K in {scan, filter, sample, finalize}:
 *            "events:K", "time_ns:K" (sum of the recorded launches; syncs on the last event)
 */
int codd_knn_set_option(codd_knn_index* index, const char* key, int64_t value);
int codd_knn_get_stat(const codd_knn_index* index, const char* key, int64_t* out);

/* What the library holds at this moment, in the whole process: device and pinned host buffers, their bytes, and HIP events.
 * Every index takes what it allocates back in codd_knn_destroy, so the three figures return to what they were before
 * codd_knn_create (tests compare against such a baseline: other indexes may be alive).  No device call; EINVAL for a null pointer. */
int codd_knn_debug_live_allocations(int64_t* buffers, int64_t* bytes, int64_t* events);

/*
 * Debug: what the LAST filter pass (sample -> anchor -> filter -> finalize) on `stream`'s workspace left behind,
 * copied to the host.  Takes that workspace, synchronises the stream, copies; launches no kernel and changes no state (a stream
 * that never searched this index takes no workspace).  A search of more than 256 queries runs one pass per 256 queries over the
 * same workspace: only its last pass is left.  EINVAL, nothing copied: null index, a negative size, no filter pass has run on that
 * workspace, or bucket_max_cap too small.  Any output pointer may be NULL.
 * "That workspace" is the slot, not the stream: an index keeps four, and a fifth stream takes over the least recently used one
 * with the record of its previous owner's last pass, until its own first filter pass replaces it.
 * The record is written on the host when the pass is enqueued, so replaying a captured graph does not refresh it; and the call
 * synchronises the stream, so it must not be made while that stream is capturing.
 *   info        the program that ran and the pass's shape (below)
 *   thr         [512]   thr[q], then thr0[q] (thr0: int8 passes only)
 *   qmeta       [1024]  int8 passes only (info->el = 1; untouched otherwise): q-scale, 2 eps(q), A(q), B(q) — for an l2 index
 *                       [512 + q] is the query's sum of squares
 *   hit_counts  [256]   the raw candidate counters as they are: above hit_cap where a list was cut
 *   fb_list     [256]   the fallback queue's words (info->fb_count of them are entries where finalize ran as its own launch; the
 *                       fused finalize derives the queue from the counters and writes neither)
 *   keys        [256][keys_per_query]  the first min(counter, hit_cap, keys_per_query) candidate keys of each query (approximate
 *                       score in the high word, 0xFFFFFFFF - local row in the low one); the rest is untouched
 *   bucket_max  [256][info->sample_tiles]  the sample pass's best key per (query, sampled tile); bucket_max_cap: u64 the buffer holds
 *                       (a cascade pass: its first sample's; info->cascade_d)
 *   bmeta       [min(bmeta_blocks, ceil(n / 32))][2]  int8 passes only: {scale, error norm} of the index's 32-row blocks as they are now
 */
typedef struct codd_knn_last_pass {
    int32_t family;             /* 0 GEMM (gemm_filter_kernel, sqd_filter_kernel), 1 TILE (i8_tile_kernel, i8_sweep_kernel), 2 TILE_F16 */
    int32_t nbq, ts, res, el, sqd;
    int32_t nq, k;
    int32_t hit_cap;
    int32_t per_block_filter;   /* the filter launch evaluated the int8 bound per 32-row block (thr0, bmeta) */
    int32_t per_block_finalize; /* ... and so did finalize */
    float eps;                  /* filter_eps(): the 2-byte filter's slack (recorded for every pass) */
    int64_t n;                  /* rows the pass ran over */
    int64_t sample_tiles, sample_stride;
    uint32_t flags[4];          /* FLAG_* words of the control block: [0] a workgroup hit list filled up, [1] a query was queued */
    uint32_t fb_count;
    uint32_t cascade_d;         /* the pass took the sample cascade with this d; then sample_tiles, sample_stride are those of
                                   its first sample, whose first tile is tile 1 and whose keys count rows from row 256.  0: it did not */
} codd_knn_last_pass;
int codd_knn_debug_last_pass(codd_knn_index* index, void* stream, codd_knn_last_pass* info, float* thr, float* qmeta,
                             uint32_t* hit_counts, uint32_t* fb_list, uint64_t* keys, int64_t keys_per_query,
                             uint64_t* bucket_max, int64_t bucket_max_cap, float* bmeta, int64_t bmeta_blocks);

#ifdef __cplusplus
}
#endif
#endif /* CODD_KNN_H */
