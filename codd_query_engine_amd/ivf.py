"""
Coarse-IVF over a DeviceKnnIndex (BASELINE config 5: the small-batch, HBM-bound regime).

Build (offline, once per corpus):  spherical k-means on a sample of the stored rows, then every
row is assigned to its nearest centroid and the rows are regrouped by list.
  * the heavy part of every step — scores of 256 rows against all centroids — is the engine's own
    bf16 MFMA GEMM (`codd_knn_approx_scores` on an index that holds the centroids);
  * torch supplies argmax / index_add / sort on the device: bookkeeping around the GEMM, not search.
An ip or l2 index (opt-in, option "space_ivf") is clustered in its own space instead: a centroid is the plain
mean of its members, and every assignment is the exact search of a centroid index of that space (nearest centroid by squared
distance for l2 — Lloyd's algorithm — and largest inner product for ip, the usual inner-product IVF).
Search: `codd_knn_ivf_search` (HIP): exact top-nprobe lists per query, canonical exact scores over
those lists, original row slots; `nprobe == nlist` reproduces the flat search bit for bit.
Writes: by default any upsert makes the layout stale and `build_ivf` is the remedy.  With `follow_writes(index)` (engine option
"ivf_follow") written rows are pending instead — every IVF search scores them exactly from the row store beside the
probed lists — until `refresh_ivf(index)`, or a write that crosses "ivf_fold_rows", folds them into their lists on the device.

The reference has no counterpart (ChromaDB answers with HNSW, store.py:63-68); results are
approximate by design and reported as recall@k against this engine's exact search.
"""

from __future__ import annotations

import ctypes
from typing import Optional

from . import native
from .knn_index import DeviceKnnIndex


def _require_cosine(index) -> None:
    """IVF serves a cosine index, and an ip or l2 index whose "space_ivf" option is on; by default an ip or l2
    index has none (spherical k-means and the bf16 cosine GEMM of the assignment are cosine-specific)."""
    space = getattr(index, "space", "cosine")
    if space != "cosine" and not index.stat("space_ivf"):
        raise native.NativeLibraryError(f"IVF exists for the cosine space only, this index is {space!r}: search it with the exact scan")


def _assign(torch, centroid_index: DeviceKnnIndex, vecs) -> "torch.Tensor":
    """nearest centroid (by approximate cosine) of every row of `vecs` [n, dim] (device fp32)."""
    nlist = centroid_index.count()
    out = torch.empty(vecs.shape[0], dtype=torch.int64, device=vecs.device)
    for a in range(0, vecs.shape[0], 256):
        chunk = vecs[a : a + 256]
        scores = centroid_index.approx_scores(chunk)[: chunk.shape[0], :nlist]
        out[a : a + chunk.shape[0]] = torch.argmax(scores, dim=1)
    return out


def _assign_exact(torch, centroid_index: DeviceKnnIndex, vecs) -> "torch.Tensor":
    """the best centroid of every row of `vecs` [n, dim] (device fp32) by the exact search of the centroid index's own space:
    smallest canonical squared distance (l2), largest canonical inner product (ip); ties to the lower list."""
    out = torch.empty(vecs.shape[0], dtype=torch.int64, device=vecs.device)
    for a in range(0, vecs.shape[0], 1024):
        chunk = vecs[a : a + 1024]
        out[a : a + chunk.shape[0]] = centroid_index.search_tensors(chunk.contiguous(), 1)[1][:, 0]
    return out


def follow_writes(index: DeviceKnnIndex, on: bool = True, fold_rows: Optional[int] = None) -> None:
    """Let an installed layout follow writes: with `on`, rows written by upsert, upsert_device and load_rows are
    pending — scanned exactly from the row store by every IVF search — until a fold puts them into their lists.  fold_rows: a
    write folds when more rows than this are pending (None leaves the option alone; 0 = one mean list, the default).  With
    `on` False the next write makes the layout stale again, and so do rows that are still pending."""
    index.set_option("ivf_follow", 1 if on else 0)
    if fold_rows is not None:
        index.set_option("ivf_fold_rows", int(fold_rows))


def refresh_ivf(index: DeviceKnnIndex) -> None:
    """Fold the pending rows into the layout now (codd_knn_ivf_refresh): each is assigned the list of its best centroid by the
    coarse index's exact search, the others keep theirs, and the layout is rebuilt on the device.  Centroids stay as they are."""
    index.ivf_refresh()


def build_ivf(index: DeviceKnnIndex, nlist: int, iters: int = 8, sample: Optional[int] = None, seed: int = 7,
              chunk_rows: int = 262_144, follow_writes: bool = False) -> dict:
    """Cluster the stored rows into `nlist` lists and install the layout on `index`.

    sample: rows used for training (default min(count, 64 * nlist)).  Returns list-size statistics.
    follow_writes: switch option "ivf_follow" on before the install, so that the layout survives later upserts (see
    follow_writes() above; off by default, and False leaves the option as it is).
    """
    import torch

    _require_cosine(index)
    if follow_writes:
        index.set_option("ivf_follow", 1)
    lib = native.load()
    n, dim, dev = index.count(), index.dim, index.device
    if n < nlist:
        raise ValueError(f"{n} rows cannot form {nlist} lists")
    stream = lambda: ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)  # noqa: E731

    def rows_f32(first: int, count: int):
        out = torch.empty((count, dim), dtype=torch.float32, device=dev)
        native.check(lib.codd_knn_copy_rows_f32(index._h, first, count, out.data_ptr(), stream()), "codd_knn_copy_rows_f32")
        return out

    g = torch.Generator(device="cpu").manual_seed(seed)
    m = min(n, sample or 64 * nlist)
    # training sample: evenly spaced blocks of rows (cheap to read back, representative of the whole corpus)
    nblk = max(1, min(m // 256, 4096))
    per = m // nblk
    starts = (torch.arange(nblk, dtype=torch.float64) * ((n - per) / max(nblk - 1, 1))).long().tolist()
    train = torch.cat([rows_f32(s, per) for s in starts])
    cent = train[torch.randperm(train.shape[0], generator=g)[:nlist].to(dev)].clone()

    space = getattr(index, "space", "cosine")
    spherical = space == "cosine"

    def centroid_index(cent):
        # cosine: unit centroids under the approximate GEMM; ip, l2: the centroids as they are, searched exactly in the index's space
        if spherical:
            cidx = DeviceKnnIndex(dim, "f32", str(dev))
            cidx.upsert_device(0, cent.contiguous())
        else:
            cidx = DeviceKnnIndex(dim, "f32", str(dev), space=space)
            cidx.upsert_device(0, cent.contiguous(), normalize=False)
        return cidx

    assign_rows = _assign if spherical else _assign_exact

    for _ in range(iters):
        cidx = centroid_index(cent)
        a = assign_rows(torch, cidx, train)
        cidx.close()
        sums = torch.zeros((nlist, dim), dtype=torch.float32, device=dev).index_add_(0, a, train)
        counts = torch.bincount(a, minlength=nlist)
        empty = counts == 0
        if empty.any():  # reseed empty lists from random training rows
            sums[empty] = train[torch.randint(0, train.shape[0], (int(empty.sum()),), generator=g).to(dev)]
        if spherical:
            cent = torch.nn.functional.normalize(sums, dim=1)
        else:  # the mean of the members (a reseeded list: the one row it was given)
            cent = sums / counts.clamp(min=1).to(torch.float32).unsqueeze(1)

    # assign every stored row, chunk by chunk, then group rows by list (stable: ascending slot inside a list)
    cidx = centroid_index(cent)
    assign = torch.empty(n, dtype=torch.int64, device=dev)
    for a0 in range(0, n, chunk_rows):
        c = min(chunk_rows, n - a0)
        assign[a0 : a0 + c] = assign_rows(torch, cidx, rows_f32(a0, c))
    cidx.close()
    perm = torch.sort(assign, stable=True).indices.contiguous()
    sizes = torch.bincount(assign, minlength=nlist)
    offsets = torch.zeros(nlist + 1, dtype=torch.int64, device=dev)
    offsets[1:] = torch.cumsum(sizes, 0)
    native.check(
        lib.codd_knn_ivf_install(index._h, cent.contiguous().data_ptr(), nlist, perm.data_ptr(), offsets.data_ptr(), stream()),
        "codd_knn_ivf_install",
    )
    torch.cuda.synchronize(dev)
    return {"nlist": nlist, "rows": n, "min_list": int(sizes.min()), "max_list": int(sizes.max()), "mean_list": n / nlist,
            "train_rows": int(train.shape[0]), "iters": iters}


def _is_device_mask(allow) -> bool:
    import torch

    return isinstance(allow, torch.Tensor) and allow.is_cuda


def search_ivf(index: DeviceKnnIndex, queries, k: int, nprobe: int, row_base: int = 0, allow=None):
    """(dist [B,k] fp32 ascending, rows [B,k] int64 original slots, -1 padded) on the device.

    allow: one row mask for the whole batch (a `where=` / `where_document=` filter).  A numpy bool array of length count() or
    packed uint32 words go through codd_knn_ivf_search_masked; a 1-d int32 CUDA tensor of packed words (match_documents' form)
    through codd_knn_ivf_search_masked_dev, with no host synchronisation.  The probed lists are the ones the unmasked search
    probes; the mask only removes rows from them, so a small mask may leave fewer than k hits."""
    import torch

    _require_cosine(index)
    row_base = native.check_row_base(row_base, index.count())
    if allow is not None:
        if _is_device_mask(allow):
            return index.ivf_search_masked_dev_tensors(queries, allow, k, nprobe, row_base)
        return index.ivf_search_masked_tensors(queries, allow, k, nprobe, row_base)
    lib = native.load()
    q = index._queries_tensor(queries)
    B = q.shape[0]
    dist = torch.empty((B, k), dtype=torch.float32, device=index.device)
    rows = torch.empty((B, k), dtype=torch.int64, device=index.device)
    native.check(
        lib.codd_knn_ivf_search(index._h, q.data_ptr(), B, int(k), int(nprobe), row_base, None, dist.data_ptr(), rows.data_ptr(),
                                index._stream()),
        "codd_knn_ivf_search",
    )
    return dist, rows


def search_ivf_keys(index: DeviceKnnIndex, queries, k: int, nprobe: int, row_base: int = 0, allow=None):
    """Shard-local half of a row-sharded IVF search: [B,k] packed keys carrying GLOBAL rows (as codd_knn_search_keys).
    allow: as in search_ivf (the mask is over the shard's LOCAL row slots)."""
    import torch

    _require_cosine(index)
    row_base = native.check_row_base(row_base, index.count())
    if allow is not None:
        if _is_device_mask(allow):
            return index.ivf_search_keys_masked_dev(queries, allow, k, nprobe, row_base)
        return index.ivf_search_keys_masked(queries, allow, k, nprobe, row_base)
    lib = native.load()
    q = index._queries_tensor(queries)
    B = q.shape[0]
    keys = torch.empty((B, k), dtype=torch.int64, device=index.device)
    native.check(
        lib.codd_knn_ivf_search(index._h, q.data_ptr(), B, int(k), int(nprobe), row_base, keys.data_ptr(), None, None, index._stream()),
        "codd_knn_ivf_search",
    )
    return keys


class IvfShardEngine:
    """What ShardedSearcher needs from an engine, answered by the shard's IVF lists (BASELINE configs[4]: every rank
    builds an IVF over its own rows; the exchange is the same all_gather of B*k keys as for the flat search).  The masked
    forms answer a shard-local `allow` under the same `nprobe` lists (search_ivf_keys(..., allow=))."""

    def __init__(self, index: DeviceKnnIndex, nprobe: int):
        _require_cosine(index)
        self.index, self.nprobe = index, int(nprobe)

    @property
    def space(self) -> str:
        """the index's space: ShardedSearcher's merges write that space's distances"""
        return getattr(self.index, "space", "cosine")

    def count(self) -> int:
        return self.index.count()

    def search_keys(self, queries, k: int, row_base: int = 0):
        return search_ivf_keys(self.index, queries, k, self.nprobe, row_base)

    def search_keys_masked(self, queries, allow, k: int, row_base: int = 0):
        return self.index.ivf_search_keys_masked(queries, allow, k, self.nprobe, row_base)

    def search_keys_masked_dev(self, queries, allow_bits, k: int, row_base: int = 0):
        return self.index.ivf_search_keys_masked_dev(queries, allow_bits, k, self.nprobe, row_base)

    def match_documents(self, needle: bytes):
        return self.index.match_documents(needle)

    def match_documents_dfa(self, dfa):
        return self.index.match_documents_dfa(dfa)

    def slice_mask(self, global_bits, global_rows: int, row_base: int):
        return self.index.slice_mask(global_bits, global_rows, row_base)
