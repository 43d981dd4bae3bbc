"""
Row-sharded search across the GPUs of one node: one process per GPU, torch.distributed
(backend "nccl" = RCCL over xGMI on ROCm; "gloo" in the CPU tests).

The reference has no distributed code at all; this is the build's own
multi-GPU shape for the k-NN behind collection.query (store.py:314-316):

  * the corpus is cut into contiguous row blocks, rank g owns rows
    [g*ceil(N/G), min(N, (g+1)*ceil(N/G))) — no rank ever sees another rank's rows;
  * every rank receives the same B x d query block and runs the single-GPU search on its
    shard, emitting B x k packed keys that already carry GLOBAL row ids
    (key = ord(score) << 32 | ~global_row, codd_knn_search_keys);
  * ONE all_gather of B*k u64 per rank (80 B at B=1, 20 KB at B=256, k=10 — latency-bound,
    nowhere near the 153 GB/s of an xGMI link) gives every rank all partials;
  * an integer top-k of the G*k keys per query (codd_knn_merge_keys) finishes on every rank;
    ties resolve exactly as on one GPU because the order lives in the keys.
"""

from __future__ import annotations

from typing import Any, Callable, Optional


def shard_bounds(n_total: int, world_size: int, rank: int) -> tuple[int, int]:
    """[begin, end) of the rows rank `rank` owns."""
    if world_size < 1 or not (0 <= rank < world_size):
        raise ValueError("bad world_size / rank")
    per = -(-int(n_total) // world_size)
    begin = min(n_total, rank * per)
    return begin, min(n_total, begin + per)


def _is_device_words(allow) -> bool:
    import torch

    return isinstance(allow, torch.Tensor) and allow.is_cuda


class PendingSearch:
    """Handle of ShardedSearcher.search_async: the results live on a side stream until `.result()`."""

    def __init__(self, stream: Any, out: tuple):
        self._stream, self._out = stream, out

    def result(self) -> tuple:
        if self._stream is not None:
            import torch

            cur = torch.cuda.current_stream(self._out[0].device)
            cur.wait_stream(self._stream)
            for t in self._out:
                t.record_stream(cur)
            self._stream = None
        return self._out


class ShardedSearcher:
    """Glue between a shard-local engine and the process group.

    engine.search_keys(queries, k, row_base) -> int64 tensor [B,k] of packed keys on the
    engine's device; merge(keys [B,m], k) -> (keys, dist, rows).  Products pass a
    DeviceKnnIndex and leave `merge` unset (HIP merge kernel, which writes the distances of the
    engine's `space`: cosine where the engine names none); the gloo tests pass the checker engine
    and its merge.

    Deletes need nothing here: tombstones are shard-local (engine.delete) and the keys carry
    global rows.  Compacting ONE shard (engine.compact) changes its local slots, so the
    caller's row_base bookkeeping must follow: a global row is row_base + local slot, and
    whatever maps global rows to records has to be renumbered for that shard.

    Masks are shard-local too: `allow=` names row slots of this rank's engine (a document filter over the shard's own
    documents is engine.match_documents' words as they are); a mask compiled once over global rows is passed with
    allow_global=True and every rank slices out rows [row_base, row_base + engine.count()) itself.
    """

    def __init__(self, engine: Any, row_base: int, group: Optional[Any] = None,
                 merge: Optional[Callable[[Any, int], tuple]] = None, always_gather: bool = False):
        import torch.distributed as dist

        from .native import check_row_base

        self.engine = engine
        self.always_gather = always_gather  # exercise the collective even with one rank (rehearsals)
        self.row_base = check_row_base(row_base, 0)  # (the sign and >= 2^32 here; row_base + count by the engine, per search)
        self.group = group
        self.world_size = dist.get_world_size(group) if dist.is_initialized() else 1
        self.rank = dist.get_rank(group) if dist.is_initialized() else 0
        self._merge_gathered = None  # [G*B,k] as gathered -> results, without a transpose pass (HIP engines only)
        if merge is None:
            from .knn_index import merge_keys as hip_merge
            from .knn_index import merge_shards as hip_merge_shards

            # the keys merge alike under every space; the distance written beside them follows the engine's
            space = getattr(engine, "space", "cosine")
            merge = lambda keys, k: hip_merge(keys, k, space=space)  # noqa: E731
            self._merge_gathered = lambda gathered, world, k: hip_merge_shards(gathered, world, k, space=space)  # noqa: E731
        self._merge = merge
        self._streams: list = []
        self._turn = 0

    def _local_allow(self, allow):
        """The shard's own mask out of one over GLOBAL rows: rows [row_base, row_base + engine.count()).  A device mask (int32
        CUDA words) is cut by the slicing kernel on its device; a host mask (bool array over the global rows, or packed uint32
        words) with numpy.  Global rows past the mask's end are not allowed."""
        import numpy as np

        count = int(self.engine.count())
        if _is_device_words(allow):
            return self.engine.slice_mask(allow, 32 * int(allow.shape[0]), self.row_base)
        a = np.asarray(allow)
        if a.ndim != 1 or a.dtype not in (np.bool_, np.uint32):
            raise ValueError(f"allow must be a bool array, packed uint32 words or int32 CUDA words, got {a.dtype} {a.shape}")
        bits = a if a.dtype == np.bool_ else np.unpackbits(np.ascontiguousarray(a).view(np.uint8), bitorder="little").astype(bool)
        local = np.zeros(count, dtype=bool)
        have = bits[self.row_base : self.row_base + count]
        local[: have.shape[0]] = have
        return local

    def search_keys_local(self, queries, k: int, scopes=None, allow=None, allow_global: bool = False):
        if allow is not None:
            if scopes is not None:
                raise ValueError("scopes and allow cannot be combined: fold the scope into the mask")
            if allow_global:
                allow = self._local_allow(allow)
            if _is_device_words(allow):
                return self.engine.search_keys_masked_dev(queries, allow, k, self.row_base)
            return self.engine.search_keys_masked(queries, allow, k, self.row_base)
        if scopes is None:
            return self.engine.search_keys(queries, k, self.row_base)
        return self.engine.search_keys_scoped(queries, scopes, k, self.row_base)

    def search_async(self, queries, k: int, depth: int = 2, scopes=None, allow=None, allow_global: bool = False) -> "PendingSearch":
        """Issue one batch on a side stream and return at once; `.result()` makes the caller's stream wait for it.

        Consecutive batches go to `depth` alternating HIP streams, so the small kernels, the all_gather and the merge
        of batch i overlap the filter kernel of batch i+1 (the engine keeps one workspace per stream).  Every rank must
        issue its batches in the same order, as with `search`.  With a host engine (gloo tests) it runs synchronously.
        A device `allow` must have been written on the caller's current stream (the side stream waits for that one).
        """
        import torch

        dev = getattr(queries, "device", None)
        if not (isinstance(queries, torch.Tensor) and dev is not None and dev.type == "cuda"):
            return PendingSearch(None, self.search(queries, k, scopes, allow, allow_global))
        if len(self._streams) != depth:
            self._streams = [torch.cuda.Stream(device=dev) for _ in range(depth)]
            self._turn = 0
        side = self._streams[self._turn]
        self._turn = (self._turn + 1) % depth
        side.wait_stream(torch.cuda.current_stream(dev))  # the queries are ready
        with torch.cuda.stream(side):
            out = self.search(queries, k, scopes, allow, allow_global)
        queries.record_stream(side)
        if _is_device_words(allow):
            allow.record_stream(side)
        return PendingSearch(side, out)

    def search(self, queries, k: int, scopes=None, allow=None, allow_global: bool = False):
        """(dist [B,k], global rows [B,k]) — identical on every rank.  `scopes` ([B] scope labels, the same on every
        rank and the same labelling on every shard) restricts each query to its scope: the shards answer with
        search_keys_scoped, the merge is the same.

        `allow` restricts the whole batch to the rows a mask names (`where=` / `where_document=`): the shard-LOCAL mask, as
        a host bool array of engine.count() entries or packed uint32 words (engine.search_keys_masked), or as int32 CUDA
        words, e.g. what engine.match_documents returned (engine.search_keys_masked_dev).  With allow_global=True it is one
        mask over the GLOBAL rows, the same on every rank, and each rank cuts its own rows out first (on the device for
        device words).  `scopes` and `allow` together raise ValueError.  A rank whose mask allows nothing still joins the
        collective, with the all-empty keys its engine returns."""
        import torch
        import torch.distributed as dist

        local = self.search_keys_local(queries, k, scopes, allow, allow_global)  # [B,k] int64
        if self.world_size == 1 and not self.always_gather:
            _, d, r = self._merge(local, k)
            return d, r
        B = local.shape[0]
        # rank-major concatenation along dim 0 (the layout both RCCL and gloo accept)
        gathered = torch.empty((self.world_size * B, k), dtype=torch.int64, device=local.device)
        dist.all_gather_into_tensor(gathered, local.contiguous(), group=self.group)
        if self._merge_gathered is not None:
            _, d, r = self._merge_gathered(gathered, self.world_size, k)
            return d, r
        merged_in = gathered.view(self.world_size, B, k).permute(1, 0, 2).reshape(B, self.world_size * k).contiguous()
        _, d, r = self._merge(merged_in, k)
        return d, r
