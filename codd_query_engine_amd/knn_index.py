"""
DeviceKnnIndex — thin Python owner of one `codd_knn_index` (include/codd_knn.h).

torch is plumbing here: it provides device buffers, the current HIP stream and (in
sharded.py) torch.distributed.  All arithmetic happens inside libcodd_knn.so.
"""

from __future__ import annotations

import ctypes

import numpy as np

from . import native


def _torch():
    import torch

    return torch


def require_gpu(device: str = "cuda:0"):
    torch = _torch()
    if not torch.cuda.is_available():
        raise native.NativeLibraryError(
            "no GPU visible to this process: the k-NN path has no CPU fallback "
            "(tests inject their own engine; products need an MI355X)"
        )
    return torch.device(device)


class DeviceKnnIndex:
    """Device-resident row store with exact top-k search: L2-normalised rows under cosine (the default `space`), rows as given
    under ChromaDB's other two spaces, "ip" (distance 1 - <q, c>) and "l2" (squared distance).  Every search method's distances
    follow the space; an ip or l2 index has no approx_scores and takes IVF with its "space_ivf" option on (§22).

    Engine protocol consumed by knn_client.Collection:
        count() / upsert(slots, vecs) / search(queries, k) -> (dist, rows) as numpy;
        optionally set_scopes / search_scoped (`where=` by namespace), search_masked (any other `where=`), set_documents /
        match_documents / match_documents_dfa / search_masked_dev (`where_document=` on the device), set_column / drop_columns /
        eval_where (`where=` on the device, opt-in: DESIGN.md §26) and delete / live_count / compact (`Collection.delete`).
    The ivf_search_*masked* methods are the same masks under an installed IVF layout (ivf.py), slice_mask cuts a shard's words
    out of a mask over global rows (sharded.py).
    """

    def __init__(self, dim: int, dtype: str = "f32", device: str = "cuda:0", space: str = "cosine"):
        if dtype not in native.DTYPE_CODES:
            raise ValueError(f"dtype must be one of {sorted(native.DTYPE_CODES)}")
        metric = native.metric_code(space)
        self.space = space
        self._lib = native.load()
        self.device = require_gpu(device)
        self.dim = int(dim)
        self.dtype = dtype
        self._dev_index = self.device.index if self.device.index is not None else _torch().cuda.current_device()
        h = ctypes.c_void_p()
        native.check(
            self._lib.codd_knn_create(ctypes.byref(h), self._dev_index, self.dim, native.DTYPE_CODES[dtype], metric),
            "codd_knn_create",
        )
        self._h = h
        pd = ctypes.c_int()
        native.check(self._lib.codd_knn_dim(self._h, None, ctypes.byref(pd), None), "codd_knn_dim")
        self.padded_dim = pd.value

    # ------------------------------------------------------------------ lifecycle
    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.codd_knn_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):  # best effort
        try:
            self.close()
        except Exception:
            pass

    def _stream(self) -> ctypes.c_void_p:
        return ctypes.c_void_p(_torch().cuda.current_stream(self.device).cuda_stream)

    # ------------------------------------------------------------------ ingest
    def count(self) -> int:
        out = ctypes.c_int64()
        native.check(self._lib.codd_knn_count(self._h, ctypes.byref(out)), "codd_knn_count")
        return out.value

    def reserve(self, rows: int) -> None:
        native.check(self._lib.codd_knn_reserve(self._h, int(rows)), "codd_knn_reserve")

    def upsert(self, slots, vecs, normalize: bool = True) -> None:
        """Host vectors [n, dim] fp32 into the given row slots (append or overwrite)."""
        slots = np.ascontiguousarray(slots, dtype=np.int64)
        vecs = np.ascontiguousarray(vecs, dtype=np.float32)
        if vecs.ndim != 2 or vecs.shape[1] != self.dim or slots.shape != (vecs.shape[0],):
            raise ValueError(f"expected vecs [n,{self.dim}] and slots [n], got {vecs.shape} / {slots.shape}")
        native.check(
            self._lib.codd_knn_upsert_host(self._h, slots.ctypes.data, vecs.ctypes.data, vecs.shape[0], int(bool(normalize))),
            "codd_knn_upsert_host",
        )

    def upsert_device(self, first_slot: int, vecs, normalize: bool = True) -> None:
        """Device tensor [n, dim] fp32 (contiguous) into slots [first_slot, first_slot+n)."""
        torch = _torch()
        if not (isinstance(vecs, torch.Tensor) and vecs.is_cuda and vecs.dtype == torch.float32 and vecs.is_contiguous()):
            raise ValueError("upsert_device wants a contiguous fp32 CUDA tensor")
        if vecs.dim() != 2 or vecs.shape[1] != self.dim:
            raise ValueError(f"expected [n,{self.dim}], got {tuple(vecs.shape)}")
        native.check(
            self._lib.codd_knn_upsert_device(self._h, int(first_slot), vecs.data_ptr(), vecs.shape[0], int(bool(normalize)), self._stream()),
            "codd_knn_upsert_device",
        )

    def read_rows(self, first: int = 0, n: int | None = None) -> np.ndarray:
        """Stored rows (normalised, padded) as fp32 or uint16 bit patterns."""
        n = self.count() - first if n is None else n
        out = np.empty((n, self.padded_dim), dtype=np.float32 if self.dtype == "f32" else np.uint16)
        native.check(self._lib.codd_knn_read_rows(self._h, int(first), int(n), out.ctypes.data), "codd_knn_read_rows")
        return out

    def load_rows(self, rows: np.ndarray, first_slot: int = 0) -> None:
        """Stored rows as read_rows() returned them (persisted index) into slots [first_slot, ...)."""
        want = np.float32 if self.dtype == "f32" else np.uint16
        rows = np.ascontiguousarray(rows, dtype=want)
        if rows.ndim != 2 or rows.shape[1] != self.padded_dim:
            raise ValueError(f"expected stored rows [n,{self.padded_dim}], got {rows.shape}")
        native.check(self._lib.codd_knn_load_rows(self._h, int(first_slot), rows.ctypes.data, rows.shape[0]), "codd_knn_load_rows")

    # ------------------------------------------------------------------ search
    def _queries_tensor(self, queries):
        torch = _torch()
        if isinstance(queries, torch.Tensor):
            q = queries.to(device=self.device, dtype=torch.float32).contiguous()
        else:
            q = torch.from_numpy(np.ascontiguousarray(queries, dtype=np.float32)).to(self.device)
        if q.dim() != 2 or q.shape[1] != self.dim:
            raise ValueError(f"expected queries [B,{self.dim}], got {tuple(q.shape)}")
        return q

    def search_tensors(self, queries, k: int):
        """Device in, device out: (dist fp32 [B,k] ascending, rows int64 [B,k], -1 padded)."""
        torch = _torch()
        q = self._queries_tensor(queries)
        B = q.shape[0]
        dist = torch.empty((B, k), dtype=torch.float32, device=self.device)
        rows = torch.empty((B, k), dtype=torch.int64, device=self.device)
        native.check(
            self._lib.codd_knn_search(self._h, q.data_ptr(), B, int(k), dist.data_ptr(), rows.data_ptr(), self._stream()),
            "codd_knn_search",
        )
        return dist, rows

    def search(self, queries, k: int):
        """numpy in, numpy out (the façade's path)."""
        dist, rows = self.search_tensors(queries, k)
        return dist.cpu().numpy(), rows.cpu().numpy()

    def search_keys(self, queries, k: int, row_base: int = 0):
        """Shard-local packed keys [B,k] (u64 bit patterns in an int64 tensor), descending."""
        row_base = native.check_row_base(row_base, self.count())
        torch = _torch()
        q = self._queries_tensor(queries)
        B = q.shape[0]
        keys = torch.empty((B, k), dtype=torch.int64, device=self.device)
        native.check(
            self._lib.codd_knn_search_keys(self._h, q.data_ptr(), B, int(k), row_base, keys.data_ptr(), self._stream()),
            "codd_knn_search_keys",
        )
        return keys

    # ------------------------------------------------------------------ scopes
    def set_scopes(self, slots, scopes) -> None:
        """Scope label (0 = none, <= native.MAX_SCOPE) of the given row slots; a slot keeps it when its vector is overwritten."""
        slots = np.ascontiguousarray(slots, dtype=np.int64)
        scopes = np.ascontiguousarray(scopes, dtype=np.uint32)
        if slots.ndim != 1 or scopes.shape != slots.shape:
            raise ValueError(f"expected slots [n] and scopes [n], got {slots.shape} / {scopes.shape}")
        native.check(self._lib.codd_knn_set_scopes_host(self._h, slots.ctypes.data, scopes.ctypes.data, slots.shape[0]), "codd_knn_set_scopes_host")

    # ------------------------------------------------------------------ deletes
    def delete(self, slots) -> None:
        """Tombstone the given row slots (each < count(); repeats and already-dead slots are no-ops).  No search returns a dead
        row; the slot stays dead, and cannot be written, until compact()."""
        slots = np.ascontiguousarray(slots, dtype=np.int64)
        if slots.ndim != 1:
            raise ValueError(f"expected slots [n], got {slots.shape}")
        native.check(self._lib.codd_knn_delete_host(self._h, slots.ctypes.data, slots.shape[0]), "codd_knn_delete_host")

    def live_count(self) -> int:
        """Row slots in use minus the dead ones (count() stays highest written slot + 1)."""
        out = ctypes.c_int64()
        native.check(self._lib.codd_knn_live_count(self._h, ctypes.byref(out)), "codd_knn_live_count")
        return out.value

    def compact(self) -> int:
        """Move the live rows to slots 0 .. live-1 in slot order (scopes move along) and return the new count()."""
        out = ctypes.c_int64()
        native.check(self._lib.codd_knn_compact(self._h, ctypes.byref(out)), "codd_knn_compact")
        return out.value

    def _scopes_tensor(self, scopes, B: int):
        torch = _torch()
        if isinstance(scopes, torch.Tensor):
            s = scopes.to(device=self.device, dtype=torch.int32).contiguous()  # (uint32 bit patterns: labels are below 2^20)
        else:
            s = torch.from_numpy(np.ascontiguousarray(scopes, dtype=np.uint32).view(np.int32)).to(self.device)
        if s.dim() != 1 or s.shape[0] != B:
            raise ValueError(f"expected scopes [{B}], got {tuple(s.shape)}")
        return s

    def search_scoped_tensors(self, queries, scopes, k: int):
        """search_tensors among the rows whose scope equals the query's (scope 0: every row)."""
        torch = _torch()
        q = self._queries_tensor(queries)
        B = q.shape[0]
        s = self._scopes_tensor(scopes, B)
        dist = torch.empty((B, k), dtype=torch.float32, device=self.device)
        rows = torch.empty((B, k), dtype=torch.int64, device=self.device)
        native.check(
            self._lib.codd_knn_search_scoped(self._h, q.data_ptr(), s.data_ptr(), B, int(k), 0, None, dist.data_ptr(), rows.data_ptr(), self._stream()),
            "codd_knn_search_scoped",
        )
        return dist, rows

    def search_scoped(self, queries, scopes, k: int):
        """numpy in, numpy out (the façade's path for `where=`)."""
        dist, rows = self.search_scoped_tensors(queries, scopes, k)
        return dist.cpu().numpy(), rows.cpu().numpy()

    def search_keys_scoped(self, queries, scopes, k: int, row_base: int = 0):
        """search_keys among the rows whose scope equals the query's."""
        row_base = native.check_row_base(row_base, self.count())
        torch = _torch()
        q = self._queries_tensor(queries)
        B = q.shape[0]
        s = self._scopes_tensor(scopes, B)
        keys = torch.empty((B, k), dtype=torch.int64, device=self.device)
        native.check(
            self._lib.codd_knn_search_scoped(self._h, q.data_ptr(), s.data_ptr(), B, int(k), row_base, keys.data_ptr(), None, None, self._stream()),
            "codd_knn_search_scoped",
        )
        return keys

    # ------------------------------------------------------------------ masks
    def _allow_words(self, allow) -> np.ndarray:
        """The allow mask as packed uint32 words: a bool array of length count() (bit r & 31 of word r >> 5 = row slot r), or the
        words themselves (uint32, ceil(count() / 32) of them)."""
        a = np.asarray(allow)
        if a.ndim != 1:
            raise ValueError(f"expected a 1-d allow mask, got shape {a.shape}")
        if a.dtype == np.bool_:
            n = self.count()
            if a.shape[0] != n:
                raise ValueError(f"expected a bool mask of length count() = {n}, got {a.shape[0]}")
            packed = np.packbits(a, bitorder="little")
            words = np.zeros((n + 31) // 32 * 4, dtype=np.uint8)
            words[: packed.shape[0]] = packed
            return words.view("<u4")
        if a.dtype != np.uint32:
            raise ValueError(f"allow must be a bool array or packed uint32 words, got dtype {a.dtype}")
        return np.ascontiguousarray(a)

    def _search_masked(self, queries, allow, k: int, row_base: int, want_keys: bool):
        row_base = native.check_row_base(row_base, self.count())
        torch = _torch()
        q = self._queries_tensor(queries)
        B = q.shape[0]
        words = self._allow_words(allow)
        keys = torch.empty((B, k), dtype=torch.int64, device=self.device) if want_keys else None
        dist = None if want_keys else torch.empty((B, k), dtype=torch.float32, device=self.device)
        rows = None if want_keys else torch.empty((B, k), dtype=torch.int64, device=self.device)
        native.check(
            self._lib.codd_knn_search_masked(self._h, q.data_ptr(), B, int(k), words.ctypes.data, words.shape[0], row_base,
                                             keys.data_ptr() if want_keys else None, None if want_keys else dist.data_ptr(),
                                             None if want_keys else rows.data_ptr(), self._stream()),
            "codd_knn_search_masked",
        )
        return keys, dist, rows

    def search_masked_tensors(self, queries, allow, k: int):
        """search_tensors among the rows `allow` names (one mask for the whole batch) that are not deleted."""
        _, dist, rows = self._search_masked(queries, allow, k, 0, False)
        return dist, rows

    def search_masked(self, queries, allow, k: int):
        """numpy in, numpy out (the façade's path for a general `where=`)."""
        dist, rows = self.search_masked_tensors(queries, allow, k)
        return dist.cpu().numpy(), rows.cpu().numpy()

    def search_keys_masked(self, queries, allow, k: int, row_base: int = 0):
        """search_keys among the rows `allow` names."""
        return self._search_masked(queries, allow, k, row_base, True)[0]

    # ------------------------------------------------------------------ documents (where_document)
    def set_documents(self, documents) -> None:
        """The document of every row slot, as bytes (None = no document, matched as empty): count() entries, none holding a 0x00
        byte.  Replaces the engine's whole snapshot; it goes stale on the next upsert / load_rows / compact."""
        docs = [b"" if d is None else bytes(d) for d in documents]
        offsets = np.zeros(len(docs) + 1, dtype=np.int64)
        if docs:
            np.cumsum([len(d) for d in docs], out=offsets[1:])
        blob = np.frombuffer(b"".join(docs), dtype=np.uint8)
        native.check(
            self._lib.codd_knn_set_documents_host(self._h, blob.ctypes.data if blob.size else None, offsets.ctypes.data, len(docs)),
            "codd_knn_set_documents_host",
        )

    def match_documents(self, needle: bytes):
        """The row slots whose document contains `needle` (1 .. native.MAX_NEEDLE bytes, no 0x00) as a byte substring: packed
        words, bit r & 31 of word r >> 5 = row slot r, in an int32 CUDA tensor of ceil(count() / 32) words (uint32 bit patterns)."""
        torch = _torch()
        needle = bytes(needle)
        nwords = (self.count() + 31) // 32
        bits = torch.empty((nwords,), dtype=torch.int32, device=self.device)
        native.check(
            self._lib.codd_knn_match_documents(self._h, needle, len(needle), bits.data_ptr() if nwords else None, nwords, self._stream()),
            "codd_knn_match_documents",
        )
        return bits

    def match_documents_dfa(self, dfa):
        """The row slots whose document a byte DFA accepts (regex_dfa.ByteDfa, or anything with its class_of / next / nstates /
        nclasses / start / accept): the walk over the document's bytes and one 0x00 ends in `accept`.  The words match_documents
        returns.  The engine checks the table before it uploads it; a malformed one is EINVAL."""
        torch = _torch()
        class_of, table, nstates, nclasses = bytes(dfa.class_of), bytes(dfa.next), int(dfa.nstates), int(dfa.nclasses)
        # (the library reads 256 and nstates * nclasses host bytes before it can check anything else)
        if len(class_of) != 256 or nstates < 1 or nclasses < 1 or len(table) != nstates * nclasses:
            raise ValueError(f"malformed DFA: class_of holds {len(class_of)} bytes (256 wanted), next {len(table)} for {nstates} x {nclasses} states x classes")
        nwords = (self.count() + 31) // 32
        bits = torch.empty((nwords,), dtype=torch.int32, device=self.device)
        native.check(
            self._lib.codd_knn_match_documents_dfa(self._h, class_of, table, nstates, nclasses, int(dfa.start),
                                                   int(dfa.accept), bits.data_ptr() if nwords else None, nwords, self._stream()),
            "codd_knn_match_documents_dfa",
        )
        return bits

    # ------------------------------------------------------------------ metadata columns (where= on the device)
    def set_column(self, column: int, slots, tags, cells) -> None:
        """Tag (uint8: 0 absent, 1 bool, 2 number, 3 str) and cell (uint64) of the given row slots of metadata column `column`
        (< native.MAX_COLUMNS); slots None: the rows 0 .. len(tags) - 1, a full upload.  The column lives beside the rows: it grows
        with them, compact() moves it, load_rows drops it (where_columns.py encodes the cells)."""
        tags = np.ascontiguousarray(tags, dtype=np.uint8)
        cells = np.ascontiguousarray(cells, dtype=np.uint64)
        if tags.ndim != 1 or cells.shape != tags.shape:
            raise ValueError(f"expected tags [n] and cells [n], got {tags.shape} / {cells.shape}")
        if slots is not None:
            slots = np.ascontiguousarray(slots, dtype=np.int64)
            if slots.shape != tags.shape:
                raise ValueError(f"expected slots [n] like the tags, got {slots.shape} / {tags.shape}")
        native.check(self._lib.codd_knn_set_column_host(self._h, int(column), None if slots is None else slots.ctypes.data, tags.ctypes.data,
                                                        cells.ctypes.data, tags.shape[0]), "codd_knn_set_column_host")

    def drop_columns(self) -> None:
        """Forget every metadata column."""
        native.check(self._lib.codd_knn_drop_columns(self._h), "codd_knn_drop_columns")

    def eval_where(self, program):
        """The live row slots a predicate program accepts (where_columns.compile_where's, or anything native.where_program takes):
        packed words in match_documents' form, an int32 CUDA tensor of ceil(count() / 32) words — what search_masked_dev,
        ivf_search_masked_dev_tensors, slice_mask and ShardedSearcher.search(allow=) take.  The engine checks the program on the
        host before it launches anything; a malformed one is EINVAL.  Asynchronous on the current stream."""
        torch = _torch()
        prog = native.where_program(program)
        nwords = (self.count() + 31) // 32
        bits = torch.empty((nwords,), dtype=torch.int32, device=self.device)
        native.check(self._lib.codd_knn_eval_where(self._h, ctypes.byref(prog), bits.data_ptr() if nwords else None, nwords, self._stream()),
                     "codd_knn_eval_where")
        return bits

    def _allow_words_tensor(self, allow_bits):
        torch = _torch()
        if not (isinstance(allow_bits, torch.Tensor) and allow_bits.is_cuda and allow_bits.dtype == torch.int32 and allow_bits.dim() == 1):
            raise ValueError("expected the allow mask as a 1-d int32 CUDA tensor of packed words (match_documents' form)")
        return allow_bits.to(self.device).contiguous()

    def _search_masked_dev(self, queries, allow_bits, k: int, row_base: int, want_keys: bool):
        row_base = native.check_row_base(row_base, self.count())
        torch = _torch()
        q = self._queries_tensor(queries)
        B = q.shape[0]
        words = self._allow_words_tensor(allow_bits)
        keys = torch.empty((B, k), dtype=torch.int64, device=self.device) if want_keys else None
        dist = None if want_keys else torch.empty((B, k), dtype=torch.float32, device=self.device)
        rows = None if want_keys else torch.empty((B, k), dtype=torch.int64, device=self.device)
        native.check(
            self._lib.codd_knn_search_masked_dev(self._h, q.data_ptr(), B, int(k), words.data_ptr() if words.shape[0] else None, words.shape[0],
                                                 row_base, keys.data_ptr() if want_keys else None, None if want_keys else dist.data_ptr(),
                                                 None if want_keys else rows.data_ptr(), self._stream()),
            "codd_knn_search_masked_dev",
        )
        return keys, dist, rows

    def search_masked_dev_tensors(self, queries, allow_bits, k: int):
        """search_masked_tensors under a mask that is on the device already: packed words as match_documents returns them."""
        _, dist, rows = self._search_masked_dev(queries, allow_bits, k, 0, False)
        return dist, rows

    def search_masked_dev(self, queries, allow_bits, k: int):
        """numpy out (the façade's path for `where_document=`)."""
        dist, rows = self.search_masked_dev_tensors(queries, allow_bits, k)
        return dist.cpu().numpy(), rows.cpu().numpy()

    def search_keys_masked_dev(self, queries, allow_bits, k: int, row_base: int = 0):
        """search_keys among the rows the device mask names."""
        return self._search_masked_dev(queries, allow_bits, k, row_base, True)[0]

    # ------------------------------------------------------------------ masks under an IVF layout
    def _ivf_search_masked(self, queries, allow, k: int, nprobe: int, row_base: int, want_keys: bool, on_device: bool):
        row_base = native.check_row_base(row_base, self.count())
        torch = _torch()
        q = self._queries_tensor(queries)
        B = q.shape[0]
        if on_device:
            words = self._allow_words_tensor(allow)
            ptr, fn, name = words.data_ptr() if words.shape[0] else None, self._lib.codd_knn_ivf_search_masked_dev, "codd_knn_ivf_search_masked_dev"
        else:
            words = self._allow_words(allow)
            ptr, fn, name = words.ctypes.data, self._lib.codd_knn_ivf_search_masked, "codd_knn_ivf_search_masked"
        keys = torch.empty((B, k), dtype=torch.int64, device=self.device) if want_keys else None
        dist = None if want_keys else torch.empty((B, k), dtype=torch.float32, device=self.device)
        rows = None if want_keys else torch.empty((B, k), dtype=torch.int64, device=self.device)
        native.check(
            fn(self._h, q.data_ptr(), B, int(k), int(nprobe), ptr, words.shape[0], row_base, keys.data_ptr() if want_keys else None,
               None if want_keys else dist.data_ptr(), None if want_keys else rows.data_ptr(), self._stream()),
            name,
        )
        return keys, dist, rows

    def ivf_search_masked_tensors(self, queries, allow, k: int, nprobe: int, row_base: int = 0):
        """ivf.search_ivf among the rows `allow` names (host mask: bool array or packed uint32 words) that are not deleted: the
        `nprobe` lists are chosen as without a mask, the top-k is exact among the allowed live rows of those lists."""
        _, dist, rows = self._ivf_search_masked(queries, allow, k, nprobe, row_base, False, False)
        return dist, rows

    def ivf_search_keys_masked(self, queries, allow, k: int, nprobe: int, row_base: int = 0):
        """ivf.search_ivf_keys among the rows the host mask names."""
        return self._ivf_search_masked(queries, allow, k, nprobe, row_base, True, False)[0]

    def ivf_search_masked_dev_tensors(self, queries, allow_bits, k: int, nprobe: int, row_base: int = 0):
        """ivf_search_masked_tensors under a mask that is on the device already (match_documents' form).  Nothing is read back:
        the call is asynchronous on the current stream."""
        _, dist, rows = self._ivf_search_masked(queries, allow_bits, k, nprobe, row_base, False, True)
        return dist, rows

    def ivf_search_keys_masked_dev(self, queries, allow_bits, k: int, nprobe: int, row_base: int = 0):
        """ivf.search_ivf_keys among the rows the device mask names."""
        return self._ivf_search_masked(queries, allow_bits, k, nprobe, row_base, True, True)[0]

    def ivf_refresh(self) -> None:
        """Fold the pending rows of an IVF layout that follows writes (option "ivf_follow", ivf.follow_writes) into the layout:
        codd_knn_ivf_refresh on the current stream.  A no-op with nothing pending; NativeLibraryError with the option off, or
        with no layout or a stale one."""
        native.check(self._lib.codd_knn_ivf_refresh(self._h, self._stream()), "codd_knn_ivf_refresh")

    def slice_mask(self, global_bits, global_rows: int, row_base: int):
        """This shard's words of a mask over GLOBAL rows: bit r of the result = global bit row_base + r, for r < count()."""
        return slice_mask(global_bits, global_rows, row_base, self.count(), self.device)

    def merge_keys(self, keys, k: int):
        """Top-k of [B,m] packed keys -> (keys [B,k], dist [B,k], rows [B,k]) on device; distances by this index's space."""
        return merge_keys(keys, k, self.device, space=self.space)

    def approx_scores(self, queries):
        """Raw approximate scores of the MFMA filter: [256, count] fp32 tensor (diagnostics).  Cosine, or an ip / l2 index
        with its int8 filter leg on ("space_filter", at most 32 queries: the values that leg filters with)."""
        if self.space != "cosine" and not self.stat("space_filter"):
            raise native.NativeLibraryError(f"approx_scores: the MFMA filters exist for the cosine space only, this index is {self.space!r}")
        torch = _torch()
        q = self._queries_tensor(queries)
        out = torch.zeros((256, self.count()), dtype=torch.float32, device=self.device)
        native.check(
            self._lib.codd_knn_approx_scores(self._h, q.data_ptr(), q.shape[0], out.data_ptr(), self._stream()),
            "codd_knn_approx_scores",
        )
        return out

    def filter_slack(self, queries):
        """eps(q) of the next int8 filter pass for up to 256 queries: [B] fp32 tensor (diagnostics; codd_knn_filter_slack)."""
        torch = _torch()
        q = self._queries_tensor(queries)
        out = torch.zeros((q.shape[0],), dtype=torch.float32, device=self.device)
        native.check(
            self._lib.codd_knn_filter_slack(self._h, q.data_ptr(), q.shape[0], out.data_ptr(), self._stream()),
            "codd_knn_filter_slack",
        )
        return out

    def last_pass(self, keys_per_query: int | None = None, want_bmeta: bool = True) -> dict:
        """What the last filter pass on this stream's workspace left behind (diagnostics; codd_knn_debug_last_pass): a dict of
        the program and shape fields of codd_knn_last_pass ("family" as its name), "flags", "fb_count", "sweep" (1: the index's last pass ran the sweep form of the static int8 tile program), and numpy arrays "thr" [256],
        "thr0" [256], "qmeta" [1024] (int8 passes, else None), "hit_counts" [256], "fb_list" [256], "keys" (a list of 256 u64
        arrays: each query's first min(counter, hit_cap, keys_per_query) candidate keys), "bucket_max" [256, sample_tiles] and
        "bmeta" [ceil(n / 32), 2] (int8 passes, else None).  keys_per_query: None = the largest list the pass left."""
        info = native.LastPassInfo()
        ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
        thr = np.zeros(512, dtype=np.float32)
        qmeta = np.zeros(1024, dtype=np.float32)
        counts = np.zeros(256, dtype=np.uint32)
        fb_list = np.zeros(256, dtype=np.uint32)
        call = self._lib.codd_knn_debug_last_pass
        native.check(call(self._h, self._stream(), ctypes.byref(info), ptr(thr), ptr(qmeta), ptr(counts), ptr(fb_list), None, 0, None, 0, None, 0),
                     "codd_knn_debug_last_pass")
        kept = np.minimum(counts.astype(np.int64), info.hit_cap)
        per_q = int(kept.max()) if keys_per_query is None else int(keys_per_query)
        kept = np.minimum(kept, per_q)
        keys = np.zeros((256, max(per_q, 1)), dtype=np.uint64)
        buckets = np.zeros((256, info.sample_tiles), dtype=np.uint64)
        nblocks = (info.n + 31) // 32 if (want_bmeta and info.el) else 0
        bmeta = np.zeros((max(nblocks, 1), 2), dtype=np.float32)
        native.check(call(self._h, self._stream(), None, None, None, None, None, ptr(keys), per_q, ptr(buckets), buckets.size, ptr(bmeta) if nblocks else None, nblocks),
                     "codd_knn_debug_last_pass")
        out = {name: getattr(info, name) for name, _ in native.LastPassInfo._fields_ if name not in ("flags", "family")}
        out["family"] = native.FILTER_FAMILIES[info.family]
        out["sweep"] = int(self.stat("last_sweep"))   # the filter launches ran i8_sweep_kernel (the index's last pass: the struct has no room for it)
        out["flags"] = list(info.flags)
        out.update(thr=thr[:256].copy(), thr0=thr[256:].copy(), qmeta=qmeta if info.el else None, hit_counts=counts, fb_list=fb_list,
                   keys=[keys[q, : kept[q]].copy() for q in range(256)], bucket_max=buckets, bmeta=bmeta[:nblocks] if nblocks else None)
        return out

    # ------------------------------------------------------------------ knobs
    def set_option(self, key: str, value: int) -> None:
        native.check(self._lib.codd_knn_set_option(self._h, key.encode(), int(value)), f"set_option({key})")

    def stat(self, key: str) -> int:
        out = ctypes.c_int64()
        native.check(self._lib.codd_knn_get_stat(self._h, key.encode(), ctypes.byref(out)), f"get_stat({key})")
        return out.value


def merge_keys(keys, k: int, device=None, space: str = "cosine"):
    """codd_knn_merge_keys_metric on a [B,m] int64 CUDA tensor of packed keys; `space` decides the distances written."""
    metric = native.metric_code(space)
    torch = _torch()
    lib = native.load()
    if not (isinstance(keys, torch.Tensor) and keys.is_cuda and keys.dtype == torch.int64 and keys.dim() == 2):
        raise ValueError("merge_keys wants a [B,m] int64 CUDA tensor")
    keys = keys.contiguous()
    dev = keys.device if device is None else torch.device(device)
    B, m = keys.shape
    out_keys = torch.empty((B, k), dtype=torch.int64, device=dev)
    dist = torch.empty((B, k), dtype=torch.float32, device=dev)
    rows = torch.empty((B, k), dtype=torch.int64, device=dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    native.check(
        lib.codd_knn_merge_keys_metric(dev.index or 0, keys.data_ptr(), B, m, int(k), metric, out_keys.data_ptr(), dist.data_ptr(), rows.data_ptr(), stream),
        "codd_knn_merge_keys_metric",
    )
    return out_keys, dist, rows


def slice_mask(global_bits, global_rows: int, row_base: int, count: int, device=None):
    """codd_knn_slice_mask: rows [row_base, row_base + count) of a mask over `global_rows` global rows (1-d int32 CUDA tensor of
    ceil(global_rows / 32) packed words) as the ceil(count / 32) words a shard's masked search takes; row_base need not be a
    multiple of 32, bits past either end are zero.  Asynchronous on the current stream."""
    torch = _torch()
    lib = native.load()
    if not (isinstance(global_bits, torch.Tensor) and global_bits.is_cuda and global_bits.dtype == torch.int32 and global_bits.dim() == 1):
        raise ValueError("slice_mask wants the global mask as a 1-d int32 CUDA tensor of packed words")
    global_rows, row_base, count = int(global_rows), int(row_base), int(count)
    if global_rows < 0 or row_base < 0 or count < 0 or global_bits.shape[0] != (global_rows + 31) // 32:
        raise ValueError(f"expected ceil({global_rows} / 32) global words and non-negative row_base / count, got {global_bits.shape[0]} words")
    global_bits = global_bits.contiguous()
    dev = global_bits.device if device is None else torch.device(device)
    nwords = (count + 31) // 32
    out = torch.empty((nwords,), dtype=torch.int32, device=dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    native.check(
        lib.codd_knn_slice_mask(dev.index or 0, global_bits.data_ptr() if global_bits.shape[0] else None, global_rows, row_base, count,
                                out.data_ptr() if nwords else None, nwords, stream),
        "codd_knn_slice_mask",
    )
    return out


def merge_shards(gathered, world_size: int, k: int, device=None, space: str = "cosine"):
    """codd_knn_merge_shards_metric on the [G*B, k_in] int64 CUDA tensor an all_gather of the ranks' [B, k_in] keys delivers;
    `space` decides the distances written."""
    metric = native.metric_code(space)
    torch = _torch()
    lib = native.load()
    if not (isinstance(gathered, torch.Tensor) and gathered.is_cuda and gathered.dtype == torch.int64 and gathered.dim() == 2
            and gathered.shape[0] % world_size == 0):
        raise ValueError("merge_shards wants a [G*B, k_in] int64 CUDA tensor")
    gathered = gathered.contiguous()
    dev = gathered.device if device is None else torch.device(device)
    B, k_in = gathered.shape[0] // world_size, gathered.shape[1]
    out_keys = torch.empty((B, k), dtype=torch.int64, device=dev)
    dist = torch.empty((B, k), dtype=torch.float32, device=dev)
    rows = torch.empty((B, k), dtype=torch.int64, device=dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    native.check(
        lib.codd_knn_merge_shards_metric(dev.index or 0, gathered.data_ptr(), int(world_size), B, k_in, int(k), metric, out_keys.data_ptr(),
                                         dist.data_ptr(), rows.data_ptr(), stream),
        "codd_knn_merge_shards_metric",
    )
    return out_keys, dist, rows
