"""
ctypes binding of include/codd_knn.h (the C ABI of the HIP library).

There is no CPU fallback: if libcodd_knn.so is missing or fails to load, or no GPU is
visible, every product entry point raises NativeLibraryError — loudly, on purpose.
"""

from __future__ import annotations

import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# CODD_KNN_LIB selects an alternative build of the SAME source (kernel A/B experiments, scripts/)
LIB_PATH = os.environ.get("CODD_KNN_LIB") or os.path.join(_HERE, "csrc", "libcodd_knn.so")

DTYPE_CODES = {"f32": 0, "bf16": 1, "f16": 2}
DTYPE_NAMES = {v: k for k, v in DTYPE_CODES.items()}
METRIC_COSINE = 0
METRIC_IP = 1
METRIC_L2 = 2
# ChromaDB's `hnsw:space` names <-> CODD_KNN_METRIC_*
METRIC_CODES = {"cosine": METRIC_COSINE, "ip": METRIC_IP, "l2": METRIC_L2}
METRIC_NAMES = {v: k for k, v in METRIC_CODES.items()}
MAX_K = 128
MAX_BATCH = 1024
MAX_SCOPE = 1048575
MAX_NEEDLE = 256
MAX_DFA_STATES = 255  # CODD_KNN_MAX_DFA_STATES
MAX_DFA_TABLE = 8192  # CODD_KNN_MAX_DFA_TABLE: bytes of a DFA's next[nstates][nclasses]
MAX_EMBED_DIM = 4096       # codd_knn_embedder_create: dim in [8, 4096]
MAX_EMBED_BYTES = 1 << 28  # CODD_KNN_MAX_EMBED_BYTES: text bytes per codd_knn_embed_texts_host call
MAX_EMBED_TEXTS = 1 << 24  # CODD_KNN_MAX_EMBED_TEXTS
MAX_GLOBAL_ROW = 0xFFFFFFFD  # the low word of a packed key is 0xFFFFFFFF - global row, and 0 = empty: row_base + count < 0xFFFFFFFF

# every symbol include/codd_knn.h declares: (name, restype, argtypes)
_c_idx = ctypes.c_void_p
_i64p = ctypes.POINTER(ctypes.c_int64)
_intp = ctypes.POINTER(ctypes.c_int)
ABI = [
    ("codd_knn_version", ctypes.c_char_p, []),
    ("codd_knn_last_error", ctypes.c_char_p, []),
    ("codd_knn_create", ctypes.c_int, [ctypes.POINTER(_c_idx), ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    ("codd_knn_destroy", ctypes.c_int, [_c_idx]),
    ("codd_knn_reserve", ctypes.c_int, [_c_idx, ctypes.c_int64]),
    ("codd_knn_upsert_host", ctypes.c_int, [_c_idx, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int]),
    ("codd_knn_upsert_device", ctypes.c_int, [_c_idx, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p]),
    ("codd_knn_load_rows", ctypes.c_int, [_c_idx, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64]),
    ("codd_knn_count", ctypes.c_int, [_c_idx, _i64p]),
    ("codd_knn_dim", ctypes.c_int, [_c_idx, _intp, _intp, _intp]),
    ("codd_knn_read_rows", ctypes.c_int, [_c_idx, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p]),
    ("codd_knn_search", ctypes.c_int, [_c_idx, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    ("codd_knn_search_keys", ctypes.c_int, [_c_idx, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]),
    ("codd_knn_merge_keys", ctypes.c_int, [ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    ("codd_knn_merge_shards", ctypes.c_int, [ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    ("codd_knn_merge_keys_metric", ctypes.c_int, [ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    ("codd_knn_merge_shards_metric", ctypes.c_int, [ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    ("codd_knn_approx_scores", ctypes.c_int, [_c_idx, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]),
    ("codd_knn_filter_slack", ctypes.c_int, [_c_idx, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]),
    ("codd_knn_copy_rows_f32",ctypes.c_int, [_c_idx, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]),
    ("codd_knn_ivf_install", ctypes.c_int, [_c_idx, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    ("codd_knn_ivf_search", ctypes.c_int, [_c_idx, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    ("codd_knn_ivf_refresh", ctypes.c_int, [_c_idx, ctypes.c_void_p]),
    ("codd_knn_set_scopes_host", ctypes.c_int, [_c_idx, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64]),
    ("codd_knn_search_scoped", ctypes.c_int, [_c_idx, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    ("codd_knn_search_masked", ctypes.c_int, [_c_idx, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    ("codd_knn_search_masked_dev", ctypes.c_int, [_c_idx, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    ("codd_knn_set_documents_host", ctypes.c_int, [_c_idx, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64]),
    ("codd_knn_match_documents", ctypes.c_int, [_c_idx, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]),
    ("codd_knn_match_documents_dfa", ctypes.c_int, [_c_idx, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                    ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]),
    ("codd_knn_ivf_search_masked", ctypes.c_int, [_c_idx, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    ("codd_knn_ivf_search_masked_dev", ctypes.c_int, [_c_idx, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    ("codd_knn_slice_mask", ctypes.c_int, [ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]),
    ("codd_knn_embedder_create", ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, ctypes.c_int, ctypes.c_float]),
    ("codd_knn_embedder_destroy", ctypes.c_int, [ctypes.c_void_p]),
    ("codd_knn_embed_texts_host", ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]),
    ("codd_knn_set_column_host", ctypes.c_int, [_c_idx, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64]),
    ("codd_knn_drop_columns", ctypes.c_int, [_c_idx]),
    ("codd_knn_eval_where", ctypes.c_int, [_c_idx, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]),
    ("codd_knn_delete_host", ctypes.c_int, [_c_idx, ctypes.c_void_p, ctypes.c_int64]),
    ("codd_knn_live_count", ctypes.c_int, [_c_idx, _i64p]),
    ("codd_knn_compact", ctypes.c_int, [_c_idx, _i64p]),
    ("codd_knn_set_option", ctypes.c_int, [_c_idx, ctypes.c_char_p, ctypes.c_int64]),
    ("codd_knn_get_stat", ctypes.c_int, [_c_idx, ctypes.c_char_p, _i64p]),
    ("codd_knn_debug_live_allocations", ctypes.c_int, [_i64p, _i64p, _i64p]),
    ("codd_knn_debug_last_pass", ctypes.c_int, [_c_idx, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64]),
]


class LastPassInfo(ctypes.Structure):
    """codd_knn_last_pass of include/codd_knn.h"""

    _fields_ = (
        [(name, ctypes.c_int32) for name in ("family", "nbq", "ts", "res", "el", "sqd", "nq", "k", "hit_cap", "per_block_filter", "per_block_finalize")]
        + [("eps", ctypes.c_float)]
        + [(name, ctypes.c_int64) for name in ("n", "sample_tiles", "sample_stride")]
        + [("flags", ctypes.c_uint32 * 4), ("fb_count", ctypes.c_uint32), ("cascade_d", ctypes.c_uint32)]
    )


FILTER_FAMILIES = ("GEMM", "TILE", "TILE_F16")

# codd_knn_eval_where: the limits of include/codd_knn.h; where_columns.py states the same numbers without ctypes
MAX_COLUMNS = 32          # CODD_KNN_MAX_COLUMNS
WHERE_MAX_LEAVES = 32     # CODD_KNN_WHERE_MAX_LEAVES
WHERE_MAX_LITERALS = 256  # CODD_KNN_WHERE_MAX_LITERALS
WHERE_MAX_OPS = 64        # CODD_KNN_WHERE_MAX_OPS


class WhereLeaf(ctypes.Structure):
    """codd_knn_where_leaf of include/codd_knn.h"""

    _fields_ = [(name, ctypes.c_uint8) for name in ("column", "tag", "kind", "negate")] + [("lit_first", ctypes.c_uint16), ("lit_count", ctypes.c_uint16)]


class WhereProgram(ctypes.Structure):
    """codd_knn_where_program of include/codd_knn.h"""

    _fields_ = [(name, ctypes.c_int32) for name in ("nleaves", "nliterals", "nops", "reserved")] + [
        ("leaves", WhereLeaf * WHERE_MAX_LEAVES), ("ops", ctypes.c_uint8 * WHERE_MAX_OPS), ("literals", ctypes.c_uint64 * WHERE_MAX_LITERALS)]


def where_program(program) -> WhereProgram:
    """The C form of a program: anything with `leaves` ((column, tag, kind, negate, lit_first, lit_count) each), `literals` (uint64
    values) and `ops` (bytes), as where_columns.compile_where returns it.  ValueError for what the struct cannot hold — more entries
    than its arrays have, a field outside its integer type; everything else is the library's own host check (EINVAL)."""
    leaves, literals, ops = list(program.leaves), list(program.literals), list(program.ops)
    if len(leaves) > WHERE_MAX_LEAVES or len(literals) > WHERE_MAX_LITERALS or len(ops) > WHERE_MAX_OPS:
        raise ValueError(f"a where program holds at most {WHERE_MAX_LEAVES} leaves, {WHERE_MAX_LITERALS} literals and {WHERE_MAX_OPS} operators, "
                         f"got {len(leaves)} / {len(literals)} / {len(ops)}")
    out = WhereProgram()
    out.nleaves, out.nliterals, out.nops = len(leaves), len(literals), len(ops)
    for i, leaf in enumerate(leaves):
        fields = [int(v) for v in leaf]
        if len(fields) != 6 or any(not 0 <= v <= 0xFF for v in fields[:4]) or any(not 0 <= v <= 0xFFFF for v in fields[4:]):
            raise ValueError(f"leaf {i} is not (column, tag, kind, negate, lit_first, lit_count) in range: {leaf!r}")
        out.leaves[i] = WhereLeaf(*fields)
    for i, lit in enumerate(literals):
        if not 0 <= int(lit) < 1 << 64:
            raise ValueError(f"literal {i} is no uint64: {lit!r}")
        out.literals[i] = int(lit)
    for i, op in enumerate(ops):
        if not 0 <= int(op) <= 0xFF:
            raise ValueError(f"operator {i} is no byte: {op!r}")
        out.ops[i] = int(op)
    return out


class NativeLibraryError(RuntimeError):
    """libcodd_knn.so is absent/unloadable, or a C-ABI call returned an error code."""


_lib = None


def load() -> ctypes.CDLL:
    """dlopen the in-tree HIP library and bind every ABI symbol.

    torch is imported first so that the process holds ONE HIP runtime: torch's wheel
    bundles libamdhip64 under the same SONAME the library was linked against, and the
    dynamic loader then resolves ours to the copy torch already mapped — device pointers
    and streams can cross between the two.
    """
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NativeLibraryError(
            f"{LIB_PATH} not found: build it with `python -m codd_query_engine_amd.build` "
            "(there is no CPU fallback for the search path)"
        )
    try:
        import torch  # noqa: F401  (side effect: maps torch's HIP runtime first)
    except Exception:  # pragma: no cover - torch is part of the image
        pass
    try:
        lib = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
    except OSError as e:
        raise NativeLibraryError(f"cannot load {LIB_PATH}: {e}") from e
    for name, restype, argtypes in ABI:
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise NativeLibraryError(f"{LIB_PATH} does not export {name}") from e
        fn.restype = restype
        fn.argtypes = argtypes
    _lib = lib
    return lib


def last_error() -> str:
    msg = load().codd_knn_last_error()
    return msg.decode("utf-8", "replace") if msg else ""


def check(rc: int, what: str) -> None:
    if rc != 0:
        raise NativeLibraryError(f"{what} failed with code {rc}: {last_error()}")


def metric_code(space: str) -> int:
    """CODD_KNN_METRIC_* of a ChromaDB space name; ValueError for a name that is none of METRIC_CODES."""
    if space not in METRIC_CODES:
        raise ValueError(f"space must be one of {sorted(METRIC_CODES)}, got {space!r}")
    return METRIC_CODES[space]


def check_row_base(row_base: int, count: int) -> int:
    """The `row_base` of a shard of `count` rows as the C ABI takes it.  ctypes converts to uint32 without a range check
    (2**32 + 5 would arrive as 5, -1 as 0xFFFFFFFF), so every wrapper that forwards a row_base passes it through here first:
    ValueError unless 0 <= row_base and row_base + count < 0xFFFFFFFF (include/codd_knn.h, conventions)."""
    row_base, count = int(row_base), int(count)
    if row_base < 0 or count < 0 or row_base + count > MAX_GLOBAL_ROW + 1:
        raise ValueError(f"global row ids must fit 32 bits: row_base {row_base} + count {count} must stay below 0xFFFFFFFF, row_base >= 0")
    return row_base


def live_allocations() -> tuple:
    """(buffers, bytes, events) the library holds in this process right now (codd_knn_debug_live_allocations)."""
    out = [ctypes.c_int64() for _ in range(3)]
    check(load().codd_knn_debug_live_allocations(*[ctypes.byref(o) for o in out]), "debug_live_allocations")
    return tuple(o.value for o in out)
