"""
where_columns — the host half of `where=` on the device: metadata as columns, filters as predicate programs.

numpy and the standard library only: neither torch nor HIP is imported here, so everything below runs, and is tested, without a GPU.

Columns.  One per metadata key.  Per row slot a column holds a tag (uint8) and a cell (uint64), Collection._value_class's classes:

    tag 0  absent   the record has no such key (or no metadata, or the slot is a tombstone); the cell is ignored
    tag 1  bool     cell 0 / 1
    tag 2  number   cell = number_key(value): the bits of float64(value) + 0.0 (so that -0.0 and +0.0 agree), all of them flipped
                    for a negative value, else the sign bit alone.  Unsigned comparison of keys is numeric comparison, so the device
                    compares integers and performs no floating-point operation.  An int is encodable only if int(float(v)) == v
                    (Python compares ints exactly; 2**53 + 1 has no float64); +-inf are, NaN is not (it equals nothing).
    tag 3  str      cell = the string's code in the column's dictionary: codes from 1 in first-seen order, never renumbered

A column that meets a value it cannot encode — NaN, an int beyond float64's exact range, a value of another type — becomes
`host_only` for good: every filter that names its key takes the façade's host route.  The numpy arrays here are the MIRRORS of what
the engine holds (DeviceKnnIndex.set_column); the façade keeps both in step (ColumnSet.encode_slots / wrote / compacted).

Programs.  compile_where turns a CHECKED filter (Collection._check_where) into leaves, literals and a postfix program — the
codd_knn_where_program of include/codd_knn.h — or returns None: the filter then runs on the host, whole.  A leaf is (column, tag
class, kind, negate, literal range): kind IN passes when the tag equals the class and the cell is among the literals; LT LE GT GE
compare a number's cell with one literal key; `negate` is $ne / $nin's rule, the row passes iff the un-negated leaf fails — so a
record without the key passes.  $eq $ne $in $nin become IN lists, one leaf per value class among the literals; a str literal the
dictionary does not know contributes no literal, and a leaf without literals is constant false.  Comparisons on a bool are evaluated
here over {False, True}, comparisons on a str over the dictionary's entries, and become IN lists.  Equal leaves are emitted once.
"""

from __future__ import annotations

import struct
from typing import Any, Iterable, Mapping, Optional, Sequence

import numpy as np

# the limits of include/codd_knn.h (tests/test_where_api.py holds the header against them)
MAX_COLUMNS = 32    # CODD_KNN_MAX_COLUMNS: columns per index
MAX_LEAVES = 32     # CODD_KNN_WHERE_MAX_LEAVES
MAX_LITERALS = 256  # CODD_KNN_WHERE_MAX_LITERALS
MAX_OPS = 64        # CODD_KNN_WHERE_MAX_OPS (a well-formed program of p pushes has 2 p - 1 operators: 63 at the most)
MAX_STACK = 32      # postfix stack entries the kernel has

TAG_ABSENT, TAG_BOOL, TAG_NUMBER, TAG_STR = 0, 1, 2, 3
KIND_IN, KIND_LT, KIND_LE, KIND_GT, KIND_GE = 0, 1, 2, 3, 4
OP_AND, OP_OR = 0xFE, 0xFF   # a postfix operator below these pushes that leaf

_SIGN = 1 << 63
_ALL = (1 << 64) - 1
_KIND_OF = {"$lt": KIND_LT, "$lte": KIND_LE, "$gt": KIND_GT, "$gte": KIND_GE}
_TESTS = {"$gt": lambda a, b: a > b, "$gte": lambda a, b: a >= b, "$lt": lambda a, b: a < b, "$lte": lambda a, b: a <= b}


def value_tag(v) -> int:
    """TAG_BOOL / TAG_NUMBER / TAG_STR by Collection._value_class's rule (a bool is no number); TAG_ABSENT for anything else."""
    if isinstance(v, bool):
        return TAG_BOOL
    if isinstance(v, (int, float)):
        return TAG_NUMBER
    return TAG_STR if isinstance(v, str) else TAG_ABSENT


def number_key(v) -> Optional[int]:
    """The order-preserving uint64 key of an int / float, None where it has none: NaN, or an int that float64 does not hold exactly."""
    if isinstance(v, int):
        try:
            x = float(v)
        except OverflowError:
            return None
        if int(x) != v:
            return None
    else:
        x = float(v)
        if x != x:
            return None
    (bits,) = struct.unpack("<Q", struct.pack("<d", x + 0.0))
    return bits ^ _ALL if bits & _SIGN else bits ^ _SIGN


def key_number(key: int) -> float:
    """number_key's inverse (tests, diagnostics)."""
    bits = key ^ _SIGN if key & _SIGN else key ^ _ALL
    return struct.unpack("<d", struct.pack("<Q", bits))[0]


class Column:
    """One metadata key's tags, cells and str dictionary over the row slots (the mirror of the engine's column `index`)."""

    def __init__(self, key: str, index: int):
        self.key = key
        self.index = index               # the engine's column number
        self.codes: dict[str, int] = {}  # str -> code, from 1, first seen first
        self.host_only = False
        self.adopt(np.zeros(0, dtype=np.uint8), np.zeros(0, dtype=np.uint64))

    def adopt(self, tags: np.ndarray, cells: np.ndarray) -> None:
        """These arrays are the mirrors from now on.  `tags` and `cells` are views of the first n slots of a store that `resize`
        grows by half at a time, as the engine grows its row store: an appending upsert does not copy the column."""
        self._tag_store, self._cell_store = tags, cells
        self.tags, self.cells = tags, cells

    def encode(self, metadata: Optional[Mapping]) -> Optional[tuple]:
        """(tag, cell) of a record with this metadata; None for a value that has no cell (the column is host_only from then on)."""
        if not metadata or self.key not in metadata:
            return TAG_ABSENT, 0
        v = metadata[self.key]
        tag = value_tag(v)
        if tag == TAG_BOOL:
            return tag, int(v)
        if tag == TAG_NUMBER:
            cell = number_key(v)
            if cell is not None:
                return tag, cell
        elif tag == TAG_STR:
            code = self.codes.get(v)
            if code is None:
                code = self.codes[v] = len(self.codes) + 1
            return tag, code
        self.retire()
        return None

    def encode_many(self, metadatas: Iterable[Optional[Mapping]], n: int) -> Optional[tuple]:
        """(tags [n], cells [n]) of n records, None once the column is host_only."""
        tags = np.zeros(n, dtype=np.uint8)
        cells = np.zeros(n, dtype=np.uint64)
        for i, md in enumerate(metadatas):
            if md and self.key in md:   # (an absent cell is the zeros the arrays start with)
                pair = self.encode(md)
                if pair is None:
                    return None
                tags[i], cells[i] = pair
        return tags, cells

    def retire(self) -> None:
        """host_only from now on, for as long as the column set lives (until the collection is loaded again): the state does not
        go back when the offending record is deleted, and the engine keeps the column's storage until its columns are dropped."""
        self.host_only = True
        self.adopt(np.zeros(0, dtype=np.uint8), np.zeros(0, dtype=np.uint64))

    def resize(self, n: int) -> None:
        """The mirrors cover n row slots; new slots are absent."""
        have = self.tags.shape[0]
        if self.host_only or n == have:
            return
        room = self._tag_store.shape[0]
        if n > room:
            room = max(n, room + room // 2 + 1024)
            tags, cells = np.zeros(room, dtype=np.uint8), np.zeros(room, dtype=np.uint64)
            tags[:have], cells[:have] = self.tags, self.cells
            self._tag_store, self._cell_store = tags, cells
        elif n < have:   # (slots given up read absent when they come back)
            self._tag_store[n:have] = 0
            self._cell_store[n:have] = 0
        self.tags, self.cells = self._tag_store[:n], self._cell_store[:n]

    def value_at(self, slot: int):
        """What the mirrors say row slot `slot` holds: (tag, value) with the value decoded (None when absent)."""
        tag, cell = int(self.tags[slot]), int(self.cells[slot])
        if tag == TAG_BOOL:
            return tag, bool(cell)
        if tag == TAG_NUMBER:
            return tag, key_number(cell)
        if tag == TAG_STR:
            return tag, next(s for s, code in self.codes.items() if code == cell)
        return TAG_ABSENT, None


class ColumnSet:
    """The columns of one collection, by key.  `build` makes a key's column from the records in one pass; afterwards the façade
    calls `encode_slots` before it tells the engine about a write and `wrote` once the engine has taken it, `compacted` after a
    compaction and `clear` when the rows are replaced."""

    def __init__(self):
        self.by_key: dict[str, Column] = {}
        self._next_index = 0

    def __len__(self) -> int:
        return len(self.by_key)

    def clear(self) -> None:
        self.by_key.clear()
        self._next_index = 0

    def get(self, key: str) -> Optional[Column]:
        return self.by_key.get(key)

    def has_room(self) -> bool:
        return self._next_index < MAX_COLUMNS

    def build(self, key: str, metadatas: Sequence[Optional[Mapping]]) -> Column:
        """A new column over all row slots (a tombstone's metadata is None: absent).  host_only if a value has no cell, or if the
        index's MAX_COLUMNS columns are taken; such a column takes no engine column."""
        col = Column(key, self._next_index)
        self.by_key[key] = col
        if not self.has_room():
            col.retire()
            return col
        pair = col.encode_many(metadatas, len(metadatas))
        if pair is not None:
            col.adopt(*pair)
            self._next_index += 1
        return col

    def device_columns(self) -> list:
        return [c for c in self.by_key.values() if not c.host_only]

    def encode_slots(self, metadatas: Sequence[Optional[Mapping]]) -> list:
        """[(column, tags, cells)] of the records an upsert writes, for every column that is on the device.  A column that meets
        a value without a cell drops out (host_only) and is left out."""
        out = []
        for col in self.device_columns():
            pair = col.encode_many(metadatas, len(metadatas))
            if pair is not None:
                out.append((col, pair[0], pair[1]))
        return out

    def wrote(self, col: Column, slots: np.ndarray, tags: np.ndarray, cells: np.ndarray) -> None:
        """The engine has taken these cells: the mirrors follow."""
        if not col.host_only:
            col.tags[slots] = tags
            col.cells[slots] = cells

    def resize(self, n: int) -> None:
        for col in self.by_key.values():
            col.resize(n)

    def compacted(self, keep: Sequence[int]) -> None:
        """The engine moved the live rows `keep` (ascending old slots) to 0 .. len(keep) - 1, its columns with them."""
        keep = np.asarray(keep, dtype=np.int64)
        for col in self.device_columns():
            col.adopt(col.tags[keep], col.cells[keep])


class Program:
    """leaves: (column, tag, kind, negate, lit_first, lit_count) each; literals: uint64 values; ops: the postfix bytes."""

    def __init__(self):
        self.leaves: list[tuple] = []
        self.literals: list[int] = []
        self.ops: list[int] = []
        self._leaf_of: dict[tuple, int] = {}

    def leaf(self, column: int, tag: int, kind: int, negate: bool, literals: Sequence[int]) -> None:
        """Push the leaf (emitted once however often the filter states it)."""
        key = (column, tag, kind, bool(negate), tuple(literals))
        at = self._leaf_of.get(key)
        if at is None:
            at = self._leaf_of[key] = len(self.leaves)
            self.leaves.append((column, tag, kind, int(bool(negate)), len(self.literals), len(literals)))
            self.literals.extend(literals)
        self.ops.append(at)

    def columns(self) -> list:
        return sorted({leaf[0] for leaf in self.leaves})

    def fits(self) -> bool:
        depth = most = 0
        for op in self.ops:
            depth += -1 if op >= OP_AND else 1
            most = max(most, depth)
        return (len(self.leaves) <= MAX_LEAVES and len(self.literals) <= MAX_LITERALS and len(self.ops) <= MAX_OPS and most <= MAX_STACK
                and all(leaf[4] + leaf[5] <= 0xFFFF for leaf in self.leaves))


def filter_keys(where) -> list:
    """The metadata keys a checked filter names, each once, in order of appearance."""
    (key, cond), = where.items()
    if key in ("$and", "$or"):
        out: list = []
        for sub in cond:
            out += [k for k in filter_keys(sub) if k not in out]
        return out
    return [key]


def _compile(where, columns: Mapping[str, Column], prog: Program) -> bool:
    (key, cond), = where.items()
    if key in ("$and", "$or"):
        for i, sub in enumerate(cond):
            if not _compile(sub, columns, prog):
                return False
            if i:
                prog.ops.append(OP_AND if key == "$and" else OP_OR)
        return True
    col = columns.get(key)
    if col is None or col.host_only:
        return False
    (op, val), = (cond if isinstance(cond, dict) else {"$eq": cond}).items()
    if op in ("$eq", "$ne", "$in", "$nin"):
        negate = op in ("$ne", "$nin")
        by_tag: dict[int, list] = {}
        seen: set = set()
        for v in (val if op in ("$in", "$nin") else [val]):
            tag = value_tag(v)
            cells = by_tag.setdefault(tag, [])
            if tag == TAG_BOOL:
                cell = int(v)
            elif tag == TAG_NUMBER:
                cell = number_key(v)
                if cell is None:
                    return False   # (NaN, 2**53 + 1: Python's own comparison decides, on the host)
            else:
                cell = col.codes.get(v)   # (a str nobody stored matches nothing: no literal)
            if cell is not None and (tag, cell) not in seen:
                seen.add((tag, cell))
                cells.append(cell)
                if len(seen) > MAX_LITERALS:
                    return False   # (over the literal budget already: no need to read the rest of the list)
        # one IN leaf per class; $in: any of them, $nin: none of them.  Classes without a literal are left out unless none has one.
        tags = [t for t in sorted(by_tag) if by_tag[t]] or sorted(by_tag)[:1]
        for i, tag in enumerate(tags):
            prog.leaf(col.index, tag, KIND_IN, negate, by_tag[tag])
            if i:
                prog.ops.append(OP_AND if negate else OP_OR)
        return True
    tag = value_tag(val)
    if tag == TAG_NUMBER:
        cell = number_key(val)
        if cell is None:
            return False
        prog.leaf(col.index, TAG_NUMBER, _KIND_OF[op], False, [cell])
        return True
    test = _TESTS[op]
    if tag == TAG_BOOL:
        prog.leaf(col.index, TAG_BOOL, KIND_IN, False, [int(b) for b in (False, True) if test(b, val)])
        return True
    accepted = [code for s, code in col.codes.items() if test(s, val)]   # (the key's distinct strings, not its records)
    if len(accepted) > MAX_LITERALS:
        return False
    prog.leaf(col.index, TAG_STR, KIND_IN, False, accepted)
    return True


def compile_where(where, columns: Mapping[str, Any]) -> Optional[Program]:
    """The program of a checked filter over `columns` (key -> Column, ColumnSet.by_key), or None where it has to run on the host: a
    key without a column or with a host_only one, a number literal without a key, a str comparison that accepts more strings
    than the literal budget holds, or a program beyond MAX_LEAVES / MAX_LITERALS / MAX_OPS / MAX_STACK."""
    prog = Program()
    if not _compile(where, columns, prog) or not prog.fits():
        return None
    return prog
