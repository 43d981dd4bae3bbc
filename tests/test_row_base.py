"""row_base on the host side (no GPU): ctypes converts a Python int to the C ABI's uint32 without a range check — 2**32 + 5 would
arrive as 5, -1 as 0xFFFFFFFF — so native.check_row_base stands in front of every wrapper that forwards one, and in front of the
checker engines under tests/ alike."""

import numpy as np
import pytest

from codd_query_engine_amd import native
from codd_query_engine_amd.sharded import ShardedSearcher
from tests._oracle_engine import OracleEngine
from tests._scoped_oracle_engine import ScopedOracleEngine

N = 1_001
TOP, OVER = 0xFFFFFFFE - N, 0xFFFFFFFF - N


def test_check_row_base_accepts_the_last_legal_base_and_nothing_beyond():
    assert native.check_row_base(TOP, N) == TOP and native.check_row_base(0, N) == 0 and native.check_row_base(0xFFFFFFFE, 0) == 0xFFFFFFFE
    assert native.check_row_base(np.int64(TOP), np.int64(N)) == TOP and isinstance(native.check_row_base(np.int64(7), N), int)
    for bad in (OVER, -1, 2**32, 2**32 + 5, 0xFFFFFFFF):
        with pytest.raises(ValueError, match="32 bits"):
            native.check_row_base(bad, N)
    with pytest.raises(ValueError, match="32 bits"):
        native.check_row_base(0xFFFFFFFF, 0)
    assert native.MAX_GLOBAL_ROW == 0xFFFFFFFD == TOP + N - 1


def engine(cls=OracleEngine):
    rng = np.random.default_rng(41)
    e = cls(64, "f32")
    e.upsert(np.arange(N, dtype=np.int64), rng.standard_normal((N, 64)).astype(np.float32))
    return e, rng.standard_normal((4, 64)).astype(np.float32)


def test_sharded_searcher_refuses_a_base_that_ctypes_would_truncate():
    e, q = engine()
    for bad in (2**32 + 5, 2**32, -1, 0xFFFFFFFF):
        with pytest.raises(ValueError, match="32 bits"):
            ShardedSearcher(e, row_base=bad, merge=OracleEngine.merge_keys)       # (not: a searcher that answers with base 5)
    d0, r0 = ShardedSearcher(e, row_base=0, merge=OracleEngine.merge_keys).search(q, 10)
    d, r = ShardedSearcher(e, row_base=TOP, merge=OracleEngine.merge_keys).search(q, 10)
    assert np.array_equal(r, r0 + TOP) and r.max() <= 0xFFFFFFFD and np.array_equal(d, d0)
    with pytest.raises(ValueError, match="32 bits"):
        ShardedSearcher(e, row_base=OVER, merge=OracleEngine.merge_keys).search(q, 10)   # row_base + count: known per search


def test_the_checker_engines_refuse_the_same_bases():
    e, q = engine(ScopedOracleEngine)
    scopes = np.zeros(4, dtype=np.uint32)
    for bad in (OVER, -1, 2**32 + 5):
        with pytest.raises(ValueError, match="32 bits"):
            e.search_keys(q, 10, bad)
        with pytest.raises(ValueError, match="32 bits"):
            e.search_keys_scoped(q, scopes, 10, bad)
    assert np.array_equal(e.search_keys(q, 10, TOP), e.search_keys_scoped(q, scopes, 10, TOP))
