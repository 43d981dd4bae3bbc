"""Row masks through the row-sharded search, worlds of 2 and 3 over gloo on the CPU: ShardedSearcher.search with
`allow=` (the shard-local mask) and with `allow_global=True` (one mask over global rows, sliced by every rank) must return what ONE
MaskedOracleEngine over the whole corpus returns under the global mask — ids and distances bit for bit, on every rank.  The
shard-local engine is the checker engine (no GPU); on the GPU the same ShardedSearcher drives DeviceKnnIndex / IvfShardEngine."""

import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from codd_query_engine_amd.sharded import ShardedSearcher
from oracle import knn_oracle as o
from tests._masked_oracle_engine import MaskedOracleEngine, allowed_rows
from tests.test_sharded_gloo import free_port, oracle_merge

D, B, K = 64, 5, 10
TIE_LO = 5


def tie_hi(n):
    return n // 2 + 3


class ShardMaskedEngine:
    """MaskedOracleEngine speaking the shard protocol: search_keys_masked(queries, allow, k, row_base) -> packed keys that carry
    GLOBAL rows, as an int64 tensor.  The keys are the oracle's own over the sub-matrix MaskedOracleEngine.search_masked searches
    (allowed AND live rows, slot order kept); only their row word is rewritten, sub-matrix index -> row_base + slot."""

    def __init__(self, inner: MaskedOracleEngine):
        self.inner = inner

    def count(self):
        return self.inner.count()

    def search_keys_masked(self, queries, allow, k, row_base=0):
        e = self.inner
        n = e.count()
        member = allowed_rows(allow, n)
        e.masks.append(member.copy())
        slots = np.flatnonzero(member & ~e._dead_mask()[:n])
        keys = np.zeros((np.asarray(queries).shape[0], k), dtype=np.uint64)
        if slots.size:
            sub = o.search_keys(np.ascontiguousarray(e._rows[slots]), e.dtype, e._prep(np.asarray(queries)), k, 0)
            hit = sub != 0
            at = (np.uint64(0xFFFFFFFF) - (sub[hit] & np.uint64(0xFFFFFFFF))).astype(np.int64)
            glob = (slots[at] + row_base).astype(np.uint64)
            keys[hit] = (sub[hit] & np.uint64(0xFFFFFFFF00000000)) | (np.uint64(0xFFFFFFFF) - glob)
        return torch.from_numpy(keys.view(np.int64).copy())


def words_of(mask):
    packed = np.packbits(mask, bitorder="little")
    words = np.zeros((mask.shape[0] + 31) // 32 * 4, dtype=np.uint8)
    words[: packed.shape[0]] = packed
    return words.view("<u4").copy()


def make_case(name):
    """(raw rows, queries, cuts: shard g owns global rows [cuts[g], cuts[g + 1]), global mask, global rows to delete)"""
    rng = np.random.default_rng(1700 + len(name))
    n, cuts = {
        "uneven":          (500, [0, 77, 401, 500]),
        "empty_shard":     (500, [0, 200, 200, 500]),
        "empty_slice":     (1001, [0, 500, 1001]),
        "cross_shard_tie": (1001, [0, 333, 1001]),
        "with_deletes":    (500, [0, 131, 300, 500]),
        "odd_row_base":    (1001, [0, 333, 1001]),      # 333 = 10 * 32 + 13: the second shard's words straddle global words
    }[name]
    raw = rng.standard_normal((n, D)).astype(np.float32)
    q = rng.standard_normal((B, D)).astype(np.float32)
    raw[tie_hi(n)] = raw[TIE_LO]                        # an exact tie across the cut: the lower GLOBAL row must win
    q[0] = raw[TIE_LO]
    mask = rng.random(n) < 0.5
    dead = np.zeros(0, dtype=np.int64)
    if name == "empty_slice":
        mask[500:] = False                              # rank 1's slice of the mask allows nothing
    if name == "cross_shard_tie":
        mask[[TIE_LO, tie_hi(n)]] = True
    if name == "with_deletes":
        dead = rng.choice(n, size=n // 5, replace=False)
        mask[dead[:20]] = True                          # allowed but dead: not returned
        mask[[TIE_LO, tie_hi(n)]] = True
        dead = dead[(dead != TIE_LO) & (dead != tie_hi(n))]
    return raw, q, cuts, mask, np.sort(dead)


def expected(name):
    raw, q, _, mask, dead = make_case(name)
    whole = MaskedOracleEngine(D)
    whole.upsert(np.arange(raw.shape[0], dtype=np.int64), raw)
    if dead.size:
        whole.delete(dead)
    return whole.search_masked(q, mask, K)


def worker(rank, world, port, name, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        raw, q, cuts, mask, dead = make_case(name)
        lo, hi = cuts[rank], cuts[rank + 1]
        eng = MaskedOracleEngine(D)
        if hi > lo:
            eng.upsert(np.arange(hi - lo, dtype=np.int64), raw[lo:hi])
            mine = dead[(dead >= lo) & (dead < hi)] - lo
            if mine.size:
                eng.delete(mine)
        searcher = ShardedSearcher(ShardMaskedEngine(eng), row_base=lo, merge=oracle_merge)
        # the same collective order on every rank: local bool, local words, global bool, global words, async
        outs = [
            searcher.search(q, K, allow=mask[lo:hi]),
            searcher.search(q, K, allow=words_of(mask[lo:hi])),
            searcher.search(q, K, allow=mask, allow_global=True),
            searcher.search(q, K, allow=words_of(mask), allow_global=True),
            searcher.search_async(q, K, allow=mask, allow_global=True).result(),
        ]
        for dd, rr in outs[1:]:
            assert torch.equal(dd, outs[0][0]) and torch.equal(rr, outs[0][1])
        assert all(np.array_equal(m, mask[lo:hi]) for m in eng.masks) and len(eng.masks) == len(outs)
        with pytest.raises(ValueError):                 # raised before any collective: the ranks stay in step
            searcher.search(q, K, scopes=np.zeros(B, dtype=np.uint32), allow=mask[lo:hi])
        np.savez(os.path.join(out_dir, f"rank{rank}.npz"), dist=outs[0][0].numpy(), rows=outs[0][1].numpy())
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize(
    "world,name",
    [(3, "uneven"), (3, "empty_shard"), (2, "empty_slice"), (2, "cross_shard_tie"), (3, "with_deletes"), (2, "odd_row_base")],
)
def test_sharded_masked_search_equals_one_masked_index(tmp_path, world, name):
    port = free_port()
    mp.spawn(worker, args=(world, port, name, str(tmp_path)), nprocs=world, join=True)
    d_ref, r_ref = expected(name)
    for rank in range(world):
        got = np.load(tmp_path / f"rank{rank}.npz")
        assert np.array_equal(got["rows"], r_ref), f"rank {rank}"
        assert np.array_equal(got["dist"], d_ref), f"rank {rank}"
    raw, _, cuts, mask, _ = make_case(name)
    if mask[TIE_LO] and mask[tie_hi(raw.shape[0])]:
        assert r_ref[0, 0] == TIE_LO and r_ref[0, 1] == tie_hi(raw.shape[0])    # tie across shards: lower global row first
    if name in ("cross_shard_tie", "with_deletes"):
        assert mask[TIE_LO] and mask[tie_hi(raw.shape[0])] and np.searchsorted(cuts, TIE_LO, "right") != np.searchsorted(cuts, tie_hi(raw.shape[0]), "right")


def test_scopes_and_allow_together_raise_without_a_process_group():
    eng = MaskedOracleEngine(D)
    eng.upsert(np.arange(40, dtype=np.int64), np.random.default_rng(3).standard_normal((40, D)).astype(np.float32))
    searcher = ShardedSearcher(ShardMaskedEngine(eng), row_base=0, merge=oracle_merge)
    q = np.ones((2, D), dtype=np.float32)
    with pytest.raises(ValueError):
        searcher.search(q, K, scopes=np.zeros(2, dtype=np.uint32), allow=np.ones(40, dtype=bool))
    with pytest.raises(ValueError):
        searcher.search_keys_local(q, K, scopes=np.zeros(2, dtype=np.uint32), allow=np.ones(40, dtype=bool), allow_global=True)
    # one rank, no collective: a global mask longer than the shard is cut to it, a shorter one allows nothing past its end
    d_ref, r_ref = eng.search_masked(q, np.arange(40) % 3 == 0, K)
    dd, rr = searcher.search(q, K, allow=np.arange(64) % 3 == 0, allow_global=True)
    assert np.array_equal(rr.numpy(), r_ref) and np.array_equal(dd.numpy(), d_ref)
    dd, rr = searcher.search(q, K, allow=np.arange(7) % 3 == 0, allow_global=True)
    assert sorted(rr.numpy()[0].tolist()) == [-1] * (K - 3) + [0, 3, 6]
