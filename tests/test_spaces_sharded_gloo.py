"""world_size-2 run of the row-sharded search of an l2 and of an ip index over gloo on the CPU: the shards' keys
carry 0 - distance (l2) or the dot product (ip) as their score, merge as integers like any keys, and the merged answer — ids and
distance bits — equals the unsharded one.  The shard-local search is the checker engine with spaces."""

import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from codd_query_engine_amd.sharded import ShardedSearcher, shard_bounds
from tests import _space_reference as sr
from tests._space_oracle_engine import SpaceOracleEngine
from tests.test_sharded_gloo import TensorOracleEngine, free_port


def make_data(n, d, B):
    rng = np.random.default_rng(78)
    raw = (rng.standard_normal((n, d)) * rng.uniform(0.5, 2.0, (n, 1))).astype(np.float32)
    q = (1.3 * rng.standard_normal((B, d))).astype(np.float32)
    raw[n // 2 + 3] = raw[5]  # a cross-shard exact tie: the lower GLOBAL row must win
    q[0] = raw[5]
    return raw, q


def worker(rank, world, port, space, n, d, B, k, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        raw, q = make_data(n, d, B)
        lo, hi = shard_bounds(n, world, rank)
        eng = SpaceOracleEngine(d, "f32", space)
        eng.upsert(np.arange(hi - lo, dtype=np.int64), raw[lo:hi], normalize=False)

        def merge(keys_t, k):
            merged, dd, rr = eng.merge_keys(keys_t.numpy().view(np.uint64), k)
            return torch.from_numpy(merged.view(np.int64).copy()), torch.from_numpy(dd), torch.from_numpy(rr)

        dd, rr = ShardedSearcher(TensorOracleEngine(eng), row_base=lo, merge=merge).search(q, k)
        np.savez(os.path.join(out_dir, f"rank{rank}.npz"), dist=dd.numpy(), rows=rr.numpy())
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("space", ["l2", "ip"])
def test_sharded_search_of_a_space_equals_the_unsharded_answer(tmp_path, space):
    world, n, d, B, k = 2, 401, 70, 5, 10
    mp.spawn(worker, args=(world, free_port(), space, n, d, B, k, str(tmp_path)), nprocs=world, join=True)
    raw, q = make_data(n, d, B)
    _, d_ref, r_ref = sr.Reference(space, raw, "f32", q).topk(B, k)
    for rank in range(world):
        got = np.load(tmp_path / f"rank{rank}.npz")
        assert np.array_equal(got["rows"], r_ref), f"rank {rank}"
        assert np.array_equal(got["dist"].view(np.uint32), d_ref.view(np.uint32)), f"rank {rank}"
    if space == "l2":
        assert r_ref[0, 0] == 5 and r_ref[0, 1] == n // 2 + 3 and d_ref[0, 0].view(np.uint32) == 0
