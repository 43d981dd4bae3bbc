"""codd_knn_slice_mask on the GPU: a shard's words out of a mask over global rows, against numpy bit slicing word
for word — and the composition it exists for: two shards of one corpus in one process, cut at a row that is no multiple of 32, one
global mask sliced per shard by the kernel, search_keys_masked_dev on each shard, merge_shards == the masked search of the unsharded
index, bit for bit; the same with an IVF layout per shard, probed exhaustively."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

G = 1_000_003                       # 31,250 * 32 + 3: the last global word is partial


def words_of(mask: np.ndarray) -> np.ndarray:
    packed = np.packbits(mask, bitorder="little")
    words = np.zeros((mask.shape[0] + 31) // 32 * 4, dtype=np.uint8)
    words[: packed.shape[0]] = packed
    return words.view("<u4").copy()


@pytest.fixture(scope="module")
def env():
    import torch

    assert torch.cuda.is_available()
    from codd_query_engine_amd import knn_index

    bits = np.random.default_rng(17).random(G) < 0.5
    words = words_of(bits)
    words[-1] |= np.uint32(0xFFFFFFFF) << np.uint32(G % 32)          # garbage above global_rows in the last word: to be ignored
    dev = torch.from_numpy(words.view(np.int32)).to("cuda:0")
    return torch, knn_index, bits, dev


def expect(bits: np.ndarray, row_base: int, count: int) -> np.ndarray:
    local = np.zeros(count, dtype=bool)
    have = bits[row_base : row_base + count]
    local[: have.shape[0]] = have
    return words_of(local)


@pytest.mark.parametrize("row_base", [0, 1, 31, 32, 33, 999_990])
def test_slices_equal_numpy_bit_slicing_word_for_word(env, row_base):
    torch, knn_index, bits, dev = env
    left = G - row_base
    counts = {left - 7 if left > 7 else 1, left, left + 40,         # ends inside, at, and past the global end
              min(left, 1), min(left, 32), min(left, 65), min(left, 100_001)}
    for count in sorted(counts):
        got = knn_index.slice_mask(dev, G, row_base, count).cpu().numpy().view(np.uint32)
        want = expect(bits, row_base, count)
        assert got.shape == want.shape and np.array_equal(got, want), (row_base, count, np.flatnonzero(got != want)[:8])


def test_edges(env):
    torch, knn_index, bits, dev = env
    assert knn_index.slice_mask(dev, G, 5, 0).shape == (0,)                                        # nothing to write
    assert not knn_index.slice_mask(dev, G, G, 70).any() and not knn_index.slice_mask(dev, G, G + 1_000, 70).any()   # wholly past the end
    empty = torch.zeros((0,), dtype=torch.int32, device="cuda:0")
    assert not knn_index.slice_mask(empty, 0, 0, 70).any()                                         # no global row at all
    with pytest.raises(ValueError):
        knn_index.slice_mask(dev[:-1], G, 0, 10)                                                   # words and global_rows disagree
    with pytest.raises(ValueError):
        knn_index.slice_mask(dev.cpu(), G, 0, 10)


@pytest.mark.parametrize("use_ivf", [False, True], ids=["flat", "ivf"])
def test_two_shards_under_one_global_mask_equal_the_unsharded_masked_search(env, use_ivf):
    torch, knn_index, _, _ = env
    from codd_query_engine_amd import ivf
    from codd_query_engine_amd.sharded import ShardedSearcher

    n, d, k, cut, nlist = 6_011, 128, 10, 2_605, 8                   # 2,605 = 81 * 32 + 13
    rng = np.random.default_rng(18)
    raw = rng.standard_normal((n, d)).astype(np.float32)
    raw[cut + 9] = raw[40]                                            # an exact tie across the cut, both rows allowed
    q = rng.standard_normal((7, d)).astype(np.float32)
    q[0] = raw[40]
    mask = rng.random(n) < 0.3
    mask[[40, cut + 9]] = True
    dead = rng.choice(n, size=n // 10, replace=False)
    dead = dead[(dead != 40) & (dead != cut + 9)]
    whole = knn_index.DeviceKnnIndex(d)
    whole.upsert(np.arange(n, dtype=np.int64), raw)
    whole.delete(dead)
    d_ref, r_ref = whole.search_masked(q, mask, k)
    assert r_ref[0, 0] == 40 and r_ref[0, 1] == cut + 9
    global_words = torch.from_numpy(words_of(mask).view(np.int32)).to(whole.device)

    parts, engines = [], []
    for lo, hi in ((0, cut), (cut, n)):
        s = knn_index.DeviceKnnIndex(d)
        s.upsert(np.arange(hi - lo, dtype=np.int64), raw[lo:hi])
        if use_ivf:
            ivf.build_ivf(s, nlist, iters=2)
        s.delete(dead[(dead >= lo) & (dead < hi)] - lo)
        eng = ivf.IvfShardEngine(s, nprobe=nlist) if use_ivf else s
        local = eng.slice_mask(global_words, n, lo)
        assert np.array_equal(local.cpu().numpy().view(np.uint32), words_of(mask[lo:hi]))
        parts.append(eng.search_keys_masked_dev(q, local, k, lo))
        engines.append((lo, s, eng))
    _, d_got, r_got = knn_index.merge_shards(torch.cat(parts, dim=0), 2, k)
    assert np.array_equal(r_got.cpu().numpy(), r_ref) and np.array_equal(d_got.cpu().numpy(), d_ref)

    # ... and each shard through ShardedSearcher (one rank: no collective): the global mask, device words and host bool, and the
    # shard-local host mask give the shard's own keys
    for (lo, s, eng), part in zip(engines, parts):
        want = knn_index.merge_keys(part, k)
        searcher = ShardedSearcher(eng, row_base=lo)
        hi = lo + s.count()
        for allow, is_global in ((global_words, True), (mask, True), (mask[lo:hi], False), (words_of(mask[lo:hi]), False)):
            dd, rr = searcher.search(q, k, allow=allow, allow_global=is_global)
            assert torch.equal(rr, want[2]) and torch.equal(dd, want[1])
        dd, rr = searcher.search_async(torch.from_numpy(q).to(s.device), k, allow=global_words, allow_global=True).result()
        assert torch.equal(rr, want[2]) and torch.equal(dd, want[1])
        with pytest.raises(ValueError):
            searcher.search(q, k, scopes=np.zeros(7, dtype=np.uint32), allow=mask[lo:hi])
    for _, s, _ in engines:
        s.close()
    whole.close()
