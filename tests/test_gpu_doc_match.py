"""Substring matching on the GPU, through the C ABI (codd_knn_set_documents_host / codd_knn_match_documents).  The
expected bitmap of every needle is Python's `needle in doc`, bit for bit over the row slots, with every bit at or above the count
zero; the expected result of a search under a bitmap is MaskedOracleEngine's on the same mask, ids and distances bit for bit.  The
arena layout the tile cases rely on is the header's: document r starts at arena offset (bytes of the documents before it) + r."""

import numpy as np
import pytest

from codd_query_engine_amd import native
from tests._masked_oracle_engine import MaskedOracleEngine

pytestmark = pytest.mark.gpu

DIM = 64


@pytest.fixture(scope="module")
def Index():
    import torch

    assert torch.cuda.is_available()
    from codd_query_engine_amd.knn_index import DeviceKnnIndex

    return DeviceKnnIndex


def build(Index, docs, seed=0):
    """(index, checker engine, raw vectors) holding one random row per document."""
    n = len(docs)
    raw = np.random.default_rng(seed).standard_normal((n, DIM)).astype(np.float32)
    ix = Index(DIM)
    ix.upsert(np.arange(n, dtype=np.int64), raw)
    ix.set_documents(docs)
    ref = MaskedOracleEngine(DIM)
    ref.upsert(np.arange(n, dtype=np.int64), raw)
    assert ix.stat("docs_valid") == 1 and ix.stat("doc_bytes") == sum(len(d or b"") for d in docs) + n
    return ix, ref, raw


def matched(ix, needle: bytes) -> np.ndarray:
    """bool over the row slots from the device words; asserts the bits at or above the count are zero."""
    n = ix.count()
    words = ix.match_documents(needle).cpu().numpy().view(np.uint32)
    assert words.shape == ((n + 31) // 32,)
    bits = np.unpackbits(words.view(np.uint8), bitorder="little").astype(bool)
    assert not bits[n:].any(), "bits at or above the count must be zero"
    return bits[:n]


def contains(docs, needle: bytes) -> np.ndarray:
    return np.array([needle in (d or b"") for d in docs], dtype=bool)


def check(ix, docs, needle: bytes) -> np.ndarray:
    got, want = matched(ix, needle), contains(docs, needle)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (needle[:40], len(needle), bad[:8], [docs[i] if len(docs[i] or b"") < 80 else len(docs[i]) for i in bad[:4]])
    return got


def random_docs(n, seed):
    """Short documents over a five-letter alphabet (every short needle occurs often, at every alignment); the first and the last
    are empty, so are some in between, and some are None."""
    rng = np.random.default_rng(seed)
    docs = []
    for i in range(n):
        length = int(rng.integers(0, 41))
        docs.append(None if i % 97 == 50 else bytes(rng.choice(list(b"abcx "), size=length).astype(np.uint8)))
    docs[0] = docs[-1] = b""
    docs[7] = b""
    return docs


@pytest.fixture(scope="module")
def corpus(Index):
    docs = random_docs(3001, seed=1)                          # 3001: no multiple of 32
    long_needle = bytes(np.random.default_rng(2).choice(list(b"abcx "), size=native.MAX_NEEDLE).astype(np.uint8))
    docs[10] = b"Q" + b"abc" * 5                              # a needle at a document's first byte ...
    docs[11] = b"abc" * 5 + b"W"                              # ... and at its last
    docs[12] = b"aaaa"
    docs[13] = b"aaa"
    docs[20], docs[21] = b"x@", b"#x"                         # "@#" exists only across two adjacent documents
    docs[30] = b"cc" + long_needle + b"x"                     # holds the longest needle there is
    docs[31] = long_needle[:-1]                               # ... and one byte short of it
    docs[40] = b"exactly this document"
    if (sum(len(d or b"") for d in docs) + len(docs)) % 16 == 0:
        docs[41] = (docs[41] or b"") + b"c"
    ix, ref, raw = build(Index, docs)
    assert ix.stat("doc_bytes") % 16 != 0, "an arena whose size is no multiple of 16"
    yield ix, ref, raw, docs, long_needle
    ix.close()


# (b"a", b" ": several matches in most documents and in most 16-byte chunks — the lane's remembered document and the bit test)
NEEDLES = [b"a", b" ", b"ab", b"abc", b"xabc", b"abcx ", b"aaa", b"aaaa", b"Q", b"W", b"Qabc", b"bcW", b"exactly this document",
           b"exactly this document!", b"c a b c a x"]


@pytest.mark.parametrize("needle", NEEDLES, ids=[n.decode().replace(" ", "_") for n in NEEDLES])
def test_the_bitmap_is_needle_in_doc_bit_for_bit(corpus, needle):
    ix, _, _, docs, _ = corpus
    before = ix.stat("doc_matches")
    got = check(ix, docs, needle)
    assert ix.stat("doc_matches") == before + 1
    if needle == b"aaa":
        assert got[12] and got[13]                            # "aaa" in "aaaa": overlapping matches in one document
    if needle == b"aaaa":
        assert got[12] and not got[13]
    if needle in (b"Q", b"Qabc"):
        assert got[10] and got.sum() == 1                     # at the document's first byte
    if needle in (b"W", b"bcW"):
        assert got[11] and got.sum() == 1                     # at its last
    if needle == b"exactly this document":
        assert got[40] and got.sum() == 1                     # the needle is the whole document
    if needle == b"exactly this document!":
        assert not got.any()


def test_the_longest_needle_and_one_longer_than_every_short_document(corpus):
    ix, _, _, docs, long_needle = corpus
    assert len(long_needle) == native.MAX_NEEDLE
    got = check(ix, docs, long_needle)
    assert got[30] and not got[31] and got.sum() == 1
    got = check(ix, docs, long_needle[:200])                  # longer than all but two documents
    assert got[30] and got[31] and got.sum() == 2
    with pytest.raises(native.NativeLibraryError, match="-22"):
        ix.match_documents(long_needle + b"a")


def test_a_needle_across_two_documents_does_not_match_and_no_match_means_nothing_comes_back(corpus):
    ix, _, _, docs, _ = corpus
    assert docs[20].endswith(b"@") and docs[21].startswith(b"#")
    got = check(ix, docs, b"@#")
    assert not got.any()                                      # an all-zero bitmap ...
    q = np.random.default_rng(3).standard_normal((3, DIM)).astype(np.float32)
    dist, rows = ix.search_masked_dev(q, ix.match_documents(b"@#"), 5)
    assert (rows == -1).all() and np.isinf(dist).all()        # ... and an empty search result
    assert ix.stat("last_mask_rows") == 0


def test_the_search_under_a_matched_bitmap_is_the_oracles_under_the_same_mask(corpus):
    ix, ref, _, docs, _ = corpus
    q = np.random.default_rng(4).standard_normal((5, DIM)).astype(np.float32)
    for needle in (b"abc", b"Q", b"x a"):
        mask = contains(docs, needle)
        d_ref, r_ref = ref.search_masked(q, mask, 10)
        dist, rows = ix.search_masked_dev(q, ix.match_documents(needle), 10)
        assert np.array_equal(rows, r_ref) and np.array_equal(dist, d_ref), needle
        assert ix.stat("last_mask_rows") == int(mask.sum())


@pytest.mark.parametrize("where", ["T-1", "T-len+1", "T"])
def test_a_match_that_straddles_a_tile_and_a_document_longer_than_two_tiles(Index, where):
    needle = b"NEEDLE!"
    probe = Index(DIM)
    T = probe.stat("doc_tile_bytes")
    probe.close()
    start = {"T-1": T - 1, "T-len+1": T - len(needle) + 1, "T": T}[where]
    # document 0 fills the arena up to start - 4 (its separator included), document 1 puts the needle at `start`
    docs = [b"f" * (start - 4), b"ggg" + needle + b"hh", b"k" * (2 * T + 100) + needle + b"k" * 50, b"NEEDLE", b"", needle, b"k" * T, needle[1:]]
    assert len(docs[0]) + 1 + 3 == start and len(docs[2]) > 2 * T
    ix, _, _ = build(Index, docs)
    got = check(ix, docs, needle)
    assert got.tolist() == [False, True, True, False, False, True, False, False]
    check(ix, docs, b"k")
    check(ix, docs, b"fg")                                    # nowhere: the separator stands between them
    check(ix, docs, b"f" * 256)                               # a long run of candidates, every pre-test passes
    check(ix, docs, b"k" * 255 + b"N")
    ix.close()


@pytest.mark.parametrize("n", [1, 31, 32, 33, 100])
def test_counts_around_a_word(Index, n):
    docs = [bytes([97 + (i * 7 + j) % 5 for j in range(i % 6)]) for i in range(n)]   # document 0 is empty
    docs[-1] = b"last" if n > 1 else b"a"
    ix, ref, _ = build(Index, docs, seed=n)
    for needle in (b"a", b"last", b"cd", b"zz"):
        got = check(ix, docs, needle)
        q = np.random.default_rng(n).standard_normal((2, DIM)).astype(np.float32)
        d_ref, r_ref = ref.search_masked(q, got, 4)
        dist, rows = ix.search_masked_dev(q, ix.match_documents(needle), 4)
        assert np.array_equal(rows, r_ref) and np.array_equal(dist, d_ref), (n, needle)
    ix.close()


def test_empty_documents_only(Index):
    docs = [b"", None, b"", b""]
    ix, _, _ = build(Index, docs)
    assert ix.stat("doc_bytes") == 4
    assert not check(ix, docs, b"a").any()
    ix.close()


def test_a_deleted_slot_is_matched_as_it_stands_and_never_returned(Index):
    docs = random_docs(500, seed=5)
    docs[100] = b"only here: ZED"
    docs[101] = b"and here: ZED too"
    ix, ref, raw = build(Index, docs)
    ix.delete(np.array([100, 3], dtype=np.int64))
    ref.delete(np.array([100, 3], dtype=np.int64))
    assert ix.stat("docs_valid") == 1, "a delete leaves the snapshot valid"
    got = check(ix, docs, b"ZED")
    assert got[100] and got[101] and got.sum() == 2           # matching is slot-addressed
    q = raw[[100, 101]]
    dist, rows = ix.search_masked_dev(q, ix.match_documents(b"ZED"), 3)
    d_ref, r_ref = ref.search_masked(q, got, 3)
    assert np.array_equal(rows, r_ref) and np.array_equal(dist, d_ref)
    assert rows.tolist() == [[101, -1, -1], [101, -1, -1]] and ix.stat("last_mask_rows") == 1
    ix.close()


def test_a_stale_or_absent_snapshot_is_einval(Index):
    docs = random_docs(64, seed=6)
    raw = np.random.default_rng(6).standard_normal((65, DIM)).astype(np.float32)
    ix = Index(DIM)
    ix.upsert(np.arange(64, dtype=np.int64), raw[:64])
    assert ix.stat("docs_valid") == 0
    with pytest.raises(native.NativeLibraryError, match="-22"):
        ix.match_documents(b"a")                              # absent
    ix.set_documents(docs)
    check(ix, docs, b"a")
    ix.upsert(np.array([5], dtype=np.int64), raw[5:6])        # an overwrite makes it stale, as it makes an IVF layout stale
    assert ix.stat("docs_valid") == 0
    with pytest.raises(native.NativeLibraryError, match="-22"):
        ix.match_documents(b"a")
    ix.set_documents(docs)
    check(ix, docs, b"a")
    ix.upsert(np.array([64], dtype=np.int64), raw[64:65])     # so does an append
    with pytest.raises(native.NativeLibraryError, match="-22"):
        ix.match_documents(b"a")
    with pytest.raises(native.NativeLibraryError, match="-22"):
        ix.set_documents(docs)                                # 64 documents for 65 rows
    docs.append(b"the new one")
    ix.set_documents(docs)
    assert check(ix, docs, b"new")[64]
    ix.delete(np.array([1], dtype=np.int64))
    assert ix.stat("docs_valid") == 1
    assert ix.compact() == 64                                 # rows moved: stale
    assert ix.stat("docs_valid") == 0
    with pytest.raises(native.NativeLibraryError, match="-22"):
        ix.match_documents(b"a")
    ix.close()


def test_a_rejected_snapshot_changes_nothing(Index):
    docs = [b"alpha", b"beta", b"gamma"]
    ix, _, _ = build(Index, docs)
    with pytest.raises(native.NativeLibraryError, match="0x00"):
        ix.set_documents([b"alpha", b"be\x00ta", b"gamma"])
    with pytest.raises(native.NativeLibraryError, match="-22"):
        ix.set_documents([b"alpha", b"beta"])
    with pytest.raises(native.NativeLibraryError, match="0x00"):
        ix.match_documents(b"a\x00")
    for needle in (b"", b"a" * (native.MAX_NEEDLE + 1)):
        with pytest.raises(native.NativeLibraryError, match="needle_len out of range"):
            ix.match_documents(needle)
    assert ix.stat("docs_valid") == 1
    assert check(ix, docs, b"eta").tolist() == [False, True, False]
    ix.close()
