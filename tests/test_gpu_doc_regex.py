"""Regular expressions on the GPU: codd_knn_match_documents_dfa / doc_regex_kernel through DeviceKnnIndex and through
the façade.  The bitmap must equal `re.search` over the same documents bit for bit; every device case asserts that
stat("doc_regex_matches") grew, so a silent host fallback cannot pass."""

import re

import numpy as np
import pytest

from codd_query_engine_amd import KnnClient, ivf, native
from codd_query_engine_amd.knn_index import DeviceKnnIndex
from codd_query_engine_amd.regex_dfa import compile_search_dfa
from codd_query_engine_amd.sharded import ShardedSearcher
from oracle import knn_oracle as o
from tests._regex_cases import MUST_COMPILE, PatternGenerator

pytestmark = pytest.mark.gpu

DIM = 16


def utf8(doc):
    return None if doc is None else doc.encode("utf-8", "surrogatepass")


def index_of(docs, seed=0):
    rows = np.random.default_rng(seed).standard_normal((len(docs), DIM)).astype(np.float32)
    ix = DeviceKnnIndex(DIM, "f32", "cuda:0")
    ix.upsert(np.arange(len(docs), dtype=np.int64), rows)
    ix.set_documents([utf8(d) for d in docs])
    return ix, rows


def device_bits(ix, pattern, ascii_documents=False):
    dfa = compile_search_dfa(pattern, ascii_documents)
    assert dfa is not None, pattern
    before = ix.stat("doc_regex_matches")
    words = ix.match_documents_dfa(dfa).cpu().numpy().view(np.uint32)
    assert ix.stat("doc_regex_matches") == before + 1
    n = ix.count()
    assert words.shape[0] == (n + 31) // 32
    bits = np.unpackbits(words.view(np.uint8), bitorder="little")
    assert not bits[n:].any(), "bits at or above the count are zero"
    return bits[:n].astype(bool)


def host_bits(docs, pattern):
    search = re.compile(pattern).search
    return np.array([search(d or "") is not None for d in docs], dtype=bool)   # (the engine sees None as an empty document)


def corpus(ascii_only: bool, longest: int = 1500):
    """About 2,000 documents: store-format lines, empty and None documents, non-ASCII ones, very short and very long ones (up to
    `longest` bytes of filler), and random strings over the generator's alphabet."""
    gen = PatternGenerator(7)
    words = ["latency", "lattncy", "http_requests_total", "http_errors_count", "http_total", "queue", "rate", "LATENCY", "xy", "12", "a1234b", "abab", "cdcd"]
    if not ascii_only:
        words += ["Größe", "日本語", "é", "\U0001F600!", "K", "ſ", "a\x1cb"]
    docs = []
    for i in range(2000):
        m = i % 10
        if m == 0:
            docs.append(None if i % 20 else "")
        elif m < 5:
            docs.append(f"{words[i % len(words)]} of service {i} | Unit: {words[(i * 5 + 1) % len(words)]} | Category: {words[(i * 7 + 3) % len(words)]}")
        elif m < 7:
            docs.append(words[(i * 3) % len(words)] + ("\n" if i % 3 == 0 else ""))
        elif m == 7:
            d = gen.document()
            docs.append(d.replace("é", "e") if ascii_only else d)
        elif m == 8:
            docs.append("ab"[i % 2])
        else:
            docs.append(("x" * (i * 13 % longest)) + words[i % len(words)] + ("-" * (i % 50)))
    return docs


@pytest.fixture(scope="module")
def mixed():
    docs = corpus(False)
    ix, rows = index_of(docs)
    yield ix, rows, docs
    ix.close()


@pytest.fixture(scope="module")
def plain():
    docs = corpus(True)
    assert all(d is None or d.isascii() for d in docs)
    ix, rows = index_of(docs)
    yield ix, rows, docs
    ix.close()


@pytest.mark.parametrize("pattern,ascii_only", MUST_COMPILE, ids=[p for p, _ in MUST_COMPILE])
def test_the_bitmap_equals_re_search_bit_for_bit(mixed, plain, pattern, ascii_only):
    for ix, _, docs in ([plain] if ascii_only else [mixed, plain]):
        got = device_bits(ix, pattern, ascii_documents=ascii_only)
        want = host_bits(docs, pattern)
        assert np.array_equal(got, want), (pattern, np.flatnonzero(got != want)[:10])


@pytest.fixture(scope="module")
def short():
    """The corpus with its long documents cut to 24 bytes of filler, for the generated patterns: the expected bits come from
    `re`, which backtracks — some generated patterns (`(?:\\n??.??)*?é.`) take `re` minutes on a document of 3,000 characters
    and microseconds on one of 30.  The long documents are checked in the same test against the table walk on the CPU."""
    docs = corpus(False, longest=24)
    ix, rows = index_of(docs)
    yield ix, rows, docs
    ix.close()


def table_walk(dfa, padded):
    """ByteDfa.matches for many documents at once: `padded` is uint8 [documents, longest + 1], each document's bytes, its 0x00
    and zeros behind it (the separator leaves ACCEPT or REJECT, which absorb, so the zeros change nothing)."""
    class_of, table = np.frombuffer(dfa.class_of, dtype=np.uint8), np.frombuffer(dfa.next, dtype=np.uint8)
    state = np.full(padded.shape[0], dfa.start, dtype=np.int64)
    for column in padded.T:
        state = table[state * dfa.nclasses + class_of[column]].astype(np.int64)
    return state == dfa.accept


@pytest.mark.parametrize("seed", [99, 100, 101])
def test_three_hundred_generated_patterns_a_hundred_at_a_time(short, mixed, seed):
    """Against `re` over the corpus of short documents, and — `re` being too slow there — against the table walk itself
    (ByteDfa.matches, which tests/test_regex_dfa.py pins to `re`) over the long documents of the full corpus."""
    ix, _, docs = short
    ix_long, _, docs_long = mixed
    long_ones = np.array([r for r, d in enumerate(docs_long) if d is not None and len(d) > 100])
    raw = [utf8(docs_long[r]) for r in long_ones]
    assert len(raw) > 150 and max(map(len, raw)) > 1400
    padded = np.zeros((len(raw), max(map(len, raw)) + 1), dtype=np.uint8)
    for row, b in zip(padded, raw):
        row[: len(b)] = np.frombuffer(b, dtype=np.uint8)
    gen = PatternGenerator(seed)
    some = 0
    for n in range(100):
        pattern = gen.pattern()
        got, want = device_bits(ix, pattern), host_bits(docs, pattern)
        assert np.array_equal(got, want), (pattern, np.flatnonzero(got != want)[:10])
        some += bool(want.any() and not want.all())
        dfa = compile_search_dfa(pattern, False)
        walked = table_walk(dfa, padded)
        assert [bool(w) for w in walked[:3]] == [dfa.matches(b) for b in raw[:3]], pattern
        got_long = device_bits(ix_long, pattern)[long_ones]
        assert np.array_equal(got_long, walked), (pattern, long_ones[np.flatnonzero(got_long != walked)[:10]])
    assert some > 30, "patterns that split the corpus"


@pytest.mark.parametrize("n", [1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 700])
def test_document_counts_around_the_ballot_words_and_the_run(n):
    probe_docs = ["b"] * n
    for at in {0, n - 1, n // 2, max(n - 33, 0), min(31, n - 1), min(32, n - 1)}:
        probe_docs[at] = "a%d" % at
    ix, _ = index_of(probe_docs)
    assert 256 <= ix.stat("doc_regex_run_docs") < 257, "257 and 700 documents are more than one workgroup's run"
    for pattern in (r"^a\d+$", "b", "^$", "c|^a"):
        assert np.array_equal(device_bits(ix, pattern, True), host_bits(probe_docs, pattern)), (n, pattern)
    ix.close()


def test_segment_edges():
    probe = DeviceKnnIndex(DIM, "f32", "cuda:0")
    T = probe.stat("doc_regex_tile_bytes")
    probe.close()
    assert T % 16 == 0 and T >= 1024
    docs = []
    used = 0

    def add(doc):
        nonlocal used
        docs.append(doc)
        used += len(doc) + 1

    add("p" * (T - 8))                               # ends inside segment 0; next document starts at T - 7
    add("q" * 6 + "Z" + "r" * 5)                      # "Z" at arena byte T - 1: the last byte of segment 0; ends in segment 1
    start = used
    add("s" * (2 * T - (start % T)) + "Z" + "t" * 3)  # longer than two segments; its "Z" is the FIRST byte of a segment
    assert (start + 2 * T - (start % T)) % T == 0
    start = used
    add("u" * (T - (start % T) - 1) + "a")            # "a" is a segment's last byte, so its separator is the next segment's first: `a$`
    assert (used - 1) % T == 0
    add("a\n")
    add("v" * (3 * T) + "a")                          # longer than two segments, decided by its last byte
    add("")
    add("Z")
    ix, _ = index_of(docs)
    for pattern in ("Z", "Zr", "sZt", "a$", r"a\Z", "^u+a$", "^v+a$", "^q+Z", "t{3}$", "^$", "Z$", "p$"):
        got, want = device_bits(ix, pattern), host_bits(docs, pattern)
        assert np.array_equal(got, want), (pattern, got, want)
    ix.close()


def test_patterns_that_kill_every_lane_at_once_match_everything_or_nothing(plain):
    ix, _, docs = plain
    for pattern, share in ((r"^~never", 0.0), (r"^", 1.0), (r"x*", 1.0), (r"~~~", 0.0), (r"[^\x01]*$", None)):
        got, want = device_bits(ix, pattern, True), host_bits(docs, pattern)
        assert np.array_equal(got, want), pattern
        if share is not None:
            assert want.mean() == share, pattern


def test_einval_leaves_the_words_and_the_stats_alone():
    import torch

    docs = ["ab", "cd", "ab cd"]
    ix, rows = index_of(docs)
    good = compile_search_dfa("a.*d", False)
    stats = lambda: (ix.stat("doc_regex_matches"), ix.stat("doc_matches"), ix.stat("workspaces"))   # noqa: E731
    ix.match_documents_dfa(good)
    before = stats()
    lib, h = ix._lib, ix._h
    words = torch.full((1,), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")

    def call(class_of=good.class_of, nxt=good.next, nstates=good.nstates, nclasses=good.nclasses, start=good.start, accept=good.accept, nwords=1):
        return lib.codd_knn_match_documents_dfa(h, bytes(class_of), bytes(nxt), nstates, nclasses, start, accept, words.data_ptr(), nwords, None)

    bad_next = bytearray(good.next)
    bad_next[3] = good.nstates
    bad_class = bytearray(good.class_of)
    bad_class[200] = good.nclasses
    leaky = bytearray(good.next)
    leaky[good.accept * good.nclasses] = good.start
    cases = [dict(nxt=bad_next), dict(class_of=bad_class), dict(nxt=leaky), dict(start=good.nstates), dict(start=-1), dict(accept=good.nstates),
             dict(nstates=0), dict(nstates=256), dict(nclasses=0), dict(nclasses=257), dict(nwords=2), dict(nwords=0),
             dict(nxt=bytes(native.MAX_DFA_TABLE + 64), nstates=129, nclasses=64, accept=0, start=0)]
    for kw in cases:
        assert call(**kw) == -22, kw
    assert stats() == before and int(words.cpu()[0]) == 0x5A5A5A5A
    # a stale snapshot, then an absent one
    ix.upsert(np.array([3], dtype=np.int64), rows[:1])
    assert call(nwords=1) == -22 and "snapshot" in native.last_error()
    fresh = DeviceKnnIndex(DIM, "f32", "cuda:0")
    fresh.upsert(np.arange(3, dtype=np.int64), rows)
    with pytest.raises(native.NativeLibraryError):
        fresh.match_documents_dfa(good)
    assert fresh.stat("doc_regex_matches") == 0 and stats() == before and int(words.cpu()[0]) == 0x5A5A5A5A
    fresh.close()
    ix.close()


def masked_oracle(rows, q, keep, k):
    keep = np.flatnonzero(keep)
    d, i = o.search(o.normalize_rows(rows[keep]), "f32", o.normalize_rows(q), k)
    return d, np.where(i >= 0, keep[np.maximum(i, 0)], -1)


def host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def test_searches_under_a_regex_bitmap_equal_the_oracle_under_the_same_mask_and_a_deleted_slot_is_never_returned(mixed):
    ix, rows, docs = mixed
    q = np.random.default_rng(5).standard_normal((3, DIM)).astype(np.float32)
    pattern = r"^http_.*_(total|count)( |$)"
    keep = host_bits(docs, pattern)
    assert 20 < keep.sum() < len(docs) // 2
    bits = ix.match_documents_dfa(compile_search_dfa(pattern, False))
    d_ref, r_ref = masked_oracle(rows, q, keep, 8)
    dist, got = ix.search_masked_dev(q, bits, 8)
    assert np.array_equal(got, r_ref) and np.array_equal(dist, d_ref)
    dd, rr = ShardedSearcher(ix, row_base=0).search(q, 8, allow=bits, allow_global=True)
    assert np.array_equal(host(rr), r_ref) and np.array_equal(host(dd), d_ref)
    # a deleted slot is matched as it stands and never returned
    gone = int(r_ref[0, 0])
    ix.delete(np.array([gone], dtype=np.int64))
    assert device_bits(ix, pattern)[gone], "slot-addressed: the dead slot's document still matches"
    keep[gone] = False
    d_ref, r_ref = masked_oracle(rows, q, keep, 8)
    dist, got = ix.search_masked_dev(q, ix.match_documents_dfa(compile_search_dfa(pattern, False)), 8)
    assert gone not in got and np.array_equal(got, r_ref) and np.array_equal(dist, d_ref)


def test_an_ivf_search_takes_a_regex_bitmap():
    docs = [f"metric_{i}_total" if i % 3 else f"metric_{i}" for i in range(600)]
    ix, rows = index_of(docs, seed=3)
    q = np.random.default_rng(6).standard_normal((2, DIM)).astype(np.float32)
    bits = ix.match_documents_dfa(compile_search_dfa(r"_[0-9]*[05]_total$", True))
    keep = host_bits(docs, r"_[0-9]*[05]_total$")
    ivf.build_ivf(ix, 4, iters=2)
    dd, rr = ivf.search_ivf(ix, q, 5, 4, allow=bits)   # every list probed: exact
    d_ref, r_ref = masked_oracle(rows, q, keep, 5)
    assert np.array_equal(host(rr), r_ref) and np.array_equal(host(dd), d_ref)
    ix.close()


FACADE_DOCS = [None if i % 9 == 8 else "" if i % 31 == 30 else f"http_{'requests' if i % 2 else 'errors'}_{'total' if i % 3 else 'count'} of service {i} | Unit: "
               f"{'Größe' if i % 7 == 0 else 'ms'}" for i in range(150)]
FACADE_FILTERS = [
    {"$regex": r"^http_.*_(total|count) "},
    {"$not_regex": r"errors_\w*"},                       # (\w on a corpus with "Größe": the host's)
    {"$not_regex": r"errors_[a-z]*"},
    {"$and": [{"$regex": r"service [0-9]*7 "}, {"$not_regex": "count"}, {"$contains": "http"}]},
    {"$or": [{"$regex": r"Gr.ße$"}, {"$regex": r"^$"}]},
    {"$regex": r"e*"},                                   # matches "": records without a document must stay out
    {"$not_regex": r"x*$"},
]


def filled_collection():
    col = KnnClient(device="cuda:0", document_regex=True).get_or_create_collection("regex")
    vecs = np.random.default_rng(21).standard_normal((len(FACADE_DOCS), DIM)).astype(np.float32)
    col.upsert(ids=[f"id{i}" for i in range(len(FACADE_DOCS))], embeddings=vecs, documents=FACADE_DOCS,
               metadatas=[{"kind": "gauge" if i % 2 else "counter"} for i in range(len(FACADE_DOCS))])
    return col


def test_the_facade_on_the_device_equals_the_same_collection_on_the_host_path():
    on_device = filled_collection()
    on_host = filled_collection()
    on_host._has_device_documents = lambda: False   # the same engine, every filter evaluated by the façade itself (search_masked)
    engine = on_device._engine
    q = np.random.default_rng(22).standard_normal((3, DIM)).astype(np.float32)
    for wd in FACADE_FILTERS:
        for where in (None, {"kind": "gauge"}):
            a = on_device.query(query_embeddings=q, n_results=6, where=where, where_document=wd)
            b = on_host.query(query_embeddings=q, n_results=6, where=where, where_document=wd)
            assert a["ids"] == b["ids"] and a["distances"] == b["distances"], (wd, where)
            assert on_device.get(where_document=wd)["ids"] == on_host.get(where_document=wd)["ids"]
    assert engine.stat("doc_regex_matches") >= 6 and on_host._engine.stat("doc_regex_matches") == 0
    # a cached pattern launches nothing; a literal pattern is a needle; a pattern outside the subset never reaches the kernel
    launches, needles = engine.stat("doc_regex_matches"), engine.stat("doc_matches")
    on_device.query(query_embeddings=q, where_document={"$regex": r"^http_.*_(total|count) "})
    assert engine.stat("doc_regex_matches") == launches
    on_device.query(query_embeddings=q, where_document={"$regex": r"http_requests"})
    assert (engine.stat("doc_regex_matches"), engine.stat("doc_matches")) == (launches, needles + 1)
    out = on_device.query(query_embeddings=q, where_document={"$regex": r"(requests|errors)_\1"})
    assert out["ids"] == [[], [], []] and engine.stat("doc_regex_matches") == launches
    on_device.query(query_embeddings=q, where_document={"$regex": r"_(total|count) of service 1[0-9] "})
    assert engine.stat("doc_regex_matches") == launches + 1
    assert ("re", r"http_requests") in on_device._doc_bits_cache and len(on_device._doc_bits_cache) <= 32
