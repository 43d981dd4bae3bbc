"""`where_document` $regex / $not_regex above the engine, on the checker engine with search_masked only (the façade's
host path): the opt-in by collection metadata and by KnnClient(document_regex=True), Python's `re.search` as the meaning, the
None-document rule, the malformed forms, persistence of the opt-in and the pass through the store.  Expected ids come from a plain
`re.search` over this file's own documents and the oracle on the rows that pass.  No GPU."""

import re

import numpy as np
import pytest

from codd_query_engine_amd import KnnClient, MetricsSearchClient, MetricsSemanticMetadataStore
from oracle import knn_oracle as o
from tests._masked_oracle_engine import MaskedOracleEngine
from tests.test_where_document_facade import DIM, N, document_of, fill, metadata_of
from tests.test_where_facade import passes as md_passes

OPT_IN = {"codd:document_regex": 1}


def client(**kw):
    return KnnClient(engine_factory=lambda dim: MaskedOracleEngine(dim), **kw)


def passes(doc, wd) -> bool:
    (op, arg), = wd.items()
    if op == "$and":
        return all(passes(doc, w) for w in arg)
    if op == "$or":
        return any(passes(doc, w) for w in arg)
    if op in ("$regex", "$not_regex"):
        hit = doc is not None and re.search(arg, doc) is not None
        return hit if op == "$regex" else not hit
    hit = doc is not None and arg in doc
    return hit if op == "$contains" else not hit


def expected(vecs, docs, q, wd, k, also=lambda i: True):
    keep = [i for i in range(len(docs)) if passes(docs[i], wd) and also(i)]
    if not keep:
        return [], []
    d, i = o.search(o.normalize_rows(vecs[keep]), "f32", o.normalize_rows(q[None, :]), min(k, len(docs)))
    hit = i[0] >= 0
    return [f"id{keep[j]}" for j in i[0][hit]], d[0][hit].tolist()


FILTERS = [
    {"$regex": r"^(latency|HTTP) of service \d+ \|"},
    {"$regex": r"Unit: (rate|queue)"},
    {"$regex": r"service [0-9]*7 "},
    {"$regex": r"(?i)^http"},
    {"$regex": r"Größe|日本語$"},
    {"$regex": r"^$"},                                        # nobody: every document has text, and None is no document
    {"$regex": r"e*"},                                        # matches "": everybody with a document, nobody without
    {"$not_regex": r"e*"},                                    # ... and exactly the records without one
    {"$not_regex": r"\bHTTP\b"},
    {"$and": [{"$regex": r"^[a-z]"}, {"$not_regex": r"rate$"}, {"$contains": "service"}]},
    {"$or": [{"$regex": r"queue of"}, {"$and": [{"$not_contains": "e"}, {"$not_regex": "x"}]}]},
    {"$regex": r"(\w+) \| Unit: \1"},                          # a back-reference: the host's on every engine
]


@pytest.fixture(scope="module", params=["metadata", "client"])
def filled(request):
    if request.param == "metadata":
        col = client().get_or_create_collection("docs", metadata=dict(OPT_IN))
    else:
        col = client(document_regex=True).get_or_create_collection("docs")
    vecs = fill(col)
    return col, vecs, [document_of(i) for i in range(N)]


@pytest.mark.parametrize("wd", FILTERS, ids=[str(i) for i in range(len(FILTERS))])
def test_query_and_get_equal_a_brute_force_restatement(filled, wd):
    col, vecs, docs = filled
    q = np.random.default_rng(2).standard_normal((2, DIM)).astype(np.float32)
    out = col.query(query_embeddings=q, n_results=7, where_document=wd)
    for b in range(2):
        ids, dist = expected(vecs, docs, q[b], wd, 7)
        assert out["ids"][b] == ids and out["distances"][b] == dist
    assert col.get(where_document=wd)["ids"] == [f"id{i}" for i in range(N) if passes(docs[i], wd)]


def test_the_filters_select_somebody_and_the_none_rule_holds(filled):
    col, _, docs = filled
    none_ids = {f"id{i}" for i in range(N) if docs[i] is None}
    assert none_ids
    assert set(col.get(where_document={"$not_regex": "e*"})["ids"]) == none_ids
    assert not none_ids & set(col.get(where_document={"$regex": "e*"})["ids"])
    assert len(col.get(where_document={"$regex": "e*"})["ids"]) == N - len(none_ids)
    assert 0 < len(col.get(where_document=FILTERS[0])["ids"]) < N


def test_an_empty_string_document_is_a_document():
    col = client(document_regex=True).get_or_create_collection("empty")
    col.upsert(ids=["none", "empty", "text", "gone"], embeddings=np.eye(4, DIM, dtype=np.float32), documents=[None, "", "text", ""])
    col.delete(ids=["gone"])
    assert col.get(where_document={"$regex": "^$"})["ids"] == ["empty"]
    assert col.get(where_document={"$not_regex": "^$"})["ids"] == ["none", "text"]
    out = col.query(query_embeddings=np.ones((1, DIM), dtype=np.float32), n_results=4, where_document={"$regex": "x*"})
    assert sorted(out["ids"][0]) == ["empty", "text"]


@pytest.mark.parametrize("where", [{"namespace": "prod:api"}, {"kind": "gauge"}, {"$and": [{"namespace": "prod:billing"}, {"rank": {"$lt": 40}}]}])
def test_where_and_a_regex_must_both_hold(filled, where):
    col, vecs, docs = filled
    q = np.random.default_rng(4).standard_normal((2, DIM)).astype(np.float32)
    wd = {"$regex": r"Category: [a-z]+$"}
    out = col.query(query_embeddings=q, n_results=6, where=where, where_document=wd)
    for b in range(2):
        ids, dist = expected(vecs, docs, q[b], wd, 6, also=lambda i: md_passes(metadata_of(i), where))
        assert out["ids"][b] == ids and out["distances"][b] == dist
    assert col.get(where=where, where_document=wd)["ids"] == [f"id{i}" for i in range(N) if passes(docs[i], wd) and md_passes(metadata_of(i), where)]


def test_without_the_opt_in_nothing_changes():
    col = client().get_or_create_collection("plain")
    fill(col, n=10)
    q = np.zeros((1, DIM), dtype=np.float32)
    for op in ("$regex", "$not_regex"):
        for call in (lambda: col.query(query_embeddings=q, where_document={op: "a.*"}), lambda: col.get(where_document={op: "a.*"})):
            with pytest.raises(ValueError) as e:
                call()
            assert f"unknown operator '{op}'" in str(e.value)
            assert str(e.value).endswith("supported: " + col._WHERE_DOCUMENT_GRAMMAR) and "$regex\"" not in str(e.value).split("supported: ")[1]
    assert col._WHERE_DOCUMENT_GRAMMAR == ('{"$contains": "text"}, {"$not_contains": "text"}, {"$and": [filters]}, {"$or": [filters]}; '
                                           'text is a non-empty str, matched case-sensitively as a substring of the stored document')
    assert not col.document_regex


BAD = [
    ({"$regex": ""}, "non-empty str"),
    ({"$not_regex": ""}, "non-empty str"),
    ({"$regex": 5}, "non-empty str"),
    ({"$regex": None}, "non-empty str"),
    ({"$regex": ["a"]}, "non-empty str"),
    ({"$regex": "("}, "missing ), unterminated subpattern"),
    ({"$not_regex": "a{2,1}"}, "min repeat greater than max repeat"),
    ({"$and": [{"$contains": "a"}, {"$regex": "[z-a]"}]}, "bad character range z-a"),
    ({"$regexp": "a"}, "unknown operator '$regexp'"),
]


@pytest.mark.parametrize("wd,why", BAD, ids=[str(i) for i in range(len(BAD))])
def test_a_malformed_pattern_is_a_value_error_that_names_every_form(filled, wd, why):
    col, _, _ = filled
    q = np.zeros((1, DIM), dtype=np.float32)
    for call in (lambda: col.query(query_embeddings=q, where_document=wd), lambda: col.get(where_document=wd)):
        with pytest.raises(ValueError) as e:
            call()
        msg = str(e.value)
        assert "unsupported where_document filter" in msg and why in msg
        for form in ('{"$contains": "text"}', '{"$not_contains": "text"}', '{"$regex": "pattern"}', '{"$not_regex": "pattern"}', '{"$and": [filters]}',
                     '{"$or": [filters]}'):
            assert form in msg


def test_the_opt_in_survives_persist_and_reload(tmp_path):
    path = str(tmp_path / "store")
    first = client(path=path)
    col = first.get_or_create_collection("kept", metadata=dict(OPT_IN))
    plain = first.get_or_create_collection("plain")
    fill(col, n=20)
    fill(plain, n=20)
    want = col.get(where_document={"$regex": "^latency"})["ids"]
    assert want
    assert first.persist() == 2
    again = client(path=path)
    assert again.get_collection("kept").metadata == OPT_IN and again.get_collection("kept").document_regex
    assert again.get_collection("kept").get(where_document={"$regex": "^latency"})["ids"] == want
    with pytest.raises(ValueError, match="unknown operator"):
        again.get_collection("plain").get(where_document={"$regex": "^latency"})
    # the client's switch covers what it loads, whatever the stored metadata says
    assert client(path=path, document_regex=True).get_collection("plain").get(where_document={"$regex": "^latency"})["ids"] == want


def test_the_store_and_the_search_client_pass_a_regex_through():
    store = MetricsSemanticMetadataStore(client(document_regex=True), collection_name="metrics")
    store.index_metadata("prod:api", {"metric_name": "http_requests_total", "description": "HTTP requests served", "unit": "1"})
    store.index_metadata("prod:api", {"metric_name": "http_errors_count", "description": "HTTP 5xx responses", "category": "errors"})
    store.index_metadata("prod:db", {"metric_name": "db_query_seconds", "description": "Database query latency", "category": "database"})
    search = MetricsSearchClient(store)
    for wd, want in (({"$regex": r"^HTTP .*(served|responses)( \||$)"}, ["http_errors_count", "http_requests_total"]),
                     ({"$regex": r"(?i)category: DATABASE$"}, ["db_query_seconds"]),
                     ({"$not_regex": "HTTP"}, ["db_query_seconds"]),
                     ({"$and": [{"$regex": r"\dxx|served"}, {"$contains": "HTTP"}]}, ["http_errors_count", "http_requests_total"]),
                     ({"$regex": "no such thing"}, [])):
        found = search.search_relevant_metrics("requests", limit=5, where_document=wd)
        assert sorted(h["metric_name"] for h in found) == want, wd
    with pytest.raises(ValueError, match="does not compile"):
        search.search_relevant_metrics("requests", where_document={"$regex": "("})
    plain = MetricsSearchClient(MetricsSemanticMetadataStore(client(), collection_name="metrics"))
    with pytest.raises(ValueError, match="unknown operator"):
        plain.search_relevant_metrics("requests", where_document={"$regex": "HTTP"})


class NoDeviceCalls(MaskedOracleEngine):
    """An engine that has the device path's methods and fails the test when one of them is called."""

    device = "cpu"

    def _never(self, *a, **kw):
        raise AssertionError("the device path was taken")

    set_documents = match_documents = match_documents_dfa = search_masked_dev = _never


@pytest.mark.parametrize("docs,fit,ascii_only", [(["é\x00x", "plain x"], False, False), (["e\x00x", "plain x"], False, True),
                                                 (["éx", "plain x", None], True, False), (["ex", "plain x", None], True, True)])
def test_a_document_that_holds_nul_keeps_the_collection_on_the_host_path_ascii_or_not(docs, fit, ascii_only):
    for opt_in in (False, True):
        col = KnnClient(engine_factory=lambda dim: NoDeviceCalls(dim), document_regex=opt_in).get_or_create_collection("nul")
        col.upsert(ids=[f"id{i}" for i in range(len(docs))], embeddings=np.eye(len(docs), DIM, dtype=np.float32), documents=docs)
        assert col._has_device_documents()
        assert col._documents_fit_device() is fit and col._docs_ascii is ascii_only
        if fit:
            continue
        q = np.ones((1, DIM), dtype=np.float32)
        filters = [{"$contains": "x"}, {"$contains": "\x00x"}] + ([{"$regex": "x$"}, {"$not_regex": "^plain"}] if opt_in else [])
        for wd in filters:
            out = col.query(query_embeddings=q, n_results=3, where_document=wd)
            assert sorted(out["ids"][0]) == sorted(f"id{i}" for i, d in enumerate(docs) if passes(d, wd)), wd
        assert col._engine.calls.count("search_masked") == len(filters)
