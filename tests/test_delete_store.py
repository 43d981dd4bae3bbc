"""delete_metadata / delete_namespace of MetricsSemanticMetadataStore (extensions beyond the reference), on the checker engine
with tombstones, and what MetricsSearchClient finds afterwards.  No GPU."""

import pytest

from codd_query_engine_amd import KnnClient, MetricsSearchClient, MetricsSemanticMetadataStore
from codd_query_engine_amd.errors import ValidationError
from tests._deleting_oracle_engine import DeletingOracleEngine
from tests._oracle_engine import OracleEngine

RECORDS = [
    {"metric_name": "http.latency", "description": "HTTP request latency in milliseconds", "golden_signal_type": "latency"},
    {"metric_name": "http.errors", "description": "HTTP responses with a 5xx status", "golden_signal_type": "errors"},
    {"metric_name": "db.query.time", "description": "Database query execution time", "category": "database"},
    {"metric_name": "network.bandwidth", "description": "Network bandwidth usage", "category": "network"},
]


def make_store():
    store = MetricsSemanticMetadataStore(KnnClient(engine_factory=lambda dim: DeletingOracleEngine(dim)), collection_name="m")
    for ns in ("prod", "staging"):
        for rec in RECORDS:
            store.index_metadata(ns, rec)
    return store


def test_delete_metadata_removes_one_record_and_says_whether_it_existed():
    store = make_store()
    search = MetricsSearchClient(store)
    assert search.search_relevant_metrics("request latency", limit=1, namespace="prod")[0]["metric_name"] == "http.latency"
    assert store.delete_metadata("prod", "http.latency") is True
    assert store.metric_exists("prod", "http.latency") is False and store.metric_exists("staging", "http.latency") is True
    assert store.collection.count() == 7
    assert "http.latency" not in [h["metric_name"] for h in search.search_relevant_metrics("request latency", limit=5, namespace="prod")]
    hits = search.search_relevant_metrics("request latency", limit=8)
    assert len(hits) == 7 and [h["metric_name"] for h in hits].count("http.latency") == 1
    assert [h["metric_name"] for h in search.search_relevant_metrics_batch(["request latency"], limit=1, namespace="staging")[0]] == ["http.latency"]
    # gone already / never there
    assert store.delete_metadata("prod", "http.latency") is False
    assert store.delete_metadata("nobody", "http.latency") is False
    assert store.collection.count() == 7
    # indexing it again brings it back
    assert store.index_metadata("prod", RECORDS[0]) == "prod#http.latency"
    assert store.metric_exists("prod", "http.latency") and store.collection.count() == 8


def test_delete_metadata_validates_the_name_like_index_metadata():
    store = make_store()
    for bad, message in (("", "metric_name cannot be empty"), ("a b", "metric_name contains invalid characters"),
                         ("x" * 256, "metric_name exceeds maximum length of 255 characters")):
        with pytest.raises(ValidationError, match=message):
            store.delete_metadata("prod", bad)
        with pytest.raises(ValidationError, match=message):
            store.index_metadata("prod", {"metric_name": bad})
    assert store.collection.count() == 8


def test_delete_namespace_removes_every_record_of_it_and_counts_them():
    store = make_store()
    search = MetricsSearchClient(store)
    assert store.delete_namespace("staging") == 4
    assert store.collection.count() == 4
    assert search.search_relevant_metrics("request latency", limit=5, namespace="staging") == []
    assert [h["metric_name"] for h in search.search_relevant_metrics("request latency", limit=1)] == ["http.latency"]
    assert len(search.search_relevant_metrics("anything at all", limit=10)) == 4
    assert all(h["namespace"] == "prod" for h in store.search_metadata("time", n_results=10))
    assert store.delete_namespace("staging") == 0 and store.delete_namespace("nobody") == 0
    # more than half of the slots dead: the collection compacted itself, answers unchanged
    assert store.collection._engine.count() == 8
    assert store.delete_metadata("prod", "db.query.time")
    assert store.collection._engine.count() == store.collection.count() == 3
    assert store.delete_metadata("prod", "network.bandwidth") and store.collection.count() == 2
    assert [h["metric_name"] for h in search.search_relevant_metrics("request latency", limit=1)] == ["http.latency"]


def test_store_deletes_need_an_engine_that_can_delete():
    store = MetricsSemanticMetadataStore(KnnClient(engine_factory=lambda dim: OracleEngine(dim)), collection_name="m")
    store.index_metadata("prod", RECORDS[0])
    with pytest.raises(NotImplementedError, match="delete"):
        store.delete_metadata("prod", "http.latency")
    with pytest.raises(NotImplementedError, match="delete"):
        store.delete_namespace("prod")
    assert store.metric_exists("prod", "http.latency")
