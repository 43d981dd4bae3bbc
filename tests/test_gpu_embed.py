"""The hashing embedder on the GPU, through the C ABI (codd_knn_embedder_create / codd_knn_embed_texts_host).  The
expected value is always HashingEmbeddingFunction(dim, weight) on the same texts, compared as uint32 bit patterns with no tolerance;
the output is pre-filled with NaN so that an element the kernel did not write shows.  tests/test_embed_reference.py keeps the fact
that makes the order cases sharp: at dim = 8 an embedder that ignores the order of the additions gets most texts wrong."""

import ctypes

import numpy as np
import pytest

from codd_query_engine_amd import native
from tests import _embed_reference as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available()
    return torch


class Embedder:
    def __init__(self, torch, dim, tw):
        self.torch, self.dim, self.lib = torch, dim, native.load()
        self.h = ctypes.c_void_p()
        native.check(self.lib.codd_knn_embedder_create(ctypes.byref(self.h), 0, dim, tw), "codd_knn_embedder_create")

    def enqueue(self, texts, stream=None):
        """The device tensor the call writes, NaN before it; nothing is read back."""
        torch = self.torch
        blob, offsets = ref.pack(texts)
        out = torch.empty((len(texts), self.dim), dtype=torch.float32, device="cuda:0")
        st = torch.cuda.current_stream() if stream is None else stream
        with torch.cuda.stream(st):   # (the fill and the embedding on one stream)
            out.fill_(float("nan"))
            native.check(self.lib.codd_knn_embed_texts_host(self.h, blob, offsets.ctypes.data, len(texts), out.data_ptr(),
                                                            ctypes.c_void_p(st.cuda_stream)), "codd_knn_embed_texts_host")
        return out

    def __call__(self, texts):
        return self.enqueue(texts).cpu().numpy()

    def close(self):
        native.check(self.lib.codd_knn_embedder_destroy(self.h), "codd_knn_embedder_destroy")


def check(torch, texts, dim, tw):
    e = Embedder(torch, dim, tw)
    try:
        got, want = ref.bits(e(texts)), ref.bits(ref.host(texts, dim, tw))
    finally:
        e.close()
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, (dim, tw, bad[:8], [texts[i][:60] for i in bad[:3]])
    return got


@pytest.mark.parametrize("dim", ref.DIMS)
def test_boundaries(torch, dim):
    texts = ref.boundary_texts()
    assert texts[7:10] == [b"", b"ab", b"cd"] and texts[-1].endswith(b"d")   # neighbours without a separator; a word byte at the arena's end
    got = check(torch, texts, dim, 0.35)
    assert not got[0].any() and not got[7].any(), "a text without a word byte is all +0.0"
    assert (got[1] == got[2]).all(), '"a" and "A"'
    alone = check(torch, [b""], dim, 0.35)
    assert alone.shape == (1, dim) and not alone.any(), "n = 1, an empty text: every element written, +0.0"
    check(torch, [b"ab", b"cd"], dim, 0.35)
    check(torch, [b"", b"", b"z"], dim, 0.35)


@pytest.mark.parametrize("dim,tw", [(8, 0.35), (384, 0.35), (4096, 0.1)])
def test_step_edges(torch, dim, tw):
    check(torch, ref.step_edge_texts(), dim, tw)


@pytest.mark.parametrize("dim,tw", [(8, 0.35), (8, 0.1), (100, 0.35)])
def test_the_additions_happen_in_text_order(torch, dim, tw):
    check(torch, ref.order_texts(), dim, tw)


@pytest.fixture(scope="module")
def coverage():
    texts = ref.coverage_texts()
    seen = set(b"".join(texts))
    assert len(texts) == 1000 and seen == set(range(128))
    return texts


@pytest.mark.parametrize("tw", ref.WEIGHTS)
@pytest.mark.parametrize("dim", ref.DIMS)
def test_every_ascii_byte_every_width_every_weight(torch, coverage, dim, tw):
    check(torch, coverage, dim, tw)


def test_back_to_back_calls_reuse_the_staging_buffer(torch):
    """Five calls of different sizes on one stream, then the same on two streams alternately, all read afterwards: a call may not
    overwrite staged texts, or their device copy, that an earlier call still needs."""
    dim, tw = 384, 0.35
    batches = [ref.random_texts(20 + i, count, ref.ALPHABET_WIDE, longest) for i, (count, longest) in
               enumerate([(300, 400), (3, 10), (1000, 50), (1, 3000), (64, 200)])]
    want = [ref.bits(ref.host(b, dim, tw)) for b in batches]
    e = Embedder(torch, dim, tw)
    try:
        outs = [e.enqueue(b) for b in batches]
        torch.cuda.synchronize()
        for got, expect in zip(outs, want):
            assert np.array_equal(ref.bits(got.cpu().numpy()), expect)
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        outs = [e.enqueue(b, streams[i % 2]) for i, b in enumerate(batches)]
        torch.cuda.synchronize()
        for got, expect in zip(outs, want):
            assert np.array_equal(ref.bits(got.cpu().numpy()), expect)
    finally:
        e.close()


def test_destroy_returns_every_allocation(torch):
    torch.cuda.synchronize()
    before = native.live_allocations()
    e = Embedder(torch, 100, 0.35)
    e(ref.random_texts(3, 50, ref.ALPHABET))
    during = native.live_allocations()
    assert during[0] == before[0] + 2 and during[2] == before[2] + 2, (before, during)   # staging buffer, device copy; two events
    e.close()
    assert native.live_allocations() == before
