"""The position-parallel definition the device embedder is written to (tests/_embed_reference.py) gives the bits of
HashingEmbeddingFunction on every text of the GPU tests, and those texts can tell an embedder that ignores the order of the
additions from a right one.  No GPU."""

import numpy as np
import pytest

from tests import _embed_reference as ref


def same_bits(texts, dim, tw):
    return np.array_equal(ref.bits(ref.embed(texts, dim, tw)), ref.bits(ref.host(texts, dim, tw)))


@pytest.mark.parametrize("dim,tw", [(8, 0.35), (100, 0.1), (384, 0.35), (384, 0.0), (768, 1.0), (4096, 0.35)])
def test_the_definition_is_the_host_embedder_bit_for_bit(dim, tw):
    texts = ref.boundary_texts() + ref.step_edge_texts() + ref.order_texts() + ref.coverage_texts()[::4] + ref.coverage_texts()[-1:]
    assert len(texts) > 450
    assert same_bits(texts, dim, tw)


def test_a_token_never_continues_into_the_neighbouring_text():
    """ "ab" and "cd" back to back are two tokens: the definition works per text, as the kernel must from the offsets alone."""
    apart = ref.embed([b"ab", b"cd"], 384, 0.35)
    assert same_bits([b"ab", b"cd"], 384, 0.35)
    assert not np.array_equal(apart.sum(0), ref.embed([b"abcd"], 384, 0.35)[0])


def test_upper_case_nul_and_del():
    assert np.array_equal(ref.embed([b"AbC_9"], 100, 0.35), ref.embed([b"abc_9"], 100, 0.35))
    assert np.array_equal(ref.embed([b"a\x00b\x7fc"], 100, 0.35), ref.embed([b"a b c"], 100, 0.35))
    assert same_bits([b"a\x00b\x7fc", b"\x00", b"\x1fa\x1c"], 100, 0.35)


def test_the_order_of_the_additions_is_in_the_bits():
    """At dim = 8 and weight 0.35 a bucket's sum depends on the order of its 1.0 and 0.35 terms: adding each bucket's word features
    before its trigram features changes the bits of more than half of the random texts, and of the 2,000-byte text."""
    texts = ref.order_texts()
    right, wrong = ref.bits(ref.embed(texts, 8, 0.35)), ref.bits(ref.embed(texts, 8, 0.35, words_first=True))
    differ = (right != wrong).any(axis=1)
    assert differ[0]
    assert differ[1:].sum() > 100, differ[1:].sum()
    assert np.array_equal(right, ref.bits(ref.host(texts, 8, 0.35)))
