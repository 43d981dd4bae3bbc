"""The pattern compiler against `re`: codd_query_engine_amd/regex_dfa.py turns a pattern into a byte DFA, and
ByteDfa.matches — the CPU restatement of doc_regex_kernel — must answer `re.search(pattern, doc) is not None` for every document,
over its UTF-8 bytes.  The lists of tests/_regex_cases.py say what must compile and what must stay with the host; a seeded
generator adds a few thousand patterns of the device subset, none of which may fall to the host.  No GPU, no engine."""

import re

import pytest

from codd_query_engine_amd import regex_dfa
from codd_query_engine_amd.regex_dfa import ByteDfa, compile_search_dfa, literal_of
from tests._regex_cases import DOCUMENTS, MUST_COMPILE, MUST_REFUSE, PatternGenerator


def utf8(doc: str) -> bytes:
    return doc.encode("utf-8", "surrogatepass")


def documents_for(ascii_only: bool):
    return [d for d in DOCUMENTS if d.isascii()] if ascii_only else DOCUMENTS


@pytest.mark.parametrize("pattern,ascii_only", MUST_COMPILE, ids=[p for p, _ in MUST_COMPILE])
def test_the_device_subset_compiles_within_the_caps_and_decides_what_re_decides(pattern, ascii_only):
    for ascii_documents in ([True] if ascii_only else [False, True]):
        dfa = compile_search_dfa(pattern, ascii_documents)
        assert isinstance(dfa, ByteDfa), (pattern, ascii_documents)
        assert 1 <= dfa.nstates <= regex_dfa.MAX_DFA_STATES == 255 and 1 <= dfa.nclasses <= 256
        assert len(dfa.next) == dfa.nstates * dfa.nclasses <= regex_dfa.MAX_DFA_TABLE and regex_dfa.MAX_DFA_TABLE >= 4096
        assert len(dfa.class_of) == 256 and max(dfa.class_of) < dfa.nclasses and max(dfa.next) < dfa.nstates
        assert all(dfa.next[dfa.accept * dfa.nclasses + c] == dfa.accept for c in range(dfa.nclasses)), "ACCEPT absorbs"
        assert list(dfa.class_of).count(dfa.class_of[0]) == 1, "the separator is in a class of its own"
        search = re.compile(pattern).search
        wrong = [d for d in documents_for(ascii_documents) if dfa.matches(utf8(d)) != (search(d) is not None)]
        assert not wrong, (pattern, ascii_documents, wrong)


@pytest.mark.parametrize("pattern,ascii_documents", MUST_REFUSE, ids=[p for p, _ in MUST_REFUSE])
def test_everything_else_is_the_hosts(pattern, ascii_documents):
    re.compile(pattern)   # (a pattern all right: only not the device's)
    assert compile_search_dfa(pattern, ascii_documents) is None


def test_what_needs_ascii_documents_is_refused_without_them():
    for pattern, ascii_only in MUST_COMPILE:
        if ascii_only:
            assert compile_search_dfa(pattern, False) is None, pattern


def test_a_pattern_that_does_not_compile_is_none_not_an_error():
    for pattern in ("(", "a{2,1}", "[z-a]", "(?P<n>a)(?P<n>b)", "*a"):
        with pytest.raises(re.error):
            re.compile(pattern)
        assert compile_search_dfa(pattern, True) is None and literal_of(pattern) is None


def test_a_leading_anchor_gives_the_table_a_dead_state_and_an_open_pattern_none():
    anchored = compile_search_dfa(r"^http_.*_(total|count)$", False)
    assert anchored.reject >= 0 and anchored.reject != anchored.accept
    assert all(anchored.next[anchored.reject * anchored.nclasses + c] == anchored.reject for c in range(anchored.nclasses))
    assert anchored.next[anchored.start * anchored.nclasses + anchored.class_of[ord("x")]] == anchored.reject, "dead at the first byte"
    # an unanchored pattern can still match until the separator: only that byte leads to the rejecting state
    free = compile_search_dfa(r"lat[a-e]ncy", False)
    into_reject = {c for s in range(free.nstates) if s != free.reject for c in range(free.nclasses) if free.next[s * free.nclasses + c] == free.reject}
    assert into_reject == {free.class_of[0]}


def test_plain_text_patterns_are_needles():
    assert literal_of("http_requests") == "http_requests"
    assert literal_of(r"a\.b\n") == "a.b\n" and literal_of("é") == "é"
    assert literal_of("[a]b") == "ab", "what counts is what the parser leaves"
    for pattern in ("a.b", "(?i)abc", "ab|cd", "^ab", "a+", "(ab)", "[ab]b"):
        assert literal_of(pattern) is None, pattern


def test_a_seeded_run_of_generated_patterns_none_of_which_falls_to_the_host():
    """3,000 patterns, each against 40 random documents over the generator's alphabet and a slice of the fixed ones.  (The
    generator's bounds, tighter than "depth 3, repeats up to 3" where the caps need it: tests/_regex_cases.py.)"""
    gen = PatternGenerator(20240611)
    fell, wrong, seen = [], [], set()
    for n in range(3000):
        pattern = gen.pattern()
        seen.add(pattern)
        search = re.compile(pattern).search
        dfa = compile_search_dfa(pattern, False)
        if dfa is None:
            fell.append(pattern)
            continue
        docs = [gen.document() for _ in range(40)] + DOCUMENTS[n % 7::7]
        wrong += [(pattern, d) for d in docs if dfa.matches(utf8(d)) != (search(d) is not None)]
    assert not fell, (len(fell), fell[:10])
    assert not wrong, (len(wrong), wrong[:10])
    assert len(seen) > 2000, "the generator repeats itself"
