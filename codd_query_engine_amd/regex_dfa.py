"""A regular expression as a byte DFA for the document arena: `re.search(pattern, doc) is not None`, decided by one
table walk over the document's UTF-8 bytes and the arena's separator byte.

    compile_search_dfa(pattern, ascii_documents) -> ByteDfa | None     None: outside the device subset, or over the caps
    literal_of(pattern) -> str | None                                  the pattern is that plain text and nothing else
    ByteDfa.matches(doc_bytes) -> bool                                 the CPU restatement of csrc/doc_regex.h

Pure Python: no torch, no engine.  The pattern is read by the standard library's own parser (sre_parse; re._parser from 3.11), so
escapes, classes and repeats are Python's reading of them; its op tree is translated into an NFA over BYTES, and the subset
construction turns "the pattern matches somewhere" into one DFA:

  - a thread of the pattern is restarted at every byte position (the implicit `(?s:.*)` in front of a search); the `^` / `\\A`
    edges can be taken only in the closure at position 0;
  - a completed match is sticky: ACCEPT absorbs;
  - the end of the document is the separator 0x00, consumed as the last symbol, in a byte class of its own.  An end assertion is
    an OBLIGATION a thread carries from the assertion on: after `\\Z` the rest of the input must be empty, after `$` empty or one
    "\\n".  A thread under `$` may still consume one "\\n" (the obligation tightens to `\\Z`'s), under `\\Z` nothing; a thread that
    completed the pattern under an obligation waits for the separator, which sends it to ACCEPT.  So `a$\\n` matches "a\\n", as in re;
  - the empty thread set with nothing to restart (a pattern that begins with `^`) is REJECT, which absorbs too: a lane of the
    kernel stops reading there.  The separator sends every state to ACCEPT or REJECT.

Every fragment that consumes input consumes whole UTF-8 sequences (a lead byte and its continuation bytes), and no fragment
begins with a continuation byte, so a thread restarted inside a code point dies on its first byte: no match begins or ends
inside a code point, and bytes decide what code points would.

The subset: literals (any code point but U+0000), `.`, `[...]` / `[^...]` with ASCII members and ranges, NOT_LITERAL of an ASCII
character, greedy and lazy `* + ? {m,n}` (laziness cannot change yes/no), `|`, groups, `^ $ \\A \\Z` without MULTILINE; and only
when every stored document is ASCII (`ascii_documents`): `\\d \\w \\s \\D \\W \\S` and a global `(?i)` over an all-ASCII pattern — there
the Unicode-aware meanings collapse to fixed ASCII sets.  Everything else is None: back-references, look-around, `\\b`, scoped or
other flags, possessive repeats and atomic groups, classes with non-ASCII members, a literal U+0000.
"""

from __future__ import annotations

import warnings
from dataclasses import dataclass
from typing import Optional

try:  # Python 3.11+
    import re._constants as _c
    import re._parser as _parser
except ImportError:  # Python 3.10 and before
    try:
        import sre_constants as _c
        import sre_parse as _parser
    except ImportError:  # no parser: every pattern is the host's
        _c = _parser = None

MAX_DFA_STATES = 255     # a state is one uint8
MAX_DFA_TABLE = 8192     # CODD_KNN_MAX_DFA_TABLE: bytes of next[nstates][nclasses]
_MAX_NFA_STATES = 4096   # {m,n} expansion gives up here

_NONE, _DOLLAR, _END = 0, 1, 2   # a thread's obligation: nothing; the rest is "" or "\n" (`$`); the rest is "" (`\Z`)
_NL = 0x0A


class _Unsupported(Exception):
    """The pattern is outside the device subset or over the caps."""


@dataclass(frozen=True)
class ByteDfa:
    """next_state = next[state * nclasses + class_of[byte]]; a document matches iff the walk over its bytes and one 0x00 from
    `start` ends in `accept`.  `accept` absorbs; so does `reject` (-1: the pattern has no state that can never match)."""

    class_of: bytes
    next: bytes
    nstates: int
    nclasses: int
    start: int
    accept: int
    reject: int

    def matches(self, doc_bytes: bytes) -> bool:
        state, nxt, cls, ncls = self.start, self.next, self.class_of, self.nclasses
        for b in doc_bytes:
            state = nxt[state * ncls + cls[b]]
            if state == self.accept or state == self.reject:   # (the kernel's lanes stop here too)
                return state == self.accept
        return nxt[state * ncls + cls[0]] == self.accept


def _parse(pattern: str):
    """(op tree, flags) by the standard library's parser; _Unsupported when there is none.  re.error passes through."""
    if _parser is None:
        raise _Unsupported("no parser")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")   # (3.10 warns about global flags that are not at the start and applies them to the whole pattern, as re.compile does there; 3.11 on refuses them)
        tree = _parser.parse(pattern)
    state = getattr(tree, "state", None) or getattr(tree, "pattern", None)
    return tree, state.flags


def literal_of(pattern: str) -> Optional[str]:
    """The text a pattern stands for when nothing but literal characters is left after parsing (`re.search` is then `text in
    doc`); None otherwise."""
    try:
        tree, flags = _parse(pattern)
    except Exception:
        return None
    if flags & ~_c.SRE_FLAG_UNICODE or len(tree) == 0:
        return None
    if any(op is not _c.LITERAL for op, _ in tree):
        return None
    return "".join(chr(av) for _, av in tree)


# ------------------------------------------------------------------------------------------------------------------ ASCII sets
def _category_set(cat) -> tuple:
    """(ASCII members as a set of ints, matches code points outside ASCII) of a class category, for ASCII documents: str.isdigit /
    isalnum / isspace restricted to ASCII, which is what the Unicode-aware \\d \\w \\s are there."""
    digits = set(range(0x30, 0x3A))
    word = digits | set(range(0x41, 0x5B)) | set(range(0x61, 0x7B)) | {0x5F}
    space = {0x09, 0x0A, 0x0B, 0x0C, 0x0D, 0x1C, 0x1D, 0x1E, 0x1F, 0x20}
    everything = set(range(1, 128))
    table = {
        _c.CATEGORY_DIGIT: (digits, False), _c.CATEGORY_NOT_DIGIT: (everything - digits, True),
        _c.CATEGORY_WORD: (word, False), _c.CATEGORY_NOT_WORD: (everything - word, True),
        _c.CATEGORY_SPACE: (space, False), _c.CATEGORY_NOT_SPACE: (everything - space, True),
    }
    if cat not in table:
        raise _Unsupported("category")
    return table[cat]


def _fold(members: set) -> set:
    """(?i) on ASCII: a character matches when its lower or its upper case is a member."""
    return {c for c in range(1, 128) if ord(chr(c).lower()) in members or ord(chr(c).upper()) in members}


# ------------------------------------------------------------------------------------------------------------------ the NFA
class _Nfa:
    """States are ints; per state a list of edges: ("b", byte set as a 256-bit int, to), ("e", to), ("^", to), ("$", to),
    ("Z", to)."""

    def __init__(self):
        self.edges: list[list[tuple]] = []

    def state(self) -> int:
        if len(self.edges) >= _MAX_NFA_STATES:
            raise _Unsupported("too many NFA states")
        self.edges.append([])
        return len(self.edges) - 1

    def eps(self, a: int, b: int, kind: str = "e") -> None:
        self.edges[a].append((kind, b))

    def on(self, a: int, byte_set: int, b: int) -> None:
        if byte_set:
            self.edges[a].append(("b", byte_set, b))


def _bits(lo: int, hi: int) -> int:
    """the byte set [lo, hi]"""
    return ((1 << (hi - lo + 1)) - 1) << lo


_CONT = _bits(0x80, 0xBF)


class _Builder:
    def __init__(self, flags: int, ascii_documents: bool):
        self.nfa = _Nfa()
        self.ascii_documents = ascii_documents
        self.ignorecase = bool(flags & _c.SRE_FLAG_IGNORECASE)

    # one code point: an ASCII byte out of `ascii_members` (never 0x00), or — with `others` — any multi-byte sequence, leniently
    # (lead byte C0-DF + 1, E0-EF + 2, F0-F7 + 3 continuation bytes: the arena's bytes come from Python's encoder)
    def code_point(self, a: int, b: int, ascii_members: set, others: bool) -> None:
        nfa = self.nfa
        mask = 0
        for ch in ascii_members:
            if 0 < ch < 128:
                mask |= 1 << ch
        nfa.on(a, mask, b)
        if others:
            c1, c2, c3 = nfa.state(), nfa.state(), nfa.state()
            nfa.on(a, _bits(0xC0, 0xDF), c1)
            nfa.on(a, _bits(0xE0, 0xEF), c2)
            nfa.on(a, _bits(0xF0, 0xF7), c3)
            nfa.on(c3, _CONT, c2)
            nfa.on(c2, _CONT, c1)
            nfa.on(c1, _CONT, b)

    def literal(self, a: int, b: int, ch: int) -> None:
        if ch == 0:
            raise _Unsupported("U+0000")
        if ch < 128:
            self.code_point(a, b, _fold({ch}) if self.ignorecase else {ch}, False)
            return
        if self.ignorecase:   # (`ſ` matches "s", the Kelvin sign "k": folding outside ASCII stays with re)
            raise _Unsupported("non-ASCII under (?i)")
        raw = chr(ch).encode("utf-8", "surrogatepass")
        at = a
        for i, byte in enumerate(raw):
            to = b if i == len(raw) - 1 else self.nfa.state()
            self.nfa.on(at, 1 << byte, to)
            at = to

    def char_class(self, a: int, b: int, items) -> None:
        negate = False
        members: set = set()
        others = False
        beyond: list = []   # single members outside ASCII (the parser writes `(?:b|é)` as the class [bé]): alternatives of their own
        for op, av in items:
            if op is _c.NEGATE:
                negate = True
            elif op is _c.LITERAL:
                if av == 0:
                    raise _Unsupported("U+0000")
                if av >= 128:
                    beyond.append(av)
                else:
                    members.add(av)
            elif op is _c.RANGE:
                lo, hi = av
                if hi >= 128 or lo == 0:
                    raise _Unsupported("class range outside ASCII")
                members.update(range(lo, hi + 1))
            elif op is _c.CATEGORY:
                if not self.ascii_documents:
                    raise _Unsupported("category on non-ASCII documents")
                more, outside = _category_set(av)
                members |= more
                others = others or outside
            else:
                raise _Unsupported(f"class item {op}")
        if beyond and (negate or self.ignorecase):
            raise _Unsupported("class member outside ASCII")
        for ch in beyond:
            self.literal(a, b, ch)
        if self.ignorecase:
            members = _fold(members)
        if negate:
            members = set(range(1, 128)) - members
            others = not others
        self.code_point(a, b, members, others)

    def repeat(self, a: int, b: int, lo: int, hi, sub) -> None:
        nfa = self.nfa
        at = a
        for _ in range(lo):
            to = nfa.state()
            self.sequence(at, to, sub)
            at = to
        if hi == _c.MAXREPEAT:
            # at -> (sub)* -> b: a loop state of its own, so that the loop cannot be entered from behind
            loop, back = nfa.state(), nfa.state()
            nfa.eps(at, loop)
            self.sequence(loop, back, sub)
            nfa.eps(back, loop)
            nfa.eps(loop, b)
        else:
            if hi < lo:
                raise _Unsupported("repeat bounds")
            for _ in range(hi - lo):
                to = nfa.state()
                nfa.eps(at, b)
                self.sequence(at, to, sub)
                at = to
            nfa.eps(at, b)

    def sequence(self, a: int, b: int, items) -> None:
        """a -> items one after the other -> b"""
        nfa = self.nfa
        items = list(items)
        at = a
        for i, (op, av) in enumerate(items):
            to = b if i == len(items) - 1 else nfa.state()
            if op is _c.LITERAL:
                self.literal(at, to, av)
            elif op is _c.NOT_LITERAL:
                if av >= 128 or av == 0:
                    raise _Unsupported("NOT_LITERAL outside ASCII")
                if self.ignorecase:
                    self.code_point(at, to, set(range(1, 128)) - _fold({av}), True)
                else:
                    self.code_point(at, to, set(range(1, 128)) - {av}, True)
            elif op is _c.ANY:
                self.code_point(at, to, set(range(1, 128)) - {_NL}, True)
            elif op is _c.IN:
                self.char_class(at, to, av)
            elif op is _c.BRANCH:
                for alt in av[1]:
                    self.sequence(at, to, alt)
            elif op is _c.SUBPATTERN:
                _, add_flags, del_flags, sub = av
                if add_flags or del_flags:
                    raise _Unsupported("scoped flags")
                self.sequence(at, to, sub)
            elif op is _c.MAX_REPEAT or op is _c.MIN_REPEAT:
                self.repeat(at, to, av[0], av[1], av[2])
            elif op is _c.AT:
                kind = {_c.AT_BEGINNING: "^", _c.AT_BEGINNING_STRING: "^", _c.AT_END: "$", _c.AT_END_STRING: "Z"}.get(av)
                if kind is None:
                    raise _Unsupported(f"assertion {av}")
                nfa.eps(at, to, kind)
            else:   # GROUPREF, ASSERT, ASSERT_NOT, GROUPREF_EXISTS, POSSESSIVE_REPEAT, ATOMIC_GROUP ...
                raise _Unsupported(f"op {op}")
            at = to
        if not items:
            nfa.eps(a, b)


# ------------------------------------------------------------------------------------------------------------------ the DFA
def _closure(nfa: _Nfa, threads, at_begin: bool) -> set:
    """Everything reachable from `threads` ((state, obligation) pairs) without consuming a byte."""
    seen = set(threads)
    todo = list(seen)
    while todo:
        s, obl = todo.pop()
        for edge in nfa.edges[s]:
            kind = edge[0]
            if kind == "b" or (kind == "^" and not at_begin):
                continue
            new = (edge[1], _END if kind == "Z" else max(obl, _DOLLAR) if kind == "$" else obl)
            if new not in seen:
                seen.add(new)
                todo.append(new)
    return seen


def _build_dfa(nfa: _Nfa, first: int, final: int) -> ByteDfa:
    consumes = [any(edge[0] == "b" for edge in edges) for edges in nfa.edges]

    def closure(threads, at_begin: bool) -> frozenset:
        # ... without the threads that can never move again: no byte edge to take, or `\Z` behind them and bytes still to match.
        # What is left decides the future alone, so states that differ only in such threads are one state, and a set that
        # empties is dead
        return frozenset((s, obl) for s, obl in _closure(nfa, threads, at_begin) if s == final or (consumes[s] and obl != _END))

    # byte classes: bytes no edge tells apart; 0x00 and "\n" each alone (the separator; the one byte a `$` thread may still see)
    sets = sorted({edge[1] for edges in nfa.edges for edge in edges if edge[0] == "b"})
    keys: dict = {}
    class_of = bytearray(256)
    for byte in range(256):
        key = ("nul",) if byte == 0 else ("nl",) + tuple((s >> byte) & 1 for s in sets) if byte == _NL else tuple((s >> byte) & 1 for s in sets)
        class_of[byte] = keys.setdefault(key, len(keys))
    nclasses = len(keys)
    sample = {c: b for b, c in reversed(list(enumerate(class_of)))}   # the lowest byte of each class
    if nclasses > MAX_DFA_TABLE:
        raise _Unsupported("too many byte classes")

    restart = closure([(first, _NONE)], False)
    begin = closure([(first, _NONE)], True)
    ACCEPT, REJECT = "accept", "reject"   # the two absorbing states
    done = lambda threads: (final, _NONE) in threads   # noqa: E731

    def step(threads: frozenset, byte: int):
        if byte == 0:
            return ACCEPT if any(s == final and obl != _NONE for s, obl in threads) else REJECT
        moved = set()
        for s, obl in threads:
            if obl == _END or (obl == _DOLLAR and byte != _NL):
                continue
            after = _NONE if obl == _NONE else _END
            if s == final:
                moved.add((final, after))   # (under `$`, in front of the last "\n": waits for the separator)
                continue
            for edge in nfa.edges[s]:
                if edge[0] == "b" and (edge[1] >> byte) & 1:
                    moved.add((edge[2], after))
        out = closure(moved, False) | restart
        return ACCEPT if done(out) else out if out else REJECT   # (empty: nothing alive and nothing to restart, for good)

    start_key = ACCEPT if done(begin) else begin if begin else REJECT
    ids = {start_key: 0}
    order = [start_key]
    rows: list[list] = []
    at = 0
    while at < len(order):
        key = order[at]
        at += 1
        row = []
        for c in range(nclasses):
            to = key if key in (ACCEPT, REJECT) else step(key, sample[c])
            if to not in ids:
                ids[to] = len(order)
                order.append(to)
                if len(order) > MAX_DFA_STATES or len(order) * nclasses > MAX_DFA_TABLE:
                    raise _Unsupported("over the caps")
            row.append(ids[to])
        rows.append(row)
    if ACCEPT not in ids:   # nothing matches: the table still names an accepting state, one nobody enters
        ids[ACCEPT] = len(order)
        order.append(ACCEPT)
        rows.append([ids[ACCEPT]] * nclasses)
        if len(order) > MAX_DFA_STATES or len(order) * nclasses > MAX_DFA_TABLE:
            raise _Unsupported("over the caps")
    nstates = len(order)
    table = bytes(v for row in rows for v in row)
    return ByteDfa(bytes(class_of), table, nstates, nclasses, 0, ids[ACCEPT], ids.get(REJECT, -1))


def compile_search_dfa(pattern: str, ascii_documents: bool) -> Optional[ByteDfa]:
    """The DFA that decides `re.search(pattern, doc) is not None` over doc's UTF-8 bytes plus one 0x00; None when the pattern is
    outside the device subset, over the caps, or not a pattern at all (the caller's re.compile says why).  `ascii_documents`: every
    document the table will run over is ASCII — the condition for \\d \\w \\s and (?i)."""
    try:
        tree, flags = _parse(pattern)
        allowed = _c.SRE_FLAG_UNICODE | (_c.SRE_FLAG_IGNORECASE if ascii_documents else 0)
        if flags & ~allowed:
            raise _Unsupported("flags")
        builder = _Builder(flags, ascii_documents)
        first, final = builder.nfa.state(), builder.nfa.state()
        builder.sequence(first, final, tree)
        return _build_dfa(builder.nfa, first, final)
    except _Unsupported:
        return None
    except Exception:   # re.error, RecursionError, a parser of another shape: the host's business
        return None
