"""Patterns and documents shared by the regular-expression tests: the lists the compiler must take and must refuse,
a fixed set of awkward documents, and a seeded generator of patterns inside the device subset.  Plain Python; no engine."""

import random

# (pattern, needs ASCII documents): every one must compile for the device
MUST_COMPILE = [
    (r"^http_.*_(total|count)$", False),
    (r"lat[a-e]ncy", False),
    (r"a.b", False),
    (r"[^a-z]+x", False),
    (r"x*?y", False),
    (r"(ab|cd){2,3}", False),
    (r"é+", False),
    (r"\Aab\Z", False),
    (r"a$", False),
    (r"^$", False),
    (r"\d{2,3}", True),
    (r"(?i)LaTeNcY", True),
    # beyond the issue's list: the end assertions in awkward places, classes, lazy repeats, a 4-byte literal
    (r"a$\n", False),
    (r"$", False),
    (r"\Z", False),
    (r"\n$", False),
    (r"a^b", False),
    (r"(?:^|_)a", False),
    (r"a{2,}?b", False),
    (r"[^\n]é.", False),
    (r"\U0001F600+!", False),
    (r"[a-c_]{3}$", False),
    (r"x[aéK]+|(?:b|é)_", False),
    (r"^(ab|cd)*x$", False),
    (r"(a+|é_)+b", False),
    (r"\s\w+\S", True),
    (r"\W\D", True),
    (r"(?i)[^k]s[Z-a]", True),
    (r"(?i)http_\w*_(TOTAL|count)$", True),
]

# (pattern, ASCII documents): every one must be the host's
MUST_REFUSE = [
    (r"(a)\1", False),
    (r"(?=a)b", False),
    (r"(?<!a)b", False),
    (r"\bfoo", False),
    (r"a\B", False),
    (r"(?m)^a", False),
    (r"(?s)a.b", False),
    (r"(?x) a b", False),
    (r"(?a)\w", True),
    (r"(?i:a)b", True),
    (r"[é-ü]", False),
    (r"[^aé]", False),
    (r"\w+", False),
    (r"\d", False),
    (r"(?i)k", False),
    (r"(?i)ſ", True),
    (r"a\x00b", False),
    (r"(a|b)*a(a|b){8}", False),        # 2^9 subsets: over the state cap
    (r"a{5000}", False),                # over the expansion cap
]

# the fixed documents of the differential check: the empty one, newlines at the end, multi-byte and 4-byte code points, the
# separators \s knows beyond the usual, the two letters whose case folding leaves ASCII, and the patterns' near-misses
DOCUMENTS = [
    "", "\n", "a\n", "a\n\n", "\na", "a", "b", "ab", "ba", "ab\n", "ab\nx", "xab", "abab", "cdab", "abcdab", "cdcdcd", "abc", "a\nb", "a-b", "aéb",
    "a\U0001F600b", "a\x1cb", "\x1c", "K", "k", "K", "ſ", "s", "S", "é", "éé", "xé", "É", "é", "日本語", "\U0001F600", "\U0001F600!",
    "\U0001F600\U0001F600!", "http_requests_total", "http_requests_count", "http_total", "http__total", "xhttp_a_total", "http_a_total\n",
    "http_a_total\n\n", "http_a_totals", "HTTP_A_TOTAL", "http_a1_COUNT", "latency", "latfncy", "latncy", "LATENCY", "LaTeNcY", "Latency!", "12", "1",
    "1234", "a12b", "x", "y", "xy", "xxy", "yx", "--x", "-X", "abx", "aab", "aaab", "b_a", "_a", "a_", "aé!", "\néx", "nés", "acb_", "ab_\n",
    "a b", " a1 ", "\ta_\x1f", "!!", "!9", "ks[", "Ks_", "sa", "xsa", "a\x7fb", "\x7f", "\ud800", "a\ud800b",
]


class PatternGenerator:
    """Seeded patterns inside the device subset over the alphabet a b _ \\n é: literals, `.`, classes and negated classes with ASCII
    members, `|`, groups, greedy and lazy repeats with bounds up to 3, and the four anchors.  The bounds are tighter than "nesting depth 3,
    repeat bounds 3" so that every pattern stays under the DFA caps (255 states, 8,192 table bytes) and `re` itself never
    backtracks for seconds: groups nest two deep, a group holds at most two alternatives of at most two items, a pattern at most
    three items, and a counted repeat {m,n} is applied to single characters and classes only, not to groups (a counted repeat of
    a counted repeat multiplies the copies); a group that holds a repeat is itself repeated at most once."""

    ALPHABET = ["a", "b", "_", "\\n", "é"]
    CLASSES = ["[ab]", "[^a]", "[a-b_]", "[^_\\n]", "[^ab]", "[b_]"]

    def __init__(self, seed: int):
        self.rng = random.Random(seed)

    def char(self) -> str:
        r = self.rng.random()
        if r < 0.6:
            return self.rng.choice(self.ALPHABET)
        if r < 0.75:
            return "."
        return self.rng.choice(self.CLASSES)

    def counted(self) -> str:
        lo = self.rng.randint(0, 3)
        hi = self.rng.randint(max(lo, 1), 3)
        form = self.rng.choice(["{%d,%d}" % (lo, hi), "{%d}" % max(lo, 1), "{%d,}" % lo, "{,%d}" % hi])
        return form + self.rng.choice(["", "", "?"])

    def atom(self, depth: int) -> str:
        r = self.rng.random()
        if depth >= 2 or r < 0.75:
            c = self.char()
            r = self.rng.random()
            if r < 0.55:
                return c
            if r < 0.8:
                return c + self.rng.choice(["*", "+", "?", "*?", "+?", "??"])
            return c + self.counted()
        alts = [self.sequence(depth + 1, 2) for _ in range(self.rng.randint(1, 2))]
        group = self.rng.choice(["(", "(?:"]) + "|".join(alts) + ")"
        if any(c in group for c in "*+{"):   # (an unbounded repeat of a group that repeats inside: `re` may backtrack for minutes)
            return group + self.rng.choice(["", "", "?", "??"])
        return group + self.rng.choice(["", "", "*", "+", "?", "*?"])

    def sequence(self, depth: int, most: int) -> str:
        out = []
        for _ in range(self.rng.randint(1, most)):
            r = self.rng.random()
            if r < 0.06:
                out.append(self.rng.choice(["^", "\\A"]))
            elif r < 0.14:
                out.append(self.rng.choice(["$", "\\Z"]))
            else:
                out.append(self.atom(depth))
        return "".join(out)

    def pattern(self) -> str:
        body = self.sequence(0, 3)
        r = self.rng.random()
        if r < 0.2:
            body = "^" + body
        if 0.1 < r < 0.35:
            body = body + "$"
        return body

    def document(self) -> str:
        return "".join(self.rng.choice(["a", "b", "_", "\n", "é", "a", "b"]) for _ in range(self.rng.randint(0, 10)))
