"""CPU reference of what each stage of a filter pass (sample -> anchor -> filter) hands on, stated over the rows as
stored and the prepared queries, for tests/test_gpu_filter_stages.py (the device side, read back through
DeviceKnnIndex.last_pass) and tests/test_filter_stage_bands.py (the same data without a device).

    approximate scores   int8 programs: the integer accumulators and the fp32 products the kernels form from them, bit for bit
                         (tests/_int8_reference.py); 2-byte programs: the fp64 dot product of the operands rounded to the shadow's
                         element type, which the device's fp32 accumulation meets within ACC(dpad) = dpad 2^-23
    sample               key[q][u] = the largest key(score, row) over the rows below n of sampled tile u (ties: the lower row)
    anchor               L(q) = the smallest canonical exact score among the live rows of the k best sample keys; thr = fp32(L - eps),
                         thr0 = fp32(L - A(q)); -inf with fewer than k live keys, +inf for padding queries
    candidates           per family, the rows a program must emit and the rows it must not (Pass.cut)

The canonical exact scores come from oracle.knn_oracle (canon_dot): one ctypes call per (query, row) pair, so they are only ever
computed for the pairs a statement needs; an fp32 matrix product with a margin of 4 dpad 2^-24 |q||c| (its own error and the
canonical chain's are each below dpad 2^-24 |q||c|) chooses those pairs."""

from __future__ import annotations

import ctypes
from dataclasses import dataclass, field

import numpy as np

from oracle import knn_oracle as o
from tests import _int8_reference as i8
from tests import _space_reference as sr

f32 = np.float32
TILE = 256
K = 10
U24 = 2.0**-24


def ACC(dpad):
    """the documented uncertainty of a 2-byte approximate score: the order of the fp32 accumulation"""
    return dpad * 2.0**-23


# ---- the cases -------------------------------------------------------------------------------------------------------------------
BASE_OPTIONS = {"filter_min_rows": 1, "filter_min_rows_small": 1, "filter_min_batch": 1, "shadow8_cooldown": 0}


@dataclass
class Case:
    id: str
    family: str                 # GEMM, TILE, TILE_F16
    nbq: int
    d: int
    B: int
    ts: int = 0
    res: int = 0
    el: int = 1
    sqd: int = 0
    space: str = "cosine"
    dtype: str = "f32"
    n: int = 5_200 + 37         # 21 tiles, the last one of 117 rows: its last 32-row block holds 21
    options: dict = field(default_factory=dict)
    multi: bool = False         # n = (2 num_cus + 2) 256 + 77: workgroups of two and of three tiles
    data: str = "gauss"
    seed: int = 0

    def rows(self, num_cus=256):
        return (2 * num_cus + 2) * TILE + 77 if self.multi else self.n

    def program(self):
        return {"family": self.family, "nbq": self.nbq, "ts": self.ts, "res": self.res, "el": self.el, "sqd": self.sqd}

    @property
    def per_block(self):
        return self.family == "TILE" and (self.options.get("per_block", 7) & 1) == 1


def _cases():
    out = []

    def add(id, family, nbq, d, B, **kw):
        kw.setdefault("seed", len(out) + 1)
        out.append(Case(id, family, nbq, d, B, **kw))

    two = {"shadow8": 0}
    # GEMM on the 2-byte shadow: 256 elements are four K-steps of 64, no multiple of 6, so 8 query blocks stay here
    for nbq, B in ((1, 20), (2, 50), (4, 100), (8, 200)):
        add(f"gemm16-nbq{nbq}", "GEMM", nbq, 256, B, el=0, options=two, data="subspace")
    # GEMM on int8 operands: staged, resident, two of six slices resident
    add("gemm8-staged-nbq1", "GEMM", 1, 768, 20)
    add("gemm8-staged-nbq2", "GEMM", 2, 768, 50)
    for nbq, B in ((1, 20), (2, 50), (4, 100), (8, 200)):
        add(f"gemm8-res1-nbq{nbq}", "GEMM", nbq, 256, B, res=1, dtype="f16" if nbq == 4 else "f32")
    add("gemm8-res2", "GEMM", 4, 768, 100, res=2, options={"i8v2_half": 0})
    add("gemm8-staged-nbq4", "GEMM", 4, 1024, 100, options={"i8v2": 0})
    add("gemm8-staged-nbq8", "GEMM", 8, 768, 200, options={"i8v2": 0})
    # TILE, staged: every ts at 8 and at 16 query blocks (8 query blocks: rows of up to 8 K-steps would stay resident)
    staged = (("ts0-d640", 0, 640, {}, "f32"), ("ts0-d1024", 0, 1024, {}, "f32"), ("ts1-d1152", 1, 1152, {}, "bf16"),
              ("ts1-d384", 1, 384, {"resident_q": 0}, "f32"), ("ts2-d1536", 2, 1536, {}, "bf16"), ("ts2-d768", 2, 768, {"i8_pair": 1}, "f32"),
              ("ts3-d768", 3, 768, {}, "f32"))
    for name, ts, d, opts, dtype in staged:
        for nbq, B in ((4, 100), (8, 200)):
            o8 = dict(opts)
            if nbq == 4 and d <= 1024:
                o8["resident_q"] = 0
            add(f"tile-staged-{name}-nbq{nbq}", "TILE", nbq, d, B, ts=ts, options=o8, dtype=dtype)
    add("tile-res-ts0-d512", "TILE", 8, 512, 200, ts=0, res=1)
    add("tile-res-ts1-d384", "TILE", 8, 384, 200, ts=1, res=1)
    # ... and what the default options run for 65..128 queries on rows of up to 1,024 elements: the 8-query-block resident form
    # (16 KiB slices packed into half slots, hit lists split by tile parity)
    add("tile-res-ts1-d768-nbq4", "TILE", 4, 768, 100, ts=1, res=1)
    add("tile-res-ts0-d640-nbq4", "TILE", 4, 640, 100, ts=0, res=1)
    # ... and under the device-wide bound, where the cut is the first-generation kernel's plus the integer slack
    add("tile-staged-ts3-d768-nbq8-pb0", "TILE", 8, 768, 200, ts=3, options={"per_block": 0})
    add("tile-staged-ts0-d640-nbq8-pb0", "TILE", 8, 640, 200, ts=0, options={"per_block": 0})
    add("tile-res-ts1-d384-pb0", "TILE", 8, 384, 200, ts=1, res=1, options={"per_block": 0})
    # TILE_F16: 18, 6 and 12 K-steps of 64 elements
    add("tilef16-ts2-d1152", "TILE_F16", 8, 1152, 200, ts=2, el=0, options=two, data="subspace", dtype="f16")
    add("tilef16-ts3-d384", "TILE_F16", 8, 384, 200, ts=3, el=0, options=two, data="subspace")
    add("tilef16-ts4-d768", "TILE_F16", 8, 768, 200, ts=4, el=0, options=two, data="subspace")
    # the squared-distance epilogue of an l2 index, and the ip leg
    sf = {"space_filter": 1}
    for nbq, B in ((1, 20), (2, 50), (4, 100), (8, 200)):
        add(f"sqd-nbq{nbq}", "GEMM", nbq, 256, B, sqd=1, space="l2", options=sf, data="scaled")
    add("ip-staged-nbq2", "GEMM", 2, 768, 50, space="ip", options=sf, data="scaled")
    add("ip-res1-nbq8", "GEMM", 8, 256, 200, res=1, space="ip", options=sf, data="scaled", dtype="bf16")
    add("ip-staged-nbq4", "GEMM", 4, 1024, 100, space="ip", options=sf, data="scaled")
    add("ip-staged-nbq8", "GEMM", 8, 768, 200, space="ip", options=sf, data="scaled")
    add("ip-res2-nbq4", "GEMM", 4, 768, 100, res=2, space="ip", options=sf, data="scaled")
    # several tiles per workgroup
    m = {"multi": True}
    add("multi-tile-ts0", "TILE", 8, 512, 130, ts=0, options={"resident_q": 0}, **m)
    add("multi-tile-ts1", "TILE", 8, 384, 130, ts=1, options={"resident_q": 0}, **m)
    add("multi-tile-ts2", "TILE", 8, 768, 130, ts=2, options={"i8_pair": 1}, **m)
    add("multi-tile-ts3", "TILE", 8, 768, 130, ts=3, **m)
    add("multi-tile-res-ts1", "TILE", 8, 384, 130, ts=1, res=1, **m)
    add("multi-tile-res-ts1-nbq4", "TILE", 4, 384, 100, ts=1, res=1, **m)
    add("multi-tilef16-ts3", "TILE_F16", 8, 384, 130, ts=3, el=0, options=two, data="subspace", **m)
    add("multi-tilef16-ts4", "TILE_F16", 8, 768, 130, ts=4, el=0, options=two, data="subspace", **m)
    add("multi-gemm8-staged", "GEMM", 2, 384, 50, options={"resident_q": 0}, **m)
    add("multi-gemm16-nbq8", "GEMM", 8, 384, 130, el=0, options={"shadow8": 0, "f16_tile": 0}, data="subspace", **m)
    return out


CASES = _cases()
CASE_BY_ID = {c.id: c for c in CASES}
assert len(CASE_BY_ID) == len(CASES)


def make_data(case: Case, num_cus=256):
    """(raw rows [n, d], raw queries [B, d]).  "gauss": Gaussian rows, the data of the kernels' own tests; "subspace": Gaussian in a
    32-dimensional subspace, so that scores spread by 1 / sqrt(32) — the 2-byte cases' ambiguity band (2 dpad 2^-23 wide) then holds
    well under 1 % of a query's candidates, which no choice of seed achieves for full-rank rows of 768 elements (band / candidates
    ~ z 2 ACC sqrt(d) with the threshold z ~ 2.9 deviations out: 1.4 %); "scaled": rows of norms 0.5 .. 2 for the ip and l2 legs.
    Three queries have a real neighbour: in the middle, in the ragged last tile, and row 0."""
    n, d, B = case.rows(num_cus), case.d, case.B
    rng = np.random.default_rng(1000 + case.seed)
    if case.data == "subspace":
        mix = rng.standard_normal((32, d)).astype(np.float32)
        raw = rng.standard_normal((n, 32)).astype(np.float32) @ mix
        q = rng.standard_normal((B, 32)).astype(np.float32) @ mix
    else:
        raw = rng.standard_normal((n, d), dtype=np.float32)
        q = rng.standard_normal((B, d), dtype=np.float32)
        if case.data == "scaled":
            raw *= rng.uniform(0.5, 2.0, (n, 1)).astype(np.float32)
            q *= f32(1.3)
    noise = np.abs(raw).mean() * f32(0.05)
    q[3] = raw[n // 2] + noise * rng.standard_normal(d).astype(np.float32)
    q[5] = raw[n - 1] + noise * rng.standard_normal(d).astype(np.float32)
    q[6] = raw[0]
    return np.ascontiguousarray(raw, dtype=np.float32), np.ascontiguousarray(q, dtype=np.float32)


def stored_rows(space, raw, dtype):
    """the rows as the index stores them (what read_rows returns)"""
    return o.to_storage(o.normalize_rows(raw), dtype) if space == "cosine" else sr.stored(raw, dtype)


def sample_geometry(ntiles, k, use8, nbq, num_cus, sample_div=40, sample_div8=28, sample_rounds8=2, sample_tiles=4096):
    """(sampled tiles, stride) of a pass: sample_tile_count() of the host code, for the tests that run without a device (the device
    tests take both from the read-back)"""
    ts = ntiles // ((2 * sample_div8 if nbq == 1 else sample_div8) if use8 else sample_div)
    if use8:
        rounds = (1 if nbq == 1 else sample_rounds8) * num_cus
        ts = max(ts, min(rounds, ntiles // 4))
    ts = max(ts, 4 * k, 64)
    if ts < num_cus and ntiles >= 2 * num_cus:
        ts = num_cus
    if ts > num_cus:
        ts = (ts + num_cus - 1) // num_cus * num_cus
    ts = max(min(ts, sample_tiles, ntiles), 1)
    return ts, ntiles // ts


# ---- keys ------------------------------------------------------------------------------------------------------------------------
def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def make_keys(score, rows):
    """packed (fp32 score, row) keys; a score that is not a number ranks as -inf, -0 below +0 (the order map of DESIGN.md §2)"""
    return sr.make_keys(np.asarray(score, dtype=np.float32), np.asarray(rows, dtype=np.int64))


key_rows = sr.key_rows
key_scores = sr.key_scores


# ---- the reference of one pass -----------------------------------------------------------------------------------------------------
class Pass:
    """One index (rows as stored), one block of raw queries, one program family."""

    def __init__(self, case: Case, stored, q_raw, shadow="f16", dead=None):
        self.case, self.space, self.dtype = case, case.space, case.dtype
        self.stored = stored
        self.W = o.widen(stored, case.dtype)
        self.n, self.dpad = self.W.shape
        self.Q = o.normalize_rows(q_raw) if self.space == "cosine" else sr.clean(q_raw, self.dpad)
        self.B = self.Q.shape[0]
        self.E = o.lib().oracle_elems_per_chunk(o._DT_BY_NAME[case.dtype])
        self.live = np.ones(self.n, dtype=bool) if dead is None else ~np.asarray(dead, dtype=bool)
        self.int8 = case.el == 1
        self._W64 = None
        self._canon = {}
        if self.int8:
            self.acc, self.cs, self.qs = i8.int8_parts(self.W, self.Q)
            if case.sqd:
                from tests import _space_filter_reference as fr

                self.rn2, self.nq2 = fr.canon_sq(self.W, self.E), fr.canon_sq(self.Q, 4)
                self.test_value, self.score = i8.sqd_from_parts(self.acc, self.cs, self.qs, self.rn2, self.nq2)   # (w, v)
                self.fold = self.test_value          # the sample folds w and shifts the best by |q|^2
            else:
                self.test_value, self.score = i8.scores_from_parts(self.acc, self.cs, self.qs)                    # (p, s~)
                self.fold = self.test_value          # the sample folds p = acc * s_row and scales the best by s_q
        else:
            cb = o.widen(o.to_storage(self.W, shadow), shadow).astype(np.float64)
            qb = o.widen(o.to_storage(self.Q, shadow), shadow).astype(np.float64)
            self.score = qb @ cb.T                   # fp64
            self.fold = self.score

    # -- sample --
    def sample(self, ts, stride):
        """int8: u64 [B, ts], bit for bit.  2-byte: (fp64 maxima [B, ts], first rows [ts], row counts [ts])"""
        first = np.arange(ts, dtype=np.int64) * stride * TILE
        last = np.minimum(first + TILE, self.n)
        if not self.int8:
            return np.stack([self.score[:, a:b].max(axis=1) for a, b in zip(first, last)], axis=1), first, last - first
        out = np.zeros((self.B, ts), dtype=np.uint64)
        for u, (a, b) in enumerate(zip(first, last)):
            # the fold runs on the unscaled value (ties: the lower row); the query's scale, or its norm, is applied to the winner
            rows = a + np.argmax(make_keys(self.fold[:, a:b], np.broadcast_to(np.arange(b - a), (self.B, b - a))), axis=1)
            best = self.fold[np.arange(self.B), rows]
            with np.errstate(invalid="ignore", over="ignore"):
                best = (best - self.nq2) if self.case.sqd else (best * self.qs)
            out[:, u] = make_keys(best.astype(np.float32), rows)
        return out

    # -- canonical exact scores --
    def canon(self, q, rows):
        """fp32 canonical exact scores of query q against `rows` (cached per pair)"""
        fn = o.lib().oracle_canon_dot
        qv = np.ascontiguousarray(self.Q[q])
        out = np.empty(len(rows), dtype=np.float32)
        for i, r in enumerate(rows):
            r = int(r)
            s = self._canon.get((q, r))
            if s is None:
                if self.space == "l2":
                    dvec = np.ascontiguousarray(qv - self.W[r], dtype=np.float32)
                    p = ctypes.c_void_p(dvec.ctypes.data)
                    s = f32(0.0) - f32(fn(p, p, self.dpad, self.E))
                else:
                    s = f32(fn(ctypes.c_void_p(qv.ctypes.data), ctypes.c_void_p(self.W[r].ctypes.data), self.dpad, self.E))
                self._canon[(q, r)] = s
            out[i] = s
        return out

    def exact64(self, q):
        """(approximate scores of query q against every row, the margin that covers their distance from the canonical ones): one fp32
        matrix product for the whole batch — its error and the canonical chain's are each below dpad 2^-24 |q||c|, the margin is twice
        their sum"""
        if self._W64 is None:
            self._W64 = (self.Q @ self.W.T).astype(np.float64)
            self._wn = np.sqrt(np.einsum("ij,ij->i", self.W, self.W, dtype=np.float64))
        qn = np.linalg.norm(self.Q[q].astype(np.float64))
        if self.space == "l2":
            s = -(self._wn**2 - 2.0 * self._W64[q] + qn**2)
            margin = 8.0 * self.dpad * U24 * (self._wn + qn) ** 2 + 1e-30
        else:
            s = self._W64[q]
            margin = 4.0 * self.dpad * U24 * self._wn * qn + 1e-30
        return s, margin

    def topk(self, q, k):
        """(canonical scores fp32 [k] descending, rows [k]) of query q over the live rows, ties to the lower row"""
        s, margin = self.exact64(q)
        s = np.where(self.live, s, -np.inf)
        kth = np.partition(s, -k)[-k]
        near = np.flatnonzero(s >= kth - 2.0 * margin.max())
        c = self.canon(q, near)
        order = np.lexsort((near, -c.astype(np.float64)))[:k]
        return c[order], near[order]

    def rows_reaching(self, q, level):
        """the live rows whose canonical exact score is >= level, ascending"""
        if level == -np.inf:
            return np.flatnonzero(self.live)
        s, margin = self.exact64(q)
        near = np.flatnonzero((s >= level - margin) & self.live)
        return near[self.canon(q, near) >= level]

    def kth_best(self, q, k):
        """the canonical k-th best exact score among the live rows (-inf with fewer than k of them)"""
        if self.live.sum() < k:
            return f32(-np.inf)
        return self.topk(q, k)[0][-1]

    # -- anchor --
    def anchors(self, bucket_keys, k, eps16, qmeta):
        """(L, thr, thr0) fp32 [256] from the DUMPED sample keys [256, ts]: thr0 is meaningful for int8 cosine passes only"""
        L = np.full(256, np.inf, dtype=np.float32)
        for q in range(self.B):
            keys = bucket_keys[q].copy()
            rows = key_rows(keys)
            keys[(rows >= 0) & ~self.live[np.clip(rows, 0, self.n - 1)]] = 0
            best = np.sort(keys)[::-1][:k]
            L[q] = self.canon(q, key_rows(best)).min() if (len(best) == k and best[-1] != 0) else -np.inf
        with np.errstate(invalid="ignore"):
            if self.int8:
                thr = (L - f32(0.5) * qmeta[256:512]).astype(np.float32)
                thr0 = (L - qmeta[512:768]).astype(np.float32)
            else:
                thr = (L - f32(eps16)).astype(np.float32)
                thr0 = thr
        pad = np.arange(256) >= self.B
        thr[pad], thr0[pad] = np.inf, np.inf
        return L, thr, thr0

    # -- the cut --
    def cut(self, q, thr, thr0, qmeta=None, bmeta=None):
        """(must, may_not, exempt): boolean [n] — rows the program must emit for query q, rows it must not, and the ambiguity band
        between them (exempt from both).  See the statements in tests/test_gpu_filter_stages.py."""
        c = self.case
        n = self.n
        t = f32(thr[q])
        if c.family == "GEMM" and self.int8:
            with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
                if c.sqd:      # !(w < thr + |q|^2): a value that is not a number is a hit
                    lim = t if t == -np.inf else f32(t + self.nq2[q])
                    must = ~(self.test_value[q] < lim)
                else:          # acc * s_row >= thr / s_q
                    must = self.test_value[q] >= f32(t / self.qs[q])
            return must, ~must, np.zeros(n, dtype=bool)
        if not self.int8:      # the accumulator is the score: within ACC of the fp64 reference, either side of thr
            delta = ACC(self.dpad)
            m = self.score[q] - float(t)
            if np.isnan(t):
                return np.zeros(n, bool), np.ones(n, bool), np.zeros(n, bool)
            must, may_not = m > delta, m < -delta
            return must, may_not, ~(must | may_not)
        if not c.per_block:
            # the device-wide bound: every row of the first-generation kernel's list, fp32(fp32(acc * scale) * s_q) >= thr; what else
            # the list may hold is bounded in accumulator levels (int_slack_ok)
            must = self.score[q] >= t
            return must, np.zeros(n, bool), np.zeros(n, bool)
        # TILE on int8 operands, in fp64 from the dumped scales: the kernel tests the INTEGER accumulator against
        # (int)(x) - 2, x = fp32 chain of (thr0 / s_q - (B / s_q) e_block) / scale_block
        sb = np.repeat(bmeta[:, 0].astype(np.float64), 32)[:n]
        eb = np.repeat(bmeta[:, 1].astype(np.float64), 32)[:n]
        sq = float(qmeta[q])
        t0 = float(thr0[q])
        Bq = float(qmeta[768 + q])
        if np.isnan(t0) or sq == 0.0:
            # a zero query: the threshold is thr0 / 0 — -inf (every row a hit) below zero, +inf or not a number (none) otherwise
            hit = np.full(n, t0 < 0.0)
            return hit, ~hit, np.zeros(n, bool)
        s_exact = self.acc[q].astype(np.float64) * sb * sq
        m = s_exact + Bq * eb - t0
        delta = 8.0 * U24 * (abs(t0) + Bq * eb)
        must = m > delta
        may_not = m < -delta - 3.0 * sb * sq
        return must, may_not, ~(must | may_not)

    def int_slack_ok(self, q, rows, thr, qmeta, bmeta):
        """per_block = 0: is every row of `rows` within three accumulator levels of the smallest accumulator whose float score
        fp32(fp32(acc * scale) * s_q) reaches thr[q]?  (the documented (int)(th / rsl) - 2, plus the truncation)"""
        t = float(f32(thr[q]))
        ok = np.ones(len(rows), dtype=bool)
        if float(qmeta[q]) == 0.0 or not np.isfinite(t):
            return ok               # a zero query, no threshold: every row a hit or none, the exact statement covers both
        for i, r in enumerate(rows):
            sb, sq = f32(bmeta[r // 32, 0]), f32(qmeta[q])
            a = int(np.floor(t / (float(sb) * float(sq)))) - 2     # below the smallest reaching accumulator; walk up to it
            while f32(f32(f32(a) * sb) * sq) < t:
                a += 1
            ok[i] = self.acc[q, r] >= a - 3
        return ok


# ---- the bound's ingredients, restated (for the tests that run without a device; the device tests read them back) -------------------
def eps16_of(dtype, dpad, shadow="f16"):
    """filter_eps() of the host code"""
    if shadow == "f16":
        u, exact_rows, sub = f32(2.0**-11), dtype == "f16", f32(2.0) * np.sqrt(f32(dpad)) * f32(2.0**-25)
    else:
        u, exact_rows, sub = f32(2.0**-8), dtype == "bf16", f32(0.0)
    rounding = u if exact_rows else f32(2.0) * u + u * u
    return f32((rounding + sub + f32(dpad) * f32(2.0**-23)) * f32(1.001))


def model_meta(p: Pass, raw=None, q_raw=None):
    """(qmeta [1024], bmeta [blocks, 2]) as prep_queries8_kernel / prep_queries8_raw_kernel and shadow8_from_rows_kernel leave them, up
    to the order of their fp32 sums (a relative 1e-6 of the slack: nothing a band population depends on)"""
    from tests import _space_filter_reference as fr

    c8, cs = i8.quantise_like_the_kernels(p.W, False)
    err = np.linalg.norm(p.W.astype(np.float64) - c8.astype(np.float64) * cs[:, None].astype(np.float64), axis=1)
    e_row = (err.astype(np.float32) * f32(1.0001) + f32(1e-7)).astype(np.float32)
    nb = (p.n + 31) // 32
    pad = np.zeros(nb * 32, dtype=np.float32)
    pad[: p.n] = e_row
    bmeta = np.stack([cs[::32][:nb], pad.reshape(nb, 32).max(axis=1)], axis=1).astype(np.float32)
    q8, qs = i8.quantise_like_the_kernels(p.Q, True)
    qerr = np.linalg.norm(p.Q.astype(np.float64) - q8.astype(np.float64) * qs[:, None].astype(np.float64), axis=1).astype(np.float32)
    qmeta = np.zeros(1024, dtype=np.float32)
    qmeta[: p.B] = qs
    if p.space == "cosine":
        eq, er = (qerr * f32(1.0001) + f32(1e-7)).astype(np.float32), bmeta[:, 1].max()
        qmeta[256 : 256 + p.B] = f32(2.0) * (eq * (f32(1.01) + er) + f32(1.001) * er + f32(2e-6))
        qmeta[512 : 512 + p.B] = eq * f32(1.01) + f32(2e-6)
        qmeta[768 : 768 + p.B] = eq + f32(1.001)
    else:
        model = fr.Model(p.space, raw, p.dtype, q_raw)
        qmeta[256 : 256 + p.B] = f32(2.0) * model.slack()
        qmeta[512 : 512 + p.B] = model.n_q
    return qmeta, bmeta


def reference_keys(p: Pass, ts, stride):
    """the sample keys [256, ts] of the reference alone (2-byte: the fp64 maxima rounded to fp32, their first row)"""
    keys = np.zeros((256, ts), dtype=np.uint64)
    if p.int8:
        keys[: p.B] = p.sample(ts, stride)
        return keys
    best, first, count = p.sample(ts, stride)
    for u in range(ts):
        rows = first[u] + np.argmax(p.score[:, first[u] : first[u] + count[u]], axis=1)
        keys[: p.B, u] = make_keys(best[:, u].astype(np.float32), rows)
    return keys


def band_population(p: Pass, thr, thr0, qmeta, bmeta):
    """(candidates, exempt rows, largest number of exempt rows of one query) of the whole batch"""
    cand = exempt = worst = 0
    for q in range(p.B):
        must, _, ex = p.cut(q, thr, thr0, qmeta, bmeta)
        cand += int(must.sum()) + int(ex.sum())
        exempt += int(ex.sum())
        worst = max(worst, int(ex.sum()))
    return cand, exempt, worst


def band_is_valid(cand, exempt, worst):
    """a case is valid only if the exempt rows are at most 1 % of its candidates, and at most 8 per query"""
    return exempt * 100 <= cand and worst <= 8


# ---- the statements about a read-back (DeviceKnnIndex.last_pass), shared by the device tests ------------------------------------------
def check_sample(p, lp):
    ts, stride = lp["sample_tiles"], lp["sample_stride"]
    got = lp["bucket_max"]
    if p.int8:
        want = p.sample(ts, stride)
        bad = np.argwhere(got[: p.B] != want)
        assert bad.size == 0, ("sample keys", len(bad), bad[:4], [(hex(got[q, u]), hex(want[q, u])) for q, u in bad[:4]])
        return
    best, first, count = p.sample(ts, stride)
    acc = ACC(p.dpad)
    score, row = key_scores(got[: p.B]).astype(np.float64), key_rows(got[: p.B])
    assert (np.abs(score - best) <= acc).all(), ("sample scores", np.abs(score - best).max(), acc)
    assert ((row >= first[None, :]) & (row < (first + count)[None, :])).all(), "a sample key names a row of another tile"
    ref_at = np.take_along_axis(p.score, row, axis=1)
    assert (ref_at >= best - 2.0 * acc).all(), "a sample key names a row that is not the tile's best"


def check_thresholds(p, lp):
    L, thr, thr0 = p.anchors(lp["bucket_max"], lp["k"], lp["eps"], lp["qmeta"])
    assert np.array_equal(bits(lp["thr"]), bits(thr)), ("thr", np.flatnonzero(bits(lp["thr"]) != bits(thr))[:8])
    if p.int8 and not p.case.sqd:
        assert np.array_equal(bits(lp["thr0"]), bits(thr0)), ("thr0", np.flatnonzero(bits(lp["thr0"]) != bits(thr0))[:8])
    for q in range(p.B):
        assert L[q] <= p.kth_best(q, lp["k"]), ("anchor above the k-th best exact score", q, L[q])
    return L, thr, thr0


def check_candidates(p, lp, L, thr, thr0, skip=(), banded=True, sound=None):
    """every statement about the lists; `skip`: queries whose list was cut at hit_cap (their raw counter says so); `sound`: the queries
    the soundness statement is taken for (None: all)"""
    case, n = p.case, p.n
    qmeta, bmeta = lp["qmeta"], lp["bmeta"]
    cand = exempt = worst = 0
    for q in range(256):
        keys = lp["keys"][q]
        if q >= p.B:
            assert lp["hit_counts"][q] == 0 and len(keys) == 0, ("a padding query has candidates", q)
            continue
        if q in skip:
            continue
        assert lp["hit_counts"][q] == len(keys) <= lp["hit_cap"], (q, lp["hit_counts"][q])
        rows = key_rows(keys)
        assert (rows >= 0).all() and (rows < n).all(), ("row past the count", q, rows.max(initial=0))
        assert len(np.unique(rows)) == len(rows), ("a row twice in one list", q, len(rows) - len(np.unique(rows)))
        got = key_scores(keys)
        if p.int8:
            want = p.score[q, rows]
            want = np.where(np.isnan(want), np.float32(-np.inf), want)
            assert np.array_equal(bits(got), bits(want)), ("a key's score is not the row's", q)
        else:
            assert (np.abs(got.astype(np.float64) - p.score[q, rows]) <= ACC(p.dpad)).all(), ("a key's score is not the row's", q)
        have = np.zeros(n, dtype=bool)
        have[rows] = True
        reach = p.rows_reaching(q, L[q]) if sound is None or q in sound else np.zeros(0, dtype=np.int64)
        assert have[reach].all(), ("a row whose exact score reaches L is missing", q, reach[~have[reach]][:8])
        must, may_not, band = p.cut(q, thr, thr0, qmeta, bmeta)
        assert have[must].all(), ("a row the cut must keep is missing", q, np.flatnonzero(must & ~have)[:8], int((must & ~have).sum()))
        assert not have[may_not].any(), ("a row the cut must drop is there", q, np.flatnonzero(may_not & have)[:8], int((may_not & have).sum()))
        if case.family == "TILE" and not case.per_block:
            extra = np.flatnonzero(have & ~must)
            ok = p.int_slack_ok(q, extra, thr, qmeta, bmeta)
            assert ok.all(), ("an extra row more than three accumulator levels below the threshold", q, extra[~ok][:8])
        cand += int(must.sum()) + int(band.sum())
        exempt += int(band.sum())
        worst = max(worst, int(band.sum()))
    if banded:
        assert band_is_valid(cand, exempt, worst), ("the ambiguity band holds too many rows for this case to count", cand, exempt, worst)
    return cand
