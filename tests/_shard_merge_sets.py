"""Input sets for the sharded search's sample, union bound, merge and merge verdict (tests/test_shard_merge_ref.py on the restatement
alone, tests/test_shard_merge_direct.py on the GPU).  Everything here is numpy on the host, deterministic and built once.

  merge_case      per-shard top-k lists [P, n, k] whose rows cycle through the contents a merge meets: exact fp32 ties across parts with few
                  distinct scores, fewer than k valid ids over all parts, all padding, +0.0 against -0.0, -FLT_MAX as a real score next to
                  padding, negative scores, ids beyond 2^32, a part that is all padding;
  verdict_sets    the table of the merge verdict: part statuses {0,1,2,3}^3 x the position of a part's bound against the restated k-th score
                  x whether k rows came back x what the other parts' bounds say, at large, ordinary, negative, tiny and zero k-th scores;
                  `rounds_up` holds the rows whose true score rounds UP to fp32 across the bound;
  union_case      shared samples [P, n, 16]: random, heavy ties, unions of exactly 15 / 16 / 17 entries, all INT_MIN, the extreme values,
                  a part that is all padding;
  sample_shards   flat shards for dph_search_sample_dev (sizes that are no multiple of 32) with the query rows that press on the ladder;
  protocol_sets   one dump of 60 011 rows cut into 2, 3 and 5 uneven range shards."""
import functools
import itertools

import numpy as np

from tests import _shard_merge_ref as M

FLT_MAX = M.FLT_MAX
INT_MIN, INT_MAX = M.INT_MIN, M.INT_MAX


# ---------------------------------------------------------------------------------------------------------------- merge
MERGE_SHAPES = [(1, 1, 1), (2, 5, 10), (3, 257, 100), (8, 3, 1024), (8, 64, 16)]
MERGE_KINDS = ("ties", "fewer_than_k", "all_padding", "signed_zeros", "flt_max_real", "negative", "big_ids", "empty_part")


def merge_case(P, n, k, seed=0):
    """-> dict D, I, best, pred, status, bound ([P, n, k] / [P, n]) and kinds [n].  Every part's list is sorted (score desc, id asc) with
    its padding (-1 / -FLT_MAX) at the end, like a search result; ids are unique within a row (over all parts)."""
    rng = np.random.default_rng(1000 * P + 10 * k + n + seed)
    D = np.full((P, n, k), -FLT_MAX, np.float32)
    I = np.full((P, n, k), -1, np.int64)
    kinds = []
    for r in range(n):
        kind = MERGE_KINDS[r % len(MERGE_KINDS)]
        kinds.append(kind)
        if kind == "all_padding":
            continue
        ids = rng.permutation(4 * P * k + 8)[:P * k].astype(np.int64).reshape(P, k)
        if kind == "big_ids" or r % 3 == 0:
            ids = ids + (np.int64(1) << 32) * rng.integers(1, 1 << 20, (P, 1))     # (distinct per part with near certainty; checked below)
        for p in range(P):
            if kind == "fewer_than_k":
                m = int(rng.integers(0, max(1, k // P)))                            # sum over parts < k
            elif kind == "empty_part" and p == P - 1:
                m = 0
            else:
                m = int(rng.integers(0, k + 1)) if r % 2 else k
            if kind == "ties":
                s = rng.integers(0, 4, m).astype(np.float32)
            elif kind == "signed_zeros":
                s = rng.choice(np.array([0.0, -0.0, 1.0, -1.0], np.float32), m)
            elif kind == "flt_max_real":
                s = rng.choice(np.array([-FLT_MAX, -FLT_MAX, -1.0e38, 3.0], np.float32), m)
            elif kind == "negative":
                s = (-np.abs(rng.normal(0, 50, m)) - 1e-3).astype(np.float32)
            else:
                s = np.round(rng.normal(0, 2, m), 1).astype(np.float32)             # one decimal: some exact ties across parts
            order = np.lexsort((ids[p, :m], -s.astype(np.float64)))
            D[p, r, :m] = s[order]
            I[p, r, :m] = ids[p, :m][order]
        v = I[:, r][I[:, r] >= 0]
        assert np.unique(v).size == v.size
    best = rng.normal(0, 1, (P, n, k))
    pred = rng.integers(0, 1000, (P, n, k)).astype(np.int32)
    status = rng.choice(np.array([0, 0, 0, 1, 2, 3], np.int32), (P, n))
    bound = np.where(rng.random((P, n)) < 0.5, -1.0e300, rng.normal(0, 2, (P, n)))
    return {"D": D, "I": I, "best": best, "pred": pred, "status": status, "bound": bound, "kinds": kinds}


# ---------------------------------------------------------------------------------------------------------------- merge verdict
VERDICT_P, VERDICT_K = 3, 4
POSITIONS = ("none", "far_below", "just_below", "just_above", "between", "above_both")
KTH_SCORES = {"kth_large": 35000.123, "kth_one": 1.2345678, "kth_negative": -2.5678, "kth_tiny": 1.0e-30, "kth_tiny_negative": -1.0e-30}
NEAR = 2.0 ** -40           # the closest a bound comes to the restated k-th score (relative); see tests/test_shard_merge_direct.py


class VerdictSet:
    """D / I / S64 [P, n, k], status / bound [P, n]; S64 = the true float64 scores behind D = fp32(S64); row_info[r] = what the row presses on"""

    def __init__(self, name, rows):
        self.name, self.k = name, VERDICT_K
        n = len(rows)
        self.D = np.full((VERDICT_P, n, VERDICT_K), -FLT_MAX, np.float32)
        self.I = np.full((VERDICT_P, n, VERDICT_K), -1, np.int64)
        self.S64 = np.full((VERDICT_P, n, VERDICT_K), -np.inf)
        self.status = np.zeros((VERDICT_P, n), np.int32)
        self.bound = np.zeros((VERDICT_P, n), np.float64)
        self.row_info = []
        for r, (scores, status, bound, info) in enumerate(rows):
            for p in range(VERDICT_P):
                s = np.asarray(scores[p], np.float64)
                self.S64[p, r, :s.size] = s
                self.D[p, r, :s.size] = s.astype(np.float32)
                self.I[p, r, :s.size] = 1000 * r + 10 * p + np.arange(s.size)
            self.status[:, r] = status
            self.bound[:, r] = bound
            self.row_info.append(info)
        self.merged = M.merge(self.D, self.I, VERDICT_K)
        self.kth = M.kth_of(self.merged["D"][:, VERDICT_K - 1], self.merged["nvalid"], VERDICT_K)

    def verdict(self, bounds=True, mutate=None):
        return M.merged_status(self.merged["D"][:, self.k - 1], self.merged["nvalid"], self.k, self.status, self.bound if bounds else None,
                               mutate=mutate)


def _below(d):
    """a float64 score that rounds to the fp32 number d: a quarter of an fp32 ulp below it"""
    d = float(np.float32(d))
    return d - 0.25 * float(np.spacing(np.float32(abs(d)))) if d != 0.0 else d


def _part_scores(dk, short):
    """part 0 holds the k best (the k-th of them is dk), part 1 one row below them, part 2 nothing; `short`: two rows fewer, so that fewer
    than k come back over all parts"""
    a = abs(dk) if dk != 0.0 else 1.0
    p0 = [np.float32(dk + a * f) for f in (0.75, 0.5, 0.25)] + [np.float32(dk)]
    p1 = [np.float32(dk - a * 0.5)]
    if short:
        p0 = p0[:VERDICT_K - 2]
    return [[_below(v) for v in p0], [_below(v) for v in p1], []]


def _bound_at(pos, dk, kth):
    a = abs(kth)
    if pos == "none":
        return -1.0e300
    if pos == "far_below":
        return kth - 0.5 * (a + 1.0)
    if pos == "just_below":
        return kth - a * NEAR
    if pos == "just_above":
        return kth + a * NEAR
    if pos == "between":
        return 0.5 * (kth + dk)
    return dk + 0.5 * abs(dk) + 1.0e-3 * (dk == 0.0)


@functools.lru_cache(maxsize=None)
def verdict_sets():
    sets = []
    combos = list(itertools.product((0, 1, 2, 3), repeat=VERDICT_P))
    for name, score in KTH_SCORES.items():
        dk = float(np.float32(score))
        kth = float(M.kth_of(np.array([dk], np.float32), [VERDICT_K], VERDICT_K)[0])
        assert kth < dk
        rows, i = [], 0
        for short in (False, True):
            for pos in POSITIONS:
                for others in ("none", "above_both"):
                    for st in combos:
                        focus = i % VERDICT_P
                        i += 1
                        bound = [_bound_at(others, dk, kth)] * VERDICT_P
                        bound[focus] = _bound_at(pos, dk, kth)
                        rows.append((_part_scores(dk, short), st, bound, {"short": short, "pos": pos, "others": others, "focus": focus}))
        sets.append(VerdictSet(name, rows))
    # a k-th score of exactly +-0: kth = 0 whatever the arithmetic, so a bound of exactly 0 is an exact case of `>` against `>=`
    rows, i = [], 0
    for dk in (0.0, -0.0):
        for short in (False, True):
            for b in (-1.0e300, -1.0, 0.0, 1.0e-300, 1.0):
                for st in combos:
                    focus = i % VERDICT_P
                    i += 1
                    bound = [-1.0e300] * VERDICT_P
                    bound[focus] = b
                    rows.append((_part_scores(dk, short), st, bound, {"short": short, "pos": b, "others": "none", "focus": focus}))
    sets.append(VerdictSet("kth_zero", rows))
    # the true k-th score rounds UP to fp32 across the bound: S_k < bound_p < fp32(S_k).  A hidden row scoring bound_p belongs in the exact
    # top-k, so the verdict must refuse; without the margin it accepts.
    rows = []
    for i, d in enumerate((35000.123, 1.2345678, 777.77, -2.5678, -0.0123, 1.0e-30)):
        dk = float(np.float32(d))
        ulp = float(np.spacing(np.float32(abs(dk))))
        sc = _part_scores(dk, False)
        sc[0][VERDICT_K - 1] = dk - 0.4 * ulp
        for focus in range(VERDICT_P):
            for st in ((2, 2, 2), (0, 0, 0), (2, 0, 0), (0, 2, 0), (0, 0, 2)):
                bound = [-1.0e300] * VERDICT_P
                bound[focus] = dk - 0.2 * ulp
                rows.append((sc, st, bound, {"short": False, "pos": "rounds_up", "others": "none", "focus": focus}))
    sets.append(VerdictSet("rounds_up", rows))
    return {s.name: s for s in sets}


# ---------------------------------------------------------------------------------------------------------------- union bound
UNION_PARTS, UNION_ROWS = (1, 2, 3, 8, 64), (1, 130, 1000)
UNION_KINDS = ("random", "ties", "exactly_15", "exactly_16", "exactly_17", "all_int_min", "extremes", "empty_part")


def union_case(P, n):
    """-> (top_parts [P, n, 16] int32, kinds [n]); valid entries sit in random slots (the kernel takes INT_MIN as padding anywhere)"""
    rng = np.random.default_rng(77 * P + n)
    top = np.full((P, n, 16), INT_MIN, np.int64)
    kinds = []
    off = UNION_PARTS.index(P) + UNION_ROWS.index(n)
    for r in range(n):
        kind = UNION_KINDS[(r + off) % len(UNION_KINDS)]
        kinds.append(kind)
        flat = top[:, r, :].reshape(-1).copy()
        m = flat.size
        if kind == "random":
            flat[:] = rng.integers(INT_MIN + 1, INT_MAX, m, endpoint=True)
            flat[rng.random(m) < 0.2] = INT_MIN
        elif kind == "ties":
            flat[:] = rng.choice(np.array([-5, 7, 7, 8, INT_MIN]), m)
        elif kind.startswith("exactly_"):
            cnt = min(int(kind[-2:]), m)
            flat[rng.permutation(m)[:cnt]] = rng.integers(-1000, 1000, cnt)
        elif kind == "extremes":
            flat[:] = rng.choice(np.array([INT_MIN, INT_MIN + 1, INT_MIN + 1, INT_MAX, INT_MAX - 1]), m)
        elif kind == "empty_part":
            flat[:] = rng.integers(-10 ** 9, 10 ** 9, m)
            flat[(P - 1) * 16:] = INT_MIN
        top[:, r, :] = flat.reshape(P, 16)
    return top.astype(np.int32), kinds


# ---------------------------------------------------------------------------------------------------------------- sample
MAIN_ROWS = 448 * 32 + 11       # 449 tiles, the last one partial; tile 448 is visited by every explicit ladder below (448 = 2^6 x 7)
PLANT_TILES = (0, 224, 448)     # ... and so are these
N_HIGHER, N_TIED = 10, 40
Q_TIES, Q_NEGATIVE, Q_POSITIVE = 0, 1, 2


class SampleShard:
    def __init__(self, name, xb, x, notes=None):
        self.name, self.x, self.notes = name, np.ascontiguousarray(x, np.float32), notes or {}
        self.shard = M.RangeShard(xb, 0)
        self._keys = None
        self._top = {}

    @property
    def xb(self):
        return self.shard.xb

    def keys(self):
        if self._keys is None:
            self._keys = self.shard.keys(self.x)
        return self._keys

    def top(self, strides, kp):
        """restated sample of EVERY query row under one plan (rows are independent: a pass takes its slice)"""
        sig = (tuple(strides), kp)
        if sig not in self._top:
            key, Hp, lmax = self.keys()
            self._top[sig] = M.sample_top(key, Hp, lmax, self.shard.outliers, strides, kp)
        return self._top[sig]

    def sample(self, n_q, grid, explicit=()):
        """-> (top [n_q, 16], [(q0, rows, strides, kp, info)])"""
        out = np.full((n_q, 16), INT_MIN, np.int64)
        log = []
        for q0, nq, qb in M.passes(n_q):
            strides, kp = M.sample_plan(self.xb.shape[0], grid, qb, explicit)
            t, info = self.top(strides, kp)
            out[q0:q0 + nq] = t[q0:q0 + nq]
            log.append((q0, nq, strides, kp, [{"stride": i["stride"], "bucket": i["bucket"][q0:q0 + nq], "tau": i["tau"][q0:q0 + nq]} for i in info]))
        return out, log


def _aligned_rows(x, n_higher, n_lower=0, step=8, amp=10):
    """rows 40 + amp sign(x): `tie`, n_higher rows above it (one more code step along sign(x) on the 8 i dimensions of largest |x|) and n_lower below"""
    sign = np.where(x >= 0, 1, -1).astype(np.int64)
    order = np.argsort(-np.abs(x), kind="stable")
    tie = 40 + amp * sign
    def bumped(i, d):
        r = tie.copy()
        r[order[:step * i]] += d * sign[order[:step * i]]
        return r
    return tie, [bumped(i, 1) for i in range(1, n_higher + 1)], [bumped(i, -1) for i in range(1, n_lower + 1)]


@functools.lru_cache(maxsize=None)
def sample_shards():
    from densephrases_amd.synth import synthetic_rows
    from tests import _certificate_sets as CS
    rng = np.random.default_rng(4242)
    out = {}
    # ---- main: i.i.d. rows, a block of exact ties at the 16-th place of query row 0, query rows whose real rows all score negative / positive.
    # Query row 0 is the input that found a kernel bug: dph_threshold_kernel let the forty ties race the ten better scores for the 16 slots
    # of `top` and shared e.g. 13 ties and only 3 of the better ones (a looser union bound, never a wrong one).  Every explicit ladder of
    # SAMPLE_CASES on "main" covers it.
    xb = synthetic_rows(0, MAIN_ROWS, seed=21, kind=0).copy()
    x = rng.normal(0, 0.5, (300, 768)).astype(np.float32)
    x[Q_NEGATIVE] = -0.5
    x[Q_POSITIVE] = 0.5
    tie, higher, _ = _aligned_rows(x[Q_TIES], N_HIGHER)
    slots = np.concatenate([np.arange(2, 32), 224 * 32 + np.arange(15), 448 * 32 + np.arange(5)])
    hi_slots = np.array([3, 9, 17, 30, 224 * 32 + 1, 224 * 32 + 8, 224 * 32 + 14, 448 * 32, 448 * 32 + 2, 448 * 32 + 4])
    tie_slots = np.setdiff1d(slots, hi_slots)
    assert tie_slots.size == N_TIED and slots.max() < MAIN_ROWS
    xb[tie_slots] = tie
    xb[hi_slots] = np.stack(higher)
    out["main"] = SampleShard("main", xb, x, {"tie_slots": tie_slots, "hi_slots": hi_slots})
    # ---- large: the upper end of the size range, random query rows
    out["large"] = SampleShard("large", synthetic_rows(0, 39979, seed=22, kind=0), rng.normal(0, 0.5, (130, 768)).astype(np.float32))
    # ---- outlier: the shard of tests/_certificate_sets.py with saturated rows; query rows 0..3 are aligned with four of them
    o = CS.build()[0]["outlier"]
    x = rng.normal(0, 0.5, (130, 768)).astype(np.float32)
    sat = np.arange(12000, 12004)
    x[:4] = np.where(o.xb[sat] > 0, 0.5, -0.5).astype(np.float32)
    out["outlier"] = SampleShard("outlier", o.xb, x, {"sat": sat})
    # ---- small: a shard the select step sorts whole has no ladder level; few: an explicit stride on a shard of 13 rows
    out["small"] = SampleShard("small", synthetic_rows(0, 5000, seed=23, kind=0), rng.normal(0, 0.5, (7, 768)).astype(np.float32))
    out["few"] = SampleShard("few", synthetic_rows(0, 13, seed=24, kind=0), rng.normal(0, 0.5, (7, 768)).astype(np.float32))
    return out


# (shard, explicit ladder -- () = the derived default --, query rows)
SAMPLE_CASES = [
    ("main", (8,), 1), ("main", (8,), 130), ("main", (16, 2), 7), ("main", (16, 2), 300), ("main", (32, 4), 128), ("main", (7, 2), 256),
    ("main", (), 1), ("main", (), 300), ("large", (), 130), ("large", (16, 2), 128), ("outlier", (16, 2), 7), ("outlier", (), 130),
    ("small", (), 7), ("few", (2,), 7),
]


# ---------------------------------------------------------------------------------------------------------------- the whole protocol
DUMP_ROWS = 60011
CUTS = {2: (0, 30011, DUMP_ROWS), 3: (0, 7000, 30011, DUMP_ROWS), 5: (0, 7000, 19003, 30011, 41000, DUMP_ROWS)}
HOME_ROWS = (7000, 30011)       # first rows of the two clusters: local tile 0 of a shard in the 3- and 5-shard cuts (30011: in every cut)
N_HOME = 24
SAT_ROWS = np.arange(35000, 35050)
Q_HOME, Q_TIE, Q_NONFINITE = (0, 1), (2, 3), 12
TIE_K = 10                      # the cross-shard ties sit at ranks k-1 and k of the k = 10 sets
# (name, shards, k)
PROTOCOL_SETS = [("p2_k12", 2, 12), ("p3_k10", 3, 10), ("p5_k10", 5, 10), ("p3_k32", 3, 32)]


class Dump:
    def __init__(self, xb, x):
        self.xb, self.x = xb, x
        self._shards, self._runs = {}, {}

    def shards(self, P):
        if P not in self._shards:
            c = CUTS[P]
            self._shards[P] = [M.RangeShard(self.xb[c[p]:c[p + 1]], c[p]) for p in range(P)]
        return self._shards[P]

    def run(self, P, k, grid=256):
        if (P, k, grid) not in self._runs:
            self._runs[(P, k, grid)] = M.protocol(self.shards(P), self.x, k, grid)
        return self._runs[(P, k, grid)]


@functools.lru_cache(maxsize=None)
def dump():
    """Query rows 0, 1: every good row lives in ONE shard, in its local tile 0 (sampled by every ladder), 24 of them -- the other shards hold
    nothing above the union bound, and with k = 32 fewer than k rows of the whole dump do.  Query rows 2, 3: the (k-1)-th and k-th best
    (k = 10) are byte-identical rows of two different shards, one of them in the shard that is too small for a ladder.  Rows 4..11: random.
    Row 12: a NaN element.  50 saturated rows (outliers of whichever shard holds them) with -128 in the first 384 dimensions, where the
    crafted query rows are positive: they rank last for those and compete for the random ones."""
    from densephrases_amd.synth import synthetic_rows
    rng = np.random.default_rng(606)
    xb = synthetic_rows(0, DUMP_ROWS, seed=31, kind=0).copy()
    x = rng.normal(0, 0.5, (13, 768)).astype(np.float32)
    for q in Q_HOME + Q_TIE:
        x[q, :384] = np.abs(x[q, :384])
    sat = np.where(rng.random((SAT_ROWS.size, 768)) < 0.5, 127, -128)
    sat[:, :384] = -128
    xb[SAT_ROWS] = sat
    for q, row0 in zip(Q_HOME, HOME_ROWS):
        tie, higher, lower = _aligned_rows(x[q], N_HOME // 2, N_HOME // 2 - 1, step=6)
        xb[row0:row0 + N_HOME] = np.stack(higher + [tie] + lower)
    spread = (100, 8000, 20000, 31000, 42000, 50000, 55000, 59000)
    for j, q in enumerate(Q_TIE):
        tie, higher, lower = _aligned_rows(x[q], TIE_K - 2, 5, step=6)
        for r, row in zip(spread, higher):
            xb[r + 40 * j] = row
        xb[3000 + j] = tie                                   # ranks k-1 and k: one copy in the small shard, one far away
        xb[45000 + j] = tie
        for i, row in enumerate(lower):
            xb[12000 + 40 * j + i] = row
    x[Q_NONFINITE, 5] = np.nan
    return Dump(xb, x)
