"""The input sets of the direct ADC scan tests (tests/test_adc_direct.py on the GPU, tests/test_adc_ref.py without one): OPQ + IVFPQ
indexes of random code bytes in which chosen codes are PLANTED at the positions where the scan cuts its work -- segment, chunk, unit,
list and stride boundaries -- so that a query row's best codes sit exactly there.  numpy and the oracle only.  Every set is a pure
function of its name (fixed seeds) and is built once per process.

Planting rule.  For a query row with inner-product tables T [M][256] the code c*[m] = argmax_j T[m][j] has the largest ADC sum any
code can have: with codewords ~ N(0, 0.1) and queries ~ N(0, 0.5) about 36 at M = 96, against a maximum of about 6 over 200 k random
codes (standard deviation 1.4); another row's c* scores like a random code.  The centroids are drawn with standard deviation 0.05 so
that the <x', centroid> term of a list (about +-1) stays far below that gap.  Three kinds of planted row:
  chain   c*, then c* with component j - 1 replaced by that table's second entry, at the row's positions j = 0, 1, ..: the row's
          top-n in that order (a single winner is a chain of one)
  ladder  E <= 1024 codes, c* with component e % M replaced by the table's rank-(1 + e // M) entry: the row's top-E as a set
  block   byte-identical copies of c* inside one list: a tie block, answered in id order
Every set asserts, through the restatement of tests/_adc_ref.py, that its planted codes are where they are meant to be in the ranking
with a margin of at least 10 standard deviations of the row's unplanted scores: a set that does not test what it claims fails here."""
import functools
from types import SimpleNamespace

import numpy as np

from oracle import ivfpq_oracle as P
from tests import _adc_ref as R
from tests._pq_build import _index_from_list_numbers

DIM = 768
CHAIN_GAP = 100 * R.ATOL          # successive members of a chain differ by far more than the comparison's tolerance


def _build(name, seed, M, sizes, planted, extra=0, zero_row=False, nprobe=None, ref_rows=None, n_q=None, row_of=None):
    """planted: [(kind, [(list, offset), ..])] one entry per planted query row; extra: ordinary random rows after them; zero_row: an
    all-zero row last.  n_q / row_of: the batch is n_q random rows and planted row e is row row_of[e] of it.  ref_rows: the rows the
    restatement is computed for (default: all)."""
    rng = np.random.default_rng(seed)
    sizes = np.asarray(sizes, dtype=np.int64)
    nlist, n = len(sizes), int(sizes.sum())
    cent = rng.normal(0, 0.05, (nlist, DIM)).astype(np.float32)
    ix, _ = _index_from_list_numbers(rng, nlist, M, np.repeat(np.arange(nlist), sizes), cent, ids=rng.permutation(n).astype(np.int64))
    n_rows = len(planted) + extra + int(zero_row) if n_q is None else n_q
    row_of = list(range(len(planted))) if row_of is None else list(row_of)
    q = rng.normal(0, 0.5, (n_rows, DIM)).astype(np.float32)
    if zero_row:
        q[-1] = 0.0
    tables = P.lut(P.apply_chain(ix.chain, q[row_of]), ix.index.pq_centroids) if planted else None
    taken, rows = set(), []
    for e, (kind, where) in enumerate(planted):
        rank = np.argsort(-tables[e].astype(np.float64), axis=1, kind="stable")        # [M][256] entries of every table, best first
        ids = []
        for j, (l, o) in enumerate(where):
            assert 0 <= o < sizes[l] and (l, o) not in taken, (name, kind, l, o)
            taken.add((l, o))
            code = rank[:, 0].astype(np.uint8)
            if kind == "chain" and j > 0:
                code[j - 1] = rank[j - 1, 1]
            if kind == "ladder":
                code[j % M] = rank[j % M, 1 + j // M]
            ix.index.list_codes[l][o] = code
            ids.append(int(ix.index.list_ids[l][o]))
        rows.append(SimpleNamespace(kind=kind, where=list(where), ids=np.asarray(ids, np.int64), row=row_of[e]))
    nprobe = nlist if nprobe is None else nprobe
    ref_rows = list(range(n_rows)) if ref_rows is None else sorted(set(ref_rows) | set(row_of))
    ref = dict(zip(ref_rows, R.adc_rows(ix, q[ref_rows], nprobe)))
    s = SimpleNamespace(name=name, ix=ix, q=q, M=M, seg=R.seg_of(M), sizes=sizes, nprobe=nprobe, planted=rows, ref=ref,
                        by_rows=R.by_rows(ix), zero_row=n_rows - 1 if zero_row else None)
    _assert_planted(s)
    return s


def _assert_planted(s):
    all_ids = np.concatenate([p.ids for p in s.planted]) if s.planted else np.zeros(0, np.int64)
    for p in s.planted:
        row = s.ref[p.row]
        n = len(p.ids)
        D, I = row.topk(n + 1)
        spread = float(row.scores[~np.isin(row.ids, all_ids)].astype(np.float64).std())
        assert len(D) == n + 1 and float(D[n - 1]) - float(D[n]) >= 10.0 * spread, (s.name, p.kind, p.row, D[n - 1], D[n], spread)
        if p.kind == "chain":
            assert (I[:n] == p.ids).all() and (np.diff(D[:n].astype(np.float64)) < -CHAIN_GAP).all(), (s.name, p.row, I[:n], p.ids, D[:n])
        elif p.kind == "ladder":
            assert set(I[:n].tolist()) == set(p.ids.tolist()), (s.name, p.row)
        else:
            assert (D[:n] == D[0]).all() and (I[:n] == np.sort(p.ids)).all(), (s.name, p.row)


def _sides(cuts, length, taken):
    """the other side of every cut position: p - 1 and p + 1 where they exist and are free"""
    out = []
    for p in cuts:
        for o in (p - 1, p + 1):
            if 0 <= o < length and o not in taken and o not in out:
                out.append(o)
    return out


# ------------------------------------------------------------------------------------------------- list-major
def _list_major_sizes(seg, long_extra=1):
    return [8 * seg + long_extra, 4 * seg, 4 * seg + 1, seg, 1, 0, 1025, 2049]


def _list_major(name, seed, M):
    """Eight lists, all probed.  List 0 is two whole chunks and ONE more code: single winners at both sides of the stride (1024, 2048),
    segment and chunk cuts and on the lone last code (a chunk, a segment and a thread pair of one code, "summed twice"); further
    single winners on the only code of list 4, the lone code that is chunk 1 of list 2, the last code of the one-segment list 3.
    The ladder takes the other side of every cut and the first and last code of the other lists."""
    seg = R.seg_of(M)
    sizes = _list_major_sizes(seg)
    cuts = [0, 1, 1023, 1024, 2047, 2048, seg - 1, seg, 4 * seg - 1, 4 * seg, 8 * seg - 1, 8 * seg]
    singles = [(0, p) for p in cuts] + [(4, 0), (2, 4 * seg), (3, seg - 1)]
    ladder = [(0, o) for o in _sides(cuts, sizes[0], cuts)]
    ladder += [(1, 0), (1, 4 * seg - 1), (2, 0), (2, 4 * seg - 1), (3, 0), (6, 0), (6, 1023), (6, 1024), (7, 0), (7, 2047), (7, 2048)]
    return _build(name, seed, M, sizes, [("chain", [w]) for w in singles] + [("ladder", ladder)])


ROW_NUMBERS = (0, 511, 512, 1023)


def _list_major_row_numbers(name, seed):
    """The list-major shape searched with a full pass of 1024 query rows: the pair record keeps the row in 10 bits next to the chunk.
    Rows 0, 511, 512 and 1023 each have their winner in chunk 1 of the long list and their runner-up in chunk 2.  (The long list of
    the first set has ONE code in chunk 2; here it has four, one per row.)  The restatement is computed for those four rows and
    eight random others."""
    seg = R.seg_of(96)
    sizes = _list_major_sizes(seg, long_extra=4)
    planted = [("chain", [(0, 4 * seg + 1000 * i), (0, 8 * seg + i)]) for i in range(4)]
    others = np.random.default_rng(seed + 1).choice(np.setdiff1d(np.arange(1024), ROW_NUMBERS), 8, replace=False).tolist()
    return _build(name, seed, 96, sizes, planted, n_q=1024, row_of=ROW_NUMBERS, ref_rows=others)


# ------------------------------------------------------------------------------------------------- row-major
def _row_major_equal(name, seed, length):
    """128 equal lists, all probed: two groups of 64 lists, each group's sequence cut into units at 12288 and 24576.  Whatever order the
    coarse quantizer emits the lists in, virtual code c * 12288 of a group is offset c * 12288 mod length of some list: planting at
    those offsets, the ones before them and the first and last code of EVERY list puts a winner on both sides of every cut."""
    nlist, seg = 128, R.seg_of(96)
    offs = {0, length - 1}
    for c in (1, 2):
        offs |= {(c * seg) % length, ((c * seg) % length - 1) % length}
    offs = sorted(offs)
    singles = [(5, o) for o in offs] + [(0, 0), (127, length - 1)]
    ladder = [(l, o) for l in range(nlist) for o in offs if (l, o) not in singles]
    assert len(ladder) <= 1024
    return _build(name, seed, 96, [length] * nlist, [("chain", [w]) for w in singles] + [("ladder", ladder)])


RAGGED_LENGTHS = (0, 1, 2, 63, 64, 65, 700, 3000)


def _row_major_ragged(name, seed, nlist):
    """Lists of very different lengths, empty ones forced at the first, a middle and the last list number, all probed: nlist = 100 is a
    full group and a partial one (36 lists, 28 empty slots), nlist = 65 a full group and a group of ONE list.  Ladder on the first
    and last code of every non-empty list; single winners on a list of one code, the last code of a list of two and both ends of
    a long one."""
    rng = np.random.default_rng(seed)
    sizes = rng.permutation(np.resize(np.asarray(RAGGED_LENGTHS), nlist))
    sizes[[0, nlist // 2, nlist - 1]] = 0
    first = {v: int(np.nonzero(sizes == v)[0][0]) for v in (1, 2, 65, 3000)}
    singles = [(first[1], 0), (first[2], 1), (first[65], 0), (first[3000], 0), (first[3000], 2999)]
    ladder = []
    for l in np.nonzero(sizes)[0]:
        for o in sorted({0, int(sizes[l]) - 1}):
            if (int(l), o) not in singles:
                ladder.append((int(l), o))
    return _build(name, seed + 1, 96, sizes, [("chain", [w]) for w in singles] + [("ladder", ladder)])


SAMPLED_N = 8188


def _row_major_sampled(name, seed):
    """One group whose only non-empty list is ONE unit of 8188 codes (empty lists at the head and the tail of the group): longer than 2048,
    so for k <= 128 the unit's bound is the k-th of the 1024 sample keys at floor(i n / 1024).  Single winners at sample positions and
    beside them, and in the last 1023 keys of the segment; the ladder fills the REST of those last 1023 keys -- a sample that
    stopped short of them (i * floor(n / 1024) ends at 7161) would have the whole block beat its k-th."""
    n = SAMPLED_N
    at = [(i * n) // 1024 for i in (1, 500, 700)]
    singles = sorted({p + d for p in at for d in (-1, 0, 1)} | {n - 1, n - 512, n - 1023})
    ladder = [o for o in range(n - 1023, n) if o not in singles]
    assert len(ladder) <= 1024 and (1023 * (n // 1024)) < n - 1023
    return _build(name, seed, 96, [0, n, 0, 0], [("chain", [(1, o)]) for o in singles] + [("ladder", [(1, o) for o in ladder])])


# ------------------------------------------------------------------------------------------------- ties
TIE_BLOCKS = (9, 11, 99, 101)          # k - 1 and k + 1 for k = 10 and k = 100
# the large exact block: 400 (list-major), 200 (row-major).  Both stay inside the 512 candidates pq_ensure reserves per row beyond
# the per-segment share (k per segment list-major, 24 k per unit row-major), however the block falls over the segments
TIE_LARGE = {"ties_list_major": 400, "ties_row_major": 200}
TIE_OVER = 5000                        # > PQ_FINAL_CAP = 4096: beyond what the final selection sorts


def _run(l, o, n):
    return [(l, o + i) for i in range(n)]


def _ties_list_major(name, seed):
    """byte-identical best codes inside one list: blocks of 9 / 11 across a segment and a chunk cut, 99 / 101 at the head and the tail
    of a list, 400 across a segment cut, 5000 across another; three ordinary rows and an all-zero row"""
    seg = R.seg_of(96)
    planted = [("block", _run(0, 2 * seg - 4, 9)), ("block", _run(0, 4 * seg - 5, 11)), ("block", _run(2, 0, 99)),
               ("block", _run(2, 9000 - 101, 101)), ("block", _run(0, seg - 200, TIE_LARGE[name])), ("block", _run(1, 10000, TIE_OVER))]
    return _build(name, seed, 96, [4 * seg + 3000, 20000, 9000, 2500], planted, extra=3, zero_row=True)


def _ties_row_major(name, seed):
    """the same on the row-major scan: 63 lists of 400 codes and one of 6000 (it holds the block of 5000), one group"""
    planted = [("block", _run(3, 0, 9)), ("block", _run(10, 389, 11)), ("block", _run(20, 100, 99)), ("block", _run(40, 0, 101)),
               ("block", _run(30, 100, TIE_LARGE[name])), ("block", _run(63, 500, TIE_OVER))]
    return _build(name, seed, 96, [400] * 63 + [6000], planted, extra=3, zero_row=True)


BUILDERS = {
    "list_major_96": lambda n: _list_major(n, 401, 96),
    "list_major_128": lambda n: _list_major(n, 402, 128),
    "list_major_rows": lambda n: _list_major_row_numbers(n, 403),
    "row_major_500": lambda n: _row_major_equal(n, 404, 500),
    "row_major_384": lambda n: _row_major_equal(n, 405, 384),
    "ragged_100": lambda n: _row_major_ragged(n, 406, 100),
    "ragged_65": lambda n: _row_major_ragged(n, 408, 65),
    "sampled": lambda n: _row_major_sampled(n, 410),
    "ties_list_major": lambda n: _ties_list_major(n, 411),
    "ties_row_major": lambda n: _ties_row_major(n, 412),
}
PLANTED_SETS = ("list_major_96", "list_major_128", "row_major_500", "row_major_384", "ragged_100", "ragged_65", "sampled")
ROW_MAJOR = {"row_major_500", "row_major_384", "ragged_100", "ragged_65", "sampled", "ties_row_major"}


@functools.lru_cache(maxsize=None)
def get(name):
    s = BUILDERS[name](name)
    assert s.by_rows == (name in ROW_MAJOR), (name, s.by_rows)
    return s


def chains(s):
    return [p for p in s.planted if p.kind == "chain"]


def ladder(s):
    (p,) = [p for p in s.planted if p.kind == "ladder"]
    return p


# ------------------------------------------------------------------------------------------------- small M
@functools.lru_cache(maxsize=None)
def small_m(M, by_residual):
    """M = 16 / 32: the generic table kernel (48- and 24-dimensional sub-vectors) and one / two 16-byte loads per code; a trained
    6000-code index as in tests/test_pq.py, with and without the <x', centroid> term"""
    from tests._pq_build import _random_index
    ix, xb, rng = _random_index(500 + M + int(by_residual), 6000, 32, M=M)
    ix.index.by_residual = by_residual
    q = (xb[rng.integers(0, 6000, 9)] + rng.normal(0, 0.1, (9, DIM))).astype(np.float32)
    return SimpleNamespace(ix=ix, q=q, M=M)
