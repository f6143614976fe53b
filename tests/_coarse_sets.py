"""Centroid sets, query rows and float64 expectations for the tests that look at the coarse quantizer directly
(tests/test_coarse_probe_sets.py).  Test infrastructure, numpy only.

The reveal: an index with exactly ONE row (one PQ code) per inverted list, searched with k = min(nprobe, nlist).  Every probed
list contributes exactly one id and there are no more than k candidates, so the returned ids ARE the probed lists -- nothing but the
coarse quantizer decides the answer."""
import numpy as np

CG_F32_ERR = 768.0 * 5.97e-8          # dph_ivf.hip: |fp32 MFMA dot - exact| <= CG_F32_ERR * ||x|| * ||c||
CS_BAND_CAP = 2048                    # dph_ivf.hip: lists the float64 re-rank of one query row holds
CS_FAST_MIN = 8192                    # dph_ivf.hip: lists from which the one-pass candidate path is tried
BLOCK = 40                            # copies / one-ulp variants planted next to their source centroid

KINDS = ("random", "dup", "ulp", "long")


def centroid_set(kind, nlist, seed):
    """(centroids fp32 [nlist, 768], src, block): `block` = ids of the planted lists (without `src`), scattered over the id range.
      random  N(0, 0.5)
      dup     + min(BLOCK, nlist // 3) exact copies of centroid `src`: exact score ties for every query, resolved by list id
      ulp     + as many one-ulp variants of `src`: copy i differs from `src` in ONE component by one fp32 ulp, and the variants' scores
              against a multiple of `src` are pairwise distinct in float64 (>= 1e-10 apart, 10^3 x the float64 summation noise) while
              the whole block spreads ~1e-7 -- far inside the fp32 error band (~1e-2): only the float64 re-rank can order it
      long    + a few centroids 3 x longer than the rest (they crowd the top of every score row and widen the band)"""
    assert kind in KINDS
    rng = np.random.default_rng(seed)
    cent = rng.normal(0.0, 0.5, (nlist, 768)).astype(np.float32)
    src = int(rng.integers(0, nlist))
    block = np.zeros(0, np.int64)
    if kind in ("dup", "ulp"):
        nb = min(BLOCK, nlist // 3)
        block = np.sort(rng.choice(np.setdiff1d(np.arange(nlist), [src]), nb, replace=False))
        cent[block] = cent[src]
        if kind == "ulp":
            c = cent[src]
            # what moving component j by one ulp adds to <src, variant>: |c_j| * ulp(c_j); components picked so that the signed
            # contributions of the block are evenly spread and pairwise distinct
            contrib = np.abs(c).astype(np.float64) * np.spacing(np.abs(c)).astype(np.float64)
            elig = np.nonzero(np.abs(c) >= 0.25)[0]
            elig = elig[np.argsort(contrib[elig])]
            pick = elig[np.linspace(0, len(elig) - 1, nb).astype(int)]
            assert len(np.unique(pick)) == nb
            for i, (l, j) in enumerate(zip(block, pick)):
                up = i % 2 == 0                                   # away from zero: score up; towards zero: score down
                cent[l, j] = np.nextafter(c[j], np.float32(np.inf if (c[j] > 0) == up else -np.inf), dtype=np.float32)
            s = cent[np.concatenate([[src], block])].astype(np.float64) @ c.astype(np.float64)
            assert np.diff(np.sort(s)).min() > 1e-10 and s.max() - s.min() < 1e-5
    if kind == "long":
        block = np.sort(rng.choice(np.setdiff1d(np.arange(nlist), [src]), min(5, nlist // 3), replace=False))
        cent[block] *= np.float32(3.0)
    return cent, src, block


def query_rows(cent, src, block, kind, n_q, seed):
    """n_q query rows: random N(0, 0.5) rows, and -- at rows 0, 1, 2 and around the 128-row tile edge where they exist -- multiples of
    the source centroid (dup / ulp: the whole block lies on top, in one exact tie or in one float64-only order) or of a long one."""
    rng = np.random.default_rng(seed)
    x = rng.normal(0.0, 0.5, (n_q, 768)).astype(np.float32)
    base = cent[block[0]] if kind == "long" else cent[src]
    for r, f in ((0, 1.0), (1, 0.5), (2, 2.0), (126, 1.0), (128, 0.25), (n_q - 1, 1.0)):
        if kind != "random" and 0 <= r < n_q:
            x[r] = base * np.float32(f)
    return x


def block_nprobes(block, nlist):
    """nprobe values that put the probe boundary before, inside, at the end of and just past a block that lies on top"""
    nb = len(block) + 1                     # with its source
    return sorted({p for p in (1, 2, nb // 2, nb - 1, nb, nb + 1) if 1 <= p})


def float64_order(x, cent):
    """(s64 [n, nlist], order [n, nlist]): the float64 scores and every row's lists in (score desc, list id asc) order"""
    s64 = x.astype(np.float64) @ cent.astype(np.float64).T
    ids = np.broadcast_to(np.arange(cent.shape[0]), s64.shape)
    return s64, np.lexsort((ids, -s64), axis=1)


def band_occupancy(s64, order, k, x, cent, err_rel=CG_F32_ERR):
    """lists per query row whose float64 score lies within 4 delta of the k-th score t, delta = err_rel ||x|| max||c||.  The kernel
    collects the fp32 scores within 2 * 1.5 delta of the fp32 k-th score (its slack of 1.5); fp32 and float64 differ by <= delta each,
    so 4 delta in float64 covers what it can collect."""
    t = np.take_along_axis(s64, order[:, k - 1:k], 1)
    cmax = np.sqrt((cent.astype(np.float64) ** 2).sum(1).max())
    delta = err_rel * np.sqrt((x.astype(np.float64) ** 2).sum(1)) * cmax
    return (np.abs(s64 - t) <= 4.0 * delta[:, None]).sum(1)


def explain(got_row, order_row, s64_row, k, block, src):
    """what a mismatching row tells: extra / missing lists with their float64 ranks, scores and block membership"""
    want = set(order_row[:k].tolist())
    got = set(int(v) for v in got_row.tolist())
    rank = {int(l): i for i, l in enumerate(order_row.tolist())}
    blk = set(block.tolist()) | {src}
    def fmt(ls):
        return [(l, rank.get(l, -1), float(s64_row[l]) if 0 <= l < len(s64_row) else None, l in blk) for l in sorted(ls)[:8]]
    return (f"k={k} boundary score {float(s64_row[order_row[k - 1]])!r}: extra (list, f64 rank, score, in block) {fmt(got - want)}; "
            f"missing {fmt(want - got)}")
