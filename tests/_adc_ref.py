"""The ADC scan of a PQ index (csrc/dph_pq.hip: pq_pairs_kernel / pq_units_kernel, pq_adc_kernel, pq_adc_rows_kernel,
pq_segment_finish, pq_final_kernel) restated in numpy on top of oracle/ivfpq_oracle.py -- apply_chain, coarse_probe, lut and
adc_scores do the arithmetic, nothing of it is derived again here.  Per query row: the probed lists, the fp32 sequential ADC
score of every probed code with its position in the code array and its id, the top-k by (score desc, id asc), and the WORK the
scan must cut out of that: (list, row) pairs per chunk of four segments (list-major), units of one segment of a group of 64
probed lists (row-major), and the bound a list-major row must end with.  The constants are the kernel's.  No GPU."""
from types import SimpleNamespace

import numpy as np

from oracle import ivfpq_oracle as P

PQ_THREADS = 1024          # threads of a scan workgroup: the stride of its loops, the size of the bound's sample
PQ_SEG = 12288             # codes per segment (M <= 96), halved for larger M
PQ_LM_CHUNK = 4            # segments per (list, row) pair record of the list-major scan
PQ_GROUP = 64              # probed lists per group of the row-major scan
PQ_FINAL_CAP = 4096        # candidates pq_final_kernel sorts
RTOL, ATOL = 3e-7, 1e-5    # the tolerance of tests/test_pq.py::_same_topk: x' and the tables are float64 sums in another order


def seg_of(M):
    return PQ_SEG if M <= 96 else PQ_SEG // 2


def list_sizes(ix):
    return np.asarray([len(i) for i in ix.index.list_ids], dtype=np.int64)


def by_rows(ix):
    """pq_by_rows: many short lists on average -> the row-major scan"""
    sizes = list_sizes(ix)
    return int(sizes.sum()) // len(sizes) < 2048 and int(sizes.max()) < (1 << 24)


def pq_key(s):
    """order-preserving uint32 of an fp32 score: larger score <=> larger key, key 0 below every score"""
    b = np.ascontiguousarray(s, dtype=np.float32).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def pq_unkey(k):
    k = np.ascontiguousarray(k, dtype=np.uint32)
    return np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(np.float32)


class Row:
    """one query row's probed codes, concatenated in probe order (best list first)"""

    def __init__(self, lists, dis0, scores, pos, ids, lst):
        self.lists, self.dis0 = lists, dis0
        self.scores, self.pos, self.ids, self.lst = scores, pos, ids, lst
        self.probed = len(scores)
        self._order = np.lexsort((ids, -scores.astype(np.float64)))

    def topk(self, k):
        """(scores [min(k, probed)] descending, ids) by (score desc, id asc)"""
        o = self._order[:k]
        return self.scores[o], self.ids[o]

    def topk_padded(self, k):
        D, I = np.full(k, P.NEG, np.float32), np.full(k, -1, np.int64)
        s, i = self.topk(k)
        D[:len(s)], I[:len(i)] = s, i
        return D, I

    def kth(self, k):
        """the k-th best score, None when fewer than k codes were probed"""
        return None if self.probed < k else self.scores[self._order[k - 1]]

    def list_major_bound(self, k, seg):
        """What the row's running bound must be once the list-major scan is done: the maximum, over the segments that hold >= k
        codes, of the segment's k-th largest score; None when no segment does (the bound word stays 0).  Segments = consecutive
        runs of <= seg codes from each list's start (a chunk is four of them).  Order-free: a segment whose k-th exceeds the bound
        it reads has >= k keys at or above that bound, so it always raises it (atomicMax); one whose k-th does not, cannot."""
        best = None
        for l in self.lists:
            s = self.scores[self.lst == l]
            for a in range(0, len(s), seg):
                part = s[a:a + seg]
                if len(part) >= k:
                    kth = np.partition(part, len(part) - k)[len(part) - k]
                    best = kth if best is None or kth > best else best
        return best


def adc_rows(ix, q, nprobe):
    """[Row] for the query rows q [n, 768]"""
    ivf = ix.index
    sizes = list_sizes(ix)
    off = np.concatenate([[0], np.cumsum(sizes)])
    xp = P.apply_chain(ix.chain, q)
    lists, dis0 = P.coarse_probe(xp, ivf.centroids, nprobe)
    tables = P.lut(xp, ivf.pq_centroids)
    out = []
    for r in range(xp.shape[0]):
        ss, pp, ii, ll = [np.zeros(0, np.float32)], [np.zeros(0, np.int64)], [np.zeros(0, np.int64)], [np.zeros(0, np.int64)]
        for l, d0 in zip(lists[r], dis0[r]):
            if sizes[l] == 0:
                continue
            base = d0 if ivf.by_residual else np.float32(0)
            ss.append(P.adc_scores(base, tables[r], np.asarray(ivf.list_codes[l])))
            pp.append(off[l] + np.arange(sizes[l], dtype=np.int64))
            ii.append(np.asarray(ivf.list_ids[l], dtype=np.int64))
            ll.append(np.full(sizes[l], l, np.int64))
        out.append(Row(lists[r], dis0[r], np.concatenate(ss), np.concatenate(pp), np.concatenate(ii), np.concatenate(ll)))
    return out


def probe_lists(ix, q, nprobe):
    """[n, min(nprobe, nlist)] probed lists of every row, best first (no scores: the work counts need no more)"""
    return P.coarse_probe(P.apply_chain(ix.chain, q), ix.index.centroids, nprobe)[0]


def work(sizes, lists, seg):
    """The work records of one pass over the rows whose probed lists are lists [n, nprobe] (sizes = codes of every list).
    pairs: list-major, one per (row, probed non-empty list, chunk of PQ_LM_CHUNK segments).  units_lo <= units <= units_hi:
    row-major, one per segment of every group of PQ_GROUP probed lists.  Which lists share a group is the coarse quantizer's
    emission order, which nothing here may assume: the count is exact (lo == hi) when that cannot matter -- one group, or probed
    lists of equal length -- and otherwise bracketed by ceil(total / seg) and that plus one partial segment per further group."""
    sizes = np.asarray(sizes, dtype=np.int64)
    chunk = seg * PQ_LM_CHUNK
    pairs = lo = hi = 0
    for row in np.asarray(lists):
        ln = sizes[row]
        pairs += int(((ln + chunk - 1) // chunk).sum())
        groups = (len(row) + PQ_GROUP - 1) // PQ_GROUP
        total = int(ln.sum())
        if groups == 1 or (ln == ln[0]).all():
            n = sum(-(-int(ln[g * PQ_GROUP:(g + 1) * PQ_GROUP].sum()) // seg) for g in range(groups))
            lo, hi = lo + n, hi + n
        else:
            lo += -(-total // seg)
            hi += -(-total // seg) + groups - 1
    return SimpleNamespace(pairs=pairs, units_lo=lo, units_hi=hi)


def same_topk(D, I, Dr, Ir):
    """tests/test_pq.py::_same_topk, imported late (that module imports the GPU package's file reader only: fine on a CPU)"""
    from tests.test_pq import _same_topk
    _same_topk(D, I, Dr, Ir)
