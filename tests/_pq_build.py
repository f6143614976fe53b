"""Synthetic OPQ + IVFPQ indexes in the reference's format (oracle/ivfpq_oracle.py trains and fills them) and their
resident shards: shared by tests/test_pq.py, tests/test_window_direct.py and tests/_adc_sets.py."""
import numpy as np

from densephrases_amd import faiss_io as F
from oracle import ivfpq_oracle as P


def _random_index(seed, n, nlist, M=96, id_offset=0, dup=0):
    rng = np.random.default_rng(seed)
    centres = rng.normal(0, 0.5, (max(4, nlist // 2), 768)).astype(np.float32)
    xb = (centres[rng.integers(0, len(centres), n)] + rng.normal(0, 0.3, (n, 768))).astype(np.float32)
    if dup:
        xb[rng.choice(n, dup, replace=False)] = xb[0]               # identical vectors -> identical codes -> score ties
    ix = P.train(xb[: min(n, 3000)], nlist=nlist, M=M, seed=seed + 1)
    ids = np.arange(n, dtype=np.int64) + id_offset
    P.add_with_ids(ix, xb, ids)
    return ix, xb, rng


def _shard(ix):
    from densephrases_amd import Shard
    s = Shard.from_faiss_index(ix, device=0)
    n = s.ntotal
    s.set_idx2id(np.zeros(n, np.int32), np.arange(n, dtype=np.int32))
    s.set_f2o(np.zeros(1, np.int32), np.asarray([0, n], np.int64), np.arange(n, dtype=np.int32))
    s.finalize()
    return s


def _index_from_list_numbers(rng, nlist, M, lists, cent, ids=None):
    """an IndexPreTransform(OPQ) -> IndexIVFPQ whose code i (random bytes) lies in list lists[i]"""
    n = len(lists)
    pqc = rng.normal(0, 0.1, (M, 256, 768 // M)).astype(np.float32)
    codes = rng.integers(0, 256, (n, M), dtype=np.uint8)
    order = np.argsort(lists, kind="stable")
    ids = np.arange(n, dtype=np.int64) if ids is None else ids
    list_codes = [np.zeros((0, M), np.uint8)] * nlist
    list_ids = [np.zeros(0, np.int64)] * nlist
    ls, cs, is_ = lists[order], codes[order], ids[order]
    cuts = np.nonzero(np.diff(ls))[0] + 1
    for seg_l, seg_c, seg_i in zip(np.split(ls, cuts), np.split(cs, cuts), np.split(is_, cuts)):
        if len(seg_l):
            list_codes[int(seg_l[0])], list_ids[int(seg_l[0])] = seg_c, seg_i
    A = P.random_rotation(768, rng)
    ix = F.PreTransformIndex([F.LinearTransform(A)], F.IVFPQIndex(768, nlist, M, 8, cent, pqc, list_codes, list_ids, True, 0, 1, 2), 768, True)
    return ix, A
