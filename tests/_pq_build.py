"""Synthetic OPQ + IVFPQ indexes in the reference's format (oracle/ivfpq_oracle.py trains and fills them) and their
resident shards: shared by tests/test_pq.py and tests/test_window_direct.py."""
import numpy as np

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
