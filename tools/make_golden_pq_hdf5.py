#!/usr/bin/env python3
"""Goldens for the HDF5 branch of the reference's window re-score behind an OPQ + IVFPQ index: the REFERENCE's own MIPS
(densephrases/index.py, loaded unmodified through oracle/refshim) over the toy layout and the index of
oracle/make_golden_pq.py (261 rows, nlist 4, M 96, R = Householder x permutation) -- with meta_compressed.pkl REMOVED, so
that index.py:72 takes "Will read metadata directly from hdf5 files" (:246-273): the windows are the dump's raw int8 `start`
rows, addressed by word inside the document, de-quantised and multiplied by R; return_idxs hands out the raw own row.

    python tools/make_golden_pq_hdf5.py          (needs the reference's sources, like the oracle/make_golden* scripts)

Reads tests/golden/pq_index.npz (the committed index pieces) and writes tests/golden/pq_hdf5_cases.json +
pq_hdf5_vecs.npz: data only.  The six parameter rows of make_golden_pq.py plus one more return_idxs row with L = 20, whose
windows run past both ends of the toy documents."""
from __future__ import annotations

import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from densephrases_amd import faiss_io                    # noqa: E402
from oracle import refshim                                # noqa: E402
from oracle.make_golden import jsonable, write_reference_layout      # noqa: E402
from oracle.make_golden_pq import INDEX_NAME, build_index              # noqa: E402
from oracle.synth_dump import make_queries                # noqa: E402

ROWS = [
    (4, 5, 10, False, "opt1", False, False),
    (4, 5, 10, True, "opt1", False, False),
    (3, 10, 3, True, "opt3", False, False),
    (2, 3, 10, False, "opt1", True, False),
    (3, 8, 10, True, "opt2", False, True),
    (1, 20, 10, False, "opt1", False, False),
    (2, 3, 20, False, "opt1", True, False),
]


def main():
    from tests._golden import GOLD, load_toy_docs
    ref = refshim.install()
    docs = load_toy_docs()
    rng = np.random.default_rng(78)
    cases, vec_store, query_store = [], [], []
    with tempfile.TemporaryDirectory() as tmp:
        dump_dir, idx = write_reference_layout(tmp, docs, INDEX_NAME)
        os.unlink(os.path.join(dump_dir, "meta_compressed.pkl"))
        index = build_index(dict(np.load(os.path.join(GOLD, "pq_index.npz"))))
        idx_dir = os.path.join(dump_dir, "start", INDEX_NAME)
        faiss_io.write_index(index, os.path.join(idx_dir, "index.faiss"), ondisk=True)
        mips = ref.MIPS(phrase_dump_dir=os.path.join(dump_dir, "phrase"), index_path=os.path.join(idx_dir, "index.faiss"),
                        idx2id_path=os.path.join(idx_dir, "idx2id.hdf5"), cuda=False)
        assert mips.index.ntotal == idx.xb.shape[0] and mips.max_idx == 1e9 and mips.doc_groups is None
        for (B, k, L, agg, strat, ridx, sent) in ROWS:
            q = make_queries(rng, idx.xb, B)
            query_store.append(q.astype(np.float32))
            dense = mips.search_dense(q, q_texts=None, top_k=k)
            res = mips.search(q.astype(np.float64), q_texts=[f"q{i}" for i in range(B)], top_k=k, aggregate=agg,
                              return_idxs=ridx, max_answer_length=L, agg_strat=strat, return_sent=sent)
            cases.append({"branch": "pq_hdf5", "B": B, "top_k": k, "L": L, "aggregate": agg, "agg_strat": strat, "return_idxs": ridx,
                          "return_sent": sent, "query": len(query_store) - 1,
                          "dense": [np.asarray(a).tolist() for a in dense], "results": jsonable(res, vec_store)})
    with open(os.path.join(GOLD, "pq_hdf5_cases.json"), "w") as f:
        json.dump(cases, f)
    np.savez_compressed(os.path.join(GOLD, "pq_hdf5_vecs.npz"), vecs=np.stack(vec_store),
                        **{f"query_{i}": q for i, q in enumerate(query_store)})
    print(f"wrote {len(cases)} PQ HDF5-branch cases, {len(vec_store)} vectors")


if __name__ == "__main__":
    main()
