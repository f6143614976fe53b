"""The float64 restatement of the doc-addressed window re-score (tests/_window_doc_ref.py) without a GPU: held against what
the reference's own index.py returned on its HDF5 branch behind an OPQ + IVFPQ index (tests/golden/pq_hdf5_cases.json,
recorded by tools/make_golden_pq_hdf5.py), and run over every input set of tests/test_window_doc_direct.py to show that it
decides the arg-max of (almost) every candidate by itself."""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest

from tests import _window_doc_sets as S
from tests._golden import GOLD, load_toy_docs
from tests._window_doc_ref import window_doc_ref


def hdf5_cases():
    cases = json.load(open(os.path.join(GOLD, "pq_hdf5_cases.json")))
    z = np.load(os.path.join(GOLD, "pq_hdf5_vecs.npz"))
    for c in cases:
        c["query_arr"] = z[f"query_{c['query']}"]
    return cases, z["vecs"]


def toy_doc_rows():
    """the toy dump as the doc-row store of a handle: whole documents, ascending doc id, and their f2o CSR"""
    docs = sorted(load_toy_docs(), key=lambda m: int(m.doc_idx))
    assert all(m.start.shape[0] == len(m.f2o_start) for m in docs)
    off = np.concatenate([[0], np.cumsum([m.start.shape[0] for m in docs])]).astype(np.int64)
    return (docs, np.concatenate([m.start for m in docs]).astype(np.int8), np.asarray([m.doc_idx for m in docs], np.int32), off,
            np.concatenate([np.asarray(m.f2o_start) for m in docs]).astype(np.int32))


def compare_hdf5(got, want, vecs, tols=None):
    """`_compare_pq` of tests/test_pq.py with its score tolerance (rtol 2e-6, atol 1e-4: the reference sums fp32 products, and a
    score of 2.3 that is 50 - 47.7 carries the rounding of its terms -- 1.6e-6 of the difference on this dump); the vectors
    within `tols` (same nesting as `got`: the restatement's own bound against fp32 accumulation) or, on the GPU path, within the
    same bound computed by the caller.  _compare_pq's 1e-5 absolute would be too tight here: the own vector is a raw int8 row
    (components up to 128, not up to 8.4) times R, so one fp32 ulp of a component is already 1.5e-5."""
    assert len(got) == len(want)
    for qi, (g, w) in enumerate(zip(got, want)):
        assert len(g) == len(w), f"query {qi}: {len(g)} results vs reference {len(w)}"
        for ri, (a, b) in enumerate(zip(g, w)):
            for key in ("context", "title", "doc_idx", "start_pos", "end_pos", "start_idx", "end_idx", "answer"):
                assert a[key] == b[key], f"query {qi} result {ri} field {key}: {a[key]!r} != {b[key]!r}"
            assert np.isclose(a["score"], b["score"], rtol=2e-6, atol=1e-4), (qi, ri, a["score"], b["score"])
            for key in ("start_vec", "end_vec"):
                if b.get(key) is None:
                    assert a.get(key) is None
                else:
                    tol = tols[qi][ri][key]
                    err = np.abs(np.asarray(a[key], np.float64) - vecs[b[key]].astype(np.float64))
                    assert (err <= tol).all(), (qi, ri, key, err.max(), np.nonzero(err > tol)[0][:5])


def restated_search(c, A, with_tol=True):
    """MIPS.search of the HDF5 branch from the golden's own dense stage: both window passes by the restatement, then
    search_phrase's host half and aggregate_results as densephrases_amd.MIPS restates them in python"""
    from densephrases_amd.index import MIPS
    docs, rows, doc_ids, off, f2o = toy_doc_rows()
    sdoc, sword, sI, edoc, eword, eI, sD, eD = [np.asarray(a) for a in c["dense"]]
    B, k, L = c["B"], c["top_k"], c["L"]
    q = c["query_arr"].astype(np.float32)
    held = lambda i: 0 <= i < 261          # noqa: E731
    r1 = window_doc_ref(rows, doc_ids, off, f2o, q[:, 768:], sI, sdoc, sword, sD.astype(np.float32), k, L, 0, held, A=A)
    r2 = window_doc_ref(rows, doc_ids, off, f2o, q[:, :768], eI, edoc, eword, eD.astype(np.float32), k, L, 1, held, A=A)
    fake = SimpleNamespace(store=SimpleNamespace(doc_meta={int(m.doc_idx): m for m in docs}.__getitem__), adjust=MIPS.adjust,
                           adjust_sent=MIPS.adjust_sent)
    flat = lambda a: np.reshape(np.asarray(a), [-1]).astype(np.int64)          # noqa: E731

    def assemble(x1, x2):
        v1 = (x1[:, 0], x1[:, 1]) if c["return_idxs"] else None
        v2 = (x2[:, 0], x2[:, 1]) if c["return_idxs"] else None
        out = MIPS._assemble_py(fake, B, k, flat(sdoc), flat(sword), flat(edoc), flat(eword), r1.pred_word, r1.best, r2.pred_word, r2.best,
                                v1, v2, c["return_sent"])
        if c["aggregate"]:
            out = [MIPS._aggregate_results_py(res, k, None, c["agg_strat"]) for res in out]
        return out

    got = assemble(r1.vecs, r2.vecs)
    tols = None
    if c["return_idxs"] and with_tol:
        t = assemble(r1.vec_tol_ref, r2.vec_tol_ref)
        tols = [[{"start_vec": x["start_vec"], "end_vec": x["end_vec"]} for x in res] for res in t]
    return got, tols, (r1, r2)


def test_restatement_reproduces_the_reference_goldens_of_the_hdf5_branch():
    from oracle.make_golden_pq import build_index
    A = build_index(dict(np.load(os.path.join(GOLD, "pq_index.npz")))).chain[0].A
    cases, vecs = hdf5_cases()
    assert [(c["L"], c["return_idxs"]) for c in cases].count((20, True)) == 1 and len(cases) == 7
    past_end = 0
    for c in cases:
        got, tols, (r1, r2) = restated_search(c, A)
        compare_hdf5(got, c["results"], vecs, tols)
        past_end += int((r1._slot_rows < 0).any(1).sum() + (r2._slot_rows < 0).any(1).sum())
    assert past_end > 0                     # windows that ran past a document end were among them


@pytest.mark.parametrize("variant", S.VARIANTS)
def test_restatement_decides_99_percent_of_every_doc_addressed_input_set(variant):
    seen = past = hit_L = 0
    for name, v, b in S.sets(variant):
        r = S.run_ref(v, b)
        left = r.left_out()
        assert len(left) <= 0.01 * len(b.ids), f"{name}: the restatement leaves {len(left)} of {len(b.ids)} candidates undecided: {left}"
        seen += 1
        past += int(((r._slot_rows < 0).any(1) & (r._slot_rows >= 0).any(1)).sum())
        # the f2o steps of the 70-row document: some arg-max sits exactly L away from its candidate
        tok = b.meta.f2o[b.meta.f2o_off[S.STEP_DOC]:b.meta.f2o_off[S.STEP_DOC + 1]].astype(np.int64)
        for c in np.nonzero(b.doc == S.DOC_IDS[S.STEP_DOC])[0]:
            s = int(r.argslot[c])
            if r.valid[c, s] and b.L > 1 and abs(int(tok[int(r.slot_words[c, s])]) - int(tok[int(b.word[c])])) == b.L:
                hit_L += 1
    assert seen == 2 * len(S.L_ALL) * (len(S.SHAPES) + 1) and past > 50 and hit_L > 0


def test_window_rows_is_refused_where_it_means_nothing(tmp_path):
    from densephrases_amd import MIPS
    from densephrases_amd.dump import DocMeta, DocStore
    from tests._golden import load_toy_docs
    docs = [DocMeta(m.doc_idx, m.title, m.context, m.f2o_start, m.word2char_start, m.word2char_end, m.start) for m in load_toy_docs()]
    store = DocStore(docs)
    for kw in ("raw", "reference", "reconstructed"):
        with pytest.raises(ValueError, match="window_rows"):
            MIPS.from_store(store, window_rows=kw)                            # a flat index
        with pytest.raises(ValueError, match="window_rows"):
            MIPS.from_store(store, window_rows=kw, ivf={"nlist": 4})
        with pytest.raises(ValueError, match="window_rows"):
            MIPS.from_store(store, window_rows=kw, pq={"trained": "nowhere.faiss"})
    with pytest.raises(ValueError, match="window_rows"):
        MIPS.from_store(store, window_rows="hdf5")
    # the whole-document iterator of the in-memory store: f2o-CSR order (ascending doc id), full documents, any block size
    ids, off, _ = store.f2o_csr()
    for block in (1, 50, 1 << 18):
        got = np.zeros((int(off[-1]), 768), np.int8)
        seen = 0
        for r0, rows in store.iter_doc_row_blocks(block=block):
            got[r0:r0 + len(rows)] = rows
            seen += len(rows)
        assert seen == int(off[-1])
        np.testing.assert_array_equal(got, np.concatenate([store.docs[int(d)].start for d in ids]))


def test_reference_dump_streams_whole_documents_in_f2o_csr_order(tmp_path):
    """h5.ReferenceDump.iter_doc_row_blocks over real HDF5 files: every document's full `start` dataset, ascending doc id, blocks of
    whole documents written into the buffers handed in, in turn"""
    from densephrases_amd.h5 import ReferenceDump
    from tests.test_pq import INDEX_NAME, _write_pq_layout
    root = _write_pq_layout(str(tmp_path / "dump"))
    dump = ReferenceDump(os.path.join(root, "phrase"), os.path.join(root, "start", INDEX_NAME, "idx2id.hdf5"))
    _, rows, doc_ids, off, _ = toy_doc_rows()
    ids, off2, _ = dump.f2o_csr()
    np.testing.assert_array_equal(ids, doc_ids)
    np.testing.assert_array_equal(off2, off)
    bufs = [np.full((64, 768), 99, np.int8), np.full((64, 768), 99, np.int8)]
    got = np.zeros_like(rows)
    turn = seen = 0
    for r0, blk in dump.iter_doc_row_blocks(block=64, buffers=bufs):
        assert r0 in off.tolist() and r0 + len(blk) in off.tolist()              # whole documents
        if len(blk) <= 64:
            assert np.shares_memory(blk, bufs[turn % 2])
        got[r0:r0 + len(blk)] = blk
        seen += len(blk)
        turn += 1
    assert seen == len(rows) and turn > 2
    np.testing.assert_array_equal(got, rows)
    # a rank's range: the documents of its rows only, offsets from zero
    lo, hi = int(dump.doc_starts()[2]), dump.n_rows
    ids_r, off_r, _ = dump.f2o_csr(lo, hi)
    part = np.concatenate([blk for _, blk in dump.iter_doc_row_blocks(lo, hi)])
    want = np.concatenate([rows[off[list(doc_ids).index(d)]:off[list(doc_ids).index(d) + 1]] for d in ids_r])
    np.testing.assert_array_equal(part, want)
    assert len(part) == int(off_r[-1]) < len(rows)
