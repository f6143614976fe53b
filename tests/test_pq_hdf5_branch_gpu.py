"""MIPS(window_rows=...) over a real OPQ + IVFPQ index file: the HDF5 branch of the reference's search_phrase (index.py:246-273)
served from raw int8 rows resident next to the codes, against goldens the reference's own index.py recorded over the same
layout WITHOUT meta_compressed.pkl (tools/make_golden_pq_hdf5.py); with the pkl in place "reference" resolves to the RAM
branch and nothing changes; range-sharded ranks equal the single rank."""
import os
import threading

import numpy as np
import pytest

from tests.test_pq import INDEX_NAME, _compare_pq, _golden_index, _pq_cases, _write_pq_layout
from tests.test_window_doc_ref import compare_hdf5, hdf5_cases, restated_search

pytestmark = pytest.mark.gpu


def _paths(root):
    idx_dir = os.path.join(root, "start", INDEX_NAME)
    return dict(phrase_dump_dir=os.path.join(root, "phrase"), index_path=os.path.join(idx_dir, "index.faiss"),
                idx2id_path=os.path.join(idx_dir, "idx2id.hdf5"), cuda=True)


def _search(mips, c):
    return mips.search(c["query_arr"].astype(np.float64), q_texts=[f"q{i}" for i in range(c["B"])], top_k=c["top_k"],
                       aggregate=c["aggregate"], return_idxs=c["return_idxs"], max_answer_length=c["L"],
                       agg_strat=c["agg_strat"], return_sent=c["return_sent"])


def test_reference_keyword_without_the_pkl_reproduces_the_hdf5_branch_goldens(tmp_path):
    from densephrases_amd import MIPS
    root = _write_pq_layout(str(tmp_path / "dump"))
    os.unlink(os.path.join(root, "meta_compressed.pkl"))
    mips = MIPS(window_rows="reference", **_paths(root))
    assert mips.window_rows == "raw" and mips.shard.n_doc_rows == 261 and mips.index.ntotal == 261
    A = _golden_index().chain[0].A
    np.testing.assert_array_equal(mips.R, A)
    cases, vecs = hdf5_cases()
    for c in cases:
        dense = mips.search_dense(c["query_arr"], q_texts=None, top_k=c["top_k"])
        for got, want in zip(dense, c["dense"]):
            want = np.asarray(want)
            if want.dtype.kind == "f":
                np.testing.assert_allclose(np.asarray(got), want, rtol=3e-7, atol=1e-5)
            else:
                np.testing.assert_array_equal(np.asarray(got), want)
        # the vectors: within the restatement's bound against the reference's fp32 accumulation (tests/_window_doc_ref.py)
        _, tols, _ = restated_search(c, A)
        compare_hdf5(_search(mips, c), c["results"], vecs, tols)
        # ... and the two-stage form answers the same
        two = mips.search_phrase(c["query_arr"], *dense, top_k=c["top_k"], max_answer_length=c["L"], return_idxs=c["return_idxs"],
                                 return_sent=c["return_sent"])
        if not c["aggregate"]:
            compare_hdf5(two, c["results"], vecs, tols)
    mips.close()


def test_with_the_pkl_present_reference_means_reconstructed_and_nothing_changed(tmp_path):
    from densephrases_amd import MIPS
    root = _write_pq_layout(str(tmp_path / "dump"))
    cases, vecs = _pq_cases()
    plain = MIPS(**_paths(root))
    want = [_search(plain, c) for c in cases]
    plain.close()
    for kw in ("reference", "reconstructed"):
        mips = MIPS(window_rows=kw, **_paths(root))
        assert mips.window_rows == "reconstructed" and not hasattr(mips.shard, "n_doc_rows")
        for c, w in zip(cases, want):
            got = _search(mips, c)
            _compare_pq(got, c["results"], vecs)
            _same(got, w)                                      # bit for bit what the keyword-less object answers
        mips.close()


def _same(got, ref):
    assert len(got) == len(ref)
    for g, w in zip(got, ref):
        assert len(g) == len(w)
        for x, y in zip(g, w):
            for key in ("context", "title", "doc_idx", "start_pos", "end_pos", "start_idx", "end_idx", "answer"):
                assert x[key] == y[key], (key, x[key], y[key])
            assert x["score"] == y["score"]
            if y.get("start_vec") is not None:
                np.testing.assert_array_equal(x["start_vec"], y["start_vec"])
                np.testing.assert_array_equal(x["end_vec"], y["end_vec"])


@pytest.mark.parametrize("world", [2, 3])
def test_raw_rows_range_sharded_over_ranks_equal_the_single_rank(tmp_path, world):
    """every rank keeps the raw rows of the documents of its own range; the merged records and the SUMMED vectors are the single rank's"""
    from densephrases_amd import MIPS
    from tests.test_gpu_search import _ThreadWorld
    root = _write_pq_layout(str(tmp_path / "dump"))
    paths = _paths(root)
    single = MIPS(window_rows="raw", **paths)
    cases, _ = hdf5_cases()
    want = [_search(single, c) for c in cases]
    single.close()
    tw = _ThreadWorld(world)
    results, errors = [None] * world, []

    def run(rank):
        try:
            m = MIPS(rank=rank, world=world, dist=tw.rank_view(rank), device=0, window_rows="raw", **paths)
            assert 0 < m.shard.n_doc_rows < 261 and m.index.ntotal == 261
            results[rank] = ([_search(m, c) for c in cases], m.shard.n_doc_rows)
        except Exception as e:                       # surface in the main thread; release the peers
            errors.append((rank, repr(e)))
            tw.bar.abort()

    threads = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=300)
    assert not errors, errors
    assert sum(r[1] for r in results) == 261
    for rank in range(world):
        for got, ref in zip(results[rank][0], want):
            _same(got, ref)


def test_attach_misuse_returns_codes_with_messages():
    """dph_index_attach_doc_rows: NULL / zero arguments, a non-PQ handle, a second attach, an attach after finalize; dph_index_finalize
    with a row count that is not the f2o table's, and with rows missing"""
    from densephrases_amd import Shard, _lib
    lib = _lib.lib
    E_ARG, E_STATE = -1, -4

    def refused(rc, code, *words):
        msg = lib.dph_last_error().decode()
        assert rc == code and all(w in msg for w in words), (rc, msg)

    refused(lib.dph_index_attach_doc_rows(None, 10), E_ARG, "dph_index_attach_doc_rows")
    flat = Shard(64, device=0)
    refused(lib.dph_index_attach_doc_rows(flat._h, 10), E_STATE, "not a PQ index")
    flat.close()
    from tests import _window_doc_sets as S
    v, m = S.variant("house"), S.meta(10)
    s = Shard.from_faiss_index(v.ix, device=0)
    refused(lib.dph_index_attach_doc_rows(s._h, 0), E_ARG, "n_doc_rows")
    refused(lib.dph_index_attach_doc_rows(s._h, -5), E_ARG, "n_doc_rows")
    # uploads on a PQ handle without rows are refused as ever
    refused(lib.dph_index_upload_rows(s._h, 0, 1, _lib._p(S.doc_rows()[:1].copy())), E_ARG, "range")
    s.attach_doc_rows(S.N_DOC_ROWS - 1)
    refused(lib.dph_index_attach_doc_rows(s._h, S.N_DOC_ROWS), E_STATE, "already")
    refused(lib.dph_index_upload_rows(s._h, S.N_DOC_ROWS - 1, 1, _lib._p(S.doc_rows()[:1].copy())), E_ARG, "range")
    s.set_idx2id(m.row2doc, m.row2word)
    s.set_f2o(m.doc_ids, m.f2o_off, m.f2o)
    s.upload(S.doc_rows()[:S.N_DOC_ROWS - 1])
    refused(lib.dph_index_finalize(s._h, None), E_STATE, "f2o", str(S.N_DOC_ROWS))
    s.close()
    s = Shard.from_faiss_index(v.ix, device=0, doc_rows=S.N_DOC_ROWS)
    s.set_idx2id(m.row2doc, m.row2word)
    s.set_f2o(m.doc_ids, m.f2o_off, m.f2o)
    s.upload(S.doc_rows()[:100], 0)
    s.upload(S.doc_rows()[150:], 150)
    refused(lib.dph_index_finalize(s._h, None), E_STATE, "uploaded")
    s.upload(S.doc_rows()[90:160], 90)
    s.finalize()
    refused(lib.dph_index_attach_doc_rows(s._h, S.N_DOC_ROWS), E_STATE, "already")
    # reconstruct still answers the rotated PQ reconstruction
    from oracle import ivfpq_oracle as P
    np.testing.assert_array_equal(s.reconstruct(3), P.reconstruct(v.ix, P.DirectMap(v.ix.index), 3))
    s.close()
    s = Shard.from_faiss_index(v.ix, device=0)
    s.set_idx2id(m.row2doc, m.row2word)
    s.set_f2o(m.doc_ids, m.f2o_off, m.f2o)
    s.finalize()
    refused(lib.dph_index_attach_doc_rows(s._h, S.N_DOC_ROWS), E_STATE, "before dph_index_finalize")
    s.close()
