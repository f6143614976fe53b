"""dph_rescore / dph_rescore_dev called directly on PQ handles with the dump's raw rows attached (dph_index_attach_doc_rows):
window_kernel<DocRows> + pq_unrotate_kernel against the float64 restatement of tests/_window_doc_ref.py, by the acceptance rule
of tests/_window_ref.py -- arg-max and pred_word exact wherever the restatement decides them (99 % of every input set:
tests/test_window_doc_ref.py asserts that without a GPU), `best` and the rotated vectors within the tolerance the documented
roundings allow.  The input sets are tests/_window_doc_sets.py: document lengths 0, 1, 2, L - 1, L, L + 1 and ~70, f2o gaps
of L, L - 1 and L + 1, L = 1 / 10 / 20 / 70, partly empty last workgroups, a rotation and a transform that is none, a
non-default codec, a filtered index (ids and dump rows diverge), ids the direct map does not hold, an id-group offset."""
import functools

import numpy as np
import pytest

from tests import _window_doc_sets as S
from tests._window_ref import check

pytestmark = pytest.mark.gpu
DIRECTIONS = pytest.mark.parametrize("direction", [0, 1])


@functools.lru_cache(maxsize=None)
def _shard(name, L, rows=True):
    from densephrases_amd import Shard
    v = S.variant(name)
    m = S.meta(L)
    s = Shard.from_faiss_index(v.ix, device=0, doc_rows=S.N_DOC_ROWS if rows else 0)
    s.set_idx2id(m.row2doc, m.row2word)
    s.set_f2o(m.doc_ids, m.f2o_off, m.f2o)
    if v.groups:
        s.set_id_groups([S.ID_OFFSET], [0, s.ntotal])
    if rows:
        s.set_codec(v.offset, v.scale)
        s.upload(S.doc_rows()[:100], 0)                       # any chunking
        s.upload(S.doc_rows()[100:], 100)
    s.finalize()
    assert s.ntotal == S.N_IDS
    return s


def _rescore(s, b):
    return s.rescore(b.direction, b.q, b.k, b.L, b.ids, b.doc, b.word, b.first, want_vecs=True)


def _rescore_dev_without_docword(s, b):
    import torch
    dev = torch.device("cuda", 0)
    n = b.n_q * b.k
    q = torch.from_numpy(np.ascontiguousarray(b.q)).to(dev)
    ids = torch.from_numpy(np.ascontiguousarray(b.ids, dtype=np.int64)).to(dev)
    first = torch.from_numpy(np.ascontiguousarray(b.first, dtype=np.float32)).to(dev)
    pred = torch.full((n,), -7, dtype=torch.int32, device=dev)
    best = torch.zeros(n, dtype=torch.float64, device=dev)
    arg = torch.full((n,), -7, dtype=torch.int32, device=dev)
    vecs = torch.full((n, 2, 768), 9.0, dtype=torch.float32, device=dev)
    s.rescore_dev(b.direction, q.data_ptr(), b.n_q, b.k, b.L, ids.data_ptr(), 0, 0, first.data_ptr(), pred.data_ptr(),
                  best.data_ptr(), arg.data_ptr(), vecs.data_ptr(), stream=torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    return pred.cpu().numpy(), best.cpu().numpy(), arg.cpu().numpy(), vecs.cpu().numpy()


def _hold(name, v, b, out):
    r = S.run_ref(v, b)
    left = check(r, *out, what=name)
    print(f"[window-doc] {name}: {len(left)} of {len(b.ids)} candidates left out")
    assert len(left) <= 0.01 * len(b.ids), (name, left)
    return r


@DIRECTIONS
@pytest.mark.parametrize("name", S.VARIANTS)
def test_doc_addressed_windows_over_raw_rows_match_the_restatement(name, direction):
    v = S.variant(name)
    np.testing.assert_array_equal(_shard(name, 10).transform(), v.A)
    for L in S.L_ALL:
        s = _shard(name, L)
        for n_q, k in S.SHAPES:
            b = S.batch(v, n_q, k, L, direction)
            out = _rescore(s, b)
            r = _hold(f"doc {name} {n_q}x{k} L{L} d{direction}", v, b, out)
            if n_q * k >= 20:
                # ids the direct map does not hold give zero vectors although their windows were read and scored
                assert (~r.is_held).sum() >= 3 and not out[3][~r.is_held].any()
                assert (r.dots[~r.is_held] != 0).any()
                assert out[3][r.is_held][:, 0].any(1).sum() >= 10 and (~r.valid).any() and r.valid.any()
                # windows that run past a document end: zero slots next to read ones
                assert L == 1 or ((r._slot_rows < 0).any(1) & (r._slot_rows >= 0).any(1)).any()


@DIRECTIONS
@pytest.mark.parametrize("name", ["house", "house_offset"])
def test_doc_addressed_windows_look_doc_and_word_up_when_none_are_passed(name, direction):
    """dph_rescore_dev(doc = NULL, word = NULL): idx2id of the local id, clipped like get_idxs -- through the id group too"""
    v = S.variant(name)
    for L in (10, 70):
        s = _shard(name, L)
        b = S.batch(v, 5, 7, L, direction, null_docword=True)
        d2, w2 = s.id2docword(b.ids)
        np.testing.assert_array_equal(d2, b.doc)
        np.testing.assert_array_equal(w2, b.word)
        out = _rescore_dev_without_docword(s, b)
        _hold(f"doc {name} NULL doc/word L{L} d{direction}", v, b, out)
        for x, y in zip(out, _rescore(s, b)):
            np.testing.assert_array_equal(x, y)


@DIRECTIONS
def test_own_vector_is_the_raw_int8_row_times_R_and_the_other_one_is_rotated_twice(direction):
    """without the restatement: vecs[c, 0] = raw int8 values (NOT de-quantised) times R, vecs[c, 1] = dequant(arg-max row) R R"""
    v = S.variant("house")
    L = 10
    b = S.batch(v, 4, 5, L, direction)
    pred, best, arg, vecs = _rescore(_shard("house", L), b)
    m = b.meta
    A64 = v.A.astype(np.float64)
    seen = 0
    for c in range(len(b.ids)):
        j = list(S.DOC_IDS).index(int(b.doc[c])) if int(b.doc[c]) in S.DOC_IDS else None
        if j is None or not (0 <= b.word[c] < S.DOC_LEN[j]) or not (0 <= b.ids[c] < S.N_IDS):
            assert not vecs[c].any()
            continue
        raw = S.doc_rows()[m.f2o_off[j] + b.word[c]].astype(np.float64)
        np.testing.assert_allclose(vecs[c, 0], raw @ A64, rtol=0, atol=1e-4)
        i = int(arg[c]) if direction == 0 else L - 1 - int(arg[c])
        ww = int(b.word[c]) + (i if direction == 0 else -i)
        if 0 <= ww < S.DOC_LEN[j]:
            deq = S.doc_rows()[m.f2o_off[j] + ww].astype(np.float64) / 20.0 - 2.0
            np.testing.assert_allclose(vecs[c, 1], deq @ A64 @ A64, rtol=0, atol=1e-4)
            seen += 1
    assert seen >= 10


@DIRECTIONS
def test_control_the_reconstruction_windows_of_a_handle_without_rows_answer_differently(direction):
    """Same index, same inputs, R != I: the handle WITHOUT rows re-scores reconstructions of ids id +- i (window_kernel<PqCodes>), the one
    with rows the dump's raw rows of word +- i -- `best` must differ, or these tests would pass on either path."""
    v = S.variant("house")
    L = 10
    b = S.batch(v, 4, 5, L, direction)
    with_rows = _rescore(_shard("house", L), b)
    without = _rescore(_shard("house", L, rows=False), b)
    ok = (b.doc >= 0) & (with_rows[1] > -9e8) & (without[1] > -9e8)
    assert ok.sum() >= 10
    assert (with_rows[1][ok] != without[1][ok]).all()
    assert np.abs(with_rows[1][ok] - without[1][ok]).min() > 1e-3
