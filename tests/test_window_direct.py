"""dph_rescore called directly: window_kernel<FlatRows> (flat, grouped, list-major and range-split raw-dump shards) and
window_kernel<PqCodes> + pq_unrotate_kernel (OPQ + IVFPQ shards) against the float64 restatement of tests/_window_ref.py, by its
acceptance rule: arg-max and pred_word exact wherever the restatement decides them (it must for 99 % of every input set:
tests/test_window_ref.py asserts that without a GPU), `best` within the tolerance the documented roundings allow, flat
vectors bit for bit, un-rotated PQ vectors within one fp32 rounding per product.  The input sets are tests/_window_sets.py."""
import functools

import numpy as np
import pytest

from oracle import mips_oracle as O
from tests import _window_sets as S
from tests._window_ref import check

pytestmark = pytest.mark.gpu
DIRECTIONS = pytest.mark.parametrize("direction", [0, 1])


# ------------------------------------------------------------------------------------------------- shards
def _with_meta(s, meta, lo=0, hi=None):
    hi = len(meta.row2doc) if hi is None else hi
    s.set_idx2id(meta.row2doc[lo:hi], meta.row2word[lo:hi])
    s.set_f2o(meta.doc_ids, meta.f2o_off, meta.f2o)
    return s


@functools.lru_cache(maxsize=None)
def _raw_shard(kind, L, lo=0, hi=S.N_ROWS):
    """kind: flat (rows [lo, hi) under ids ID_BASE + row) | groups (three id groups) | lists (list-major, 7 lists)"""
    from densephrases_amd import Shard
    meta = S.raw_meta(L)
    s = Shard(hi - lo, device=0, id_base=0 if kind == "groups" else S.ID_BASE + lo)
    s.upload(S.raw_rows()[lo:hi])
    _with_meta(s, meta, lo, hi)
    if kind == "groups":
        s.set_id_groups(S.GROUP_OFFSETS, S.GROUP_ROWS)
    if kind == "lists":
        import torch
        dev = torch.device("cuda", 0)
        assign = torch.from_numpy(S.list_assignment()).to(dev)
        cent = np.random.default_rng(3).normal(0, 0.5, (S.N_LISTS, 768)).astype(np.float32)
        s.make_list_major(assign.data_ptr(), cent, stream=torch.cuda.current_stream(dev).cuda_stream)
        torch.cuda.synchronize(dev)
        assert s.n_rows > S.N_ROWS and s.n_rows % 32 == 0            # every list padded to whole tiles
    s.finalize()
    assert s.ntotal == hi - lo
    return s


@functools.lru_cache(maxsize=None)
def _pq_shard(variant, groups=False):
    from densephrases_amd import Shard
    v = S.pq_variant(variant)
    s = Shard.from_faiss_index(v.ix, device=0)
    _with_meta(s, v.meta)
    if groups:
        s.set_id_groups([S.PQ_OFFSET], [0, s.ntotal])
    s.finalize()
    return s


def _rescore(s, b):
    return s.rescore(b.direction, b.q, b.k, b.L, b.ids, b.doc, b.word, b.first, want_vecs=True)


def _rescore_dev_without_docword(s, b):
    """dph_rescore_dev with doc = word = NULL: the resident idx2id is asked"""
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


def _hold(name, b, out, vec_of, held, A=None):
    """one input set against the restatement; the left-out share is capped like in tests/test_window_ref.py"""
    r = S.run_ref(b, vec_of, held, A=A)
    left = check(r, *out, what=name)
    print(f"[window] {name}: {len(left)} of {len(b.ids)} candidates left out")
    assert len(left) <= 0.01 * len(b.ids), (name, left)
    return r


# ------------------------------------------------------------------------------------------------- raw-dump shards
@DIRECTIONS
def test_flat_shard_every_shape_with_the_candidate_edges_mixed_in(direction):
    """(n_q, k) from one candidate to 640, L 1 .. 65, partial last workgroups; ids -1, around both ends of the shard and
    2^40, words and documents around every edge of the CSR, FAISS padding, (doc, word) that are not the id's, planted
    runs of identical rows (the first of them must win), saturated rows"""
    vec_of, held = S.flat_lookup()
    for (n_q, k), L in S.RAW_SHAPES:
        b = S.raw_batch(n_q, k, L, direction)
        out = _rescore(_raw_shard("flat", L), b)
        r = _hold(f"flat {n_q}x{k} L{L} d{direction}", b, out, vec_of, held)
        # vectors once more, without the restatement: the de-quantised rows bit for bit, zero outside the shard
        inside = (b.ids >= S.ID_BASE) & (b.ids < S.ID_BASE + S.N_ROWS)
        rows = np.clip(b.ids - S.ID_BASE, 0, S.N_ROWS - 1)
        np.testing.assert_array_equal(out[3][:, 0], np.where(inside[:, None], O.int8_to_float(S.raw_rows()[rows]), np.float32(0)))
        assert not out[3][~inside].any()
        if n_q * k >= 35:
            assert (~inside).any() and (~r.valid).any() and r.valid.any()


@DIRECTIONS
def test_flat_shard_gaps_of_exactly_L_are_valid_and_L_plus_one_and_negative_gaps_are_not(direction):
    vec_of, held = S.flat_lookup()
    for L in S.L_ALL:
        b = S.gap_batch(L, direction)
        _hold(f"gap L{L} d{direction}", b, _rescore(_raw_shard("flat", L), b), vec_of, held)


@DIRECTIONS
def test_flat_shard_candidates_without_a_valid_slot(direction):
    vec_of, held = S.flat_lookup()
    for L in S.L_ALL:
        b = S.invalid_batch(L, direction)
        pred, best, arg, vecs = out = _rescore(_raw_shard("flat", L), b)
        r = _hold(f"invalid L{L} d{direction}", b, out, vec_of, held)
        assert (pred == -1).all() and (best < -9e8).all()
        np.testing.assert_array_equal(arg, r.argslot)


@DIRECTIONS
def test_flat_shard_looks_doc_and_word_up_when_none_are_passed(direction):
    """dph_rescore_dev(doc = NULL, word = NULL): idx2id of the local id, clipped into the shard like get_idxs"""
    vec_of, held = S.flat_lookup()
    for (n_q, k), L in S.NULL_SHAPES:
        b = S.null_batch(n_q, k, L, direction)
        s = _raw_shard("flat", L)
        d2, w2 = s.id2docword(b.ids)
        np.testing.assert_array_equal(d2, b.doc)
        np.testing.assert_array_equal(w2, b.word)
        out = _rescore_dev_without_docword(s, b)
        _hold(f"flat NULL doc/word {n_q}x{k} L{L} d{direction}", b, out, vec_of, held)
        for x, y in zip(out, _rescore(s, b)):                       # ... and the same as with them passed
            np.testing.assert_array_equal(x, y)


@DIRECTIONS
def test_flat_shard_gives_no_vectors_for_a_candidate_it_does_not_hold(direction):
    """the candidate next to the shard: its window lies inside (the slot is read and scored), both its vectors are zero"""
    L = 10
    b = S.not_held_batch(direction, L)
    pred, best, arg, vecs = out = _rescore(_raw_shard("flat", L), b)
    r = _hold(f"not held d{direction}", b, out, *S.flat_lookup())
    assert (r.dots[:2] != 0).sum(1).min() >= L - 4                  # their windows lie in the shard and were scored
    assert not vecs[:2].any() and vecs[2].any()


@DIRECTIONS
def test_id_groups_with_64_bit_offsets_and_windows_into_the_holes(direction):
    for L in (2, 10, 33):
        b = S.group_batch(L, direction)
        out = _rescore(_raw_shard("groups", L), b)
        r = _hold(f"groups L{L} d{direction}", b, out, *S.group_lookup())
        hole = np.asarray([S.group_of(int(i)) < 0 for i in b.ids])
        assert hole.sum() >= 8 and not out[3][hole].any()
        if L > 1:
            assert ((r.vec_key == 0).any(1) & (r.vec_key != 0).any(1)).sum() >= 6        # windows half inside a group, half in a hole


@DIRECTIONS
def test_list_major_shard_equals_the_flat_shard_and_the_restatement(direction):
    vec_of, held = S.flat_lookup()
    for L in (2, 10, 33):
        b = S.list_batch(L, direction)
        out = _rescore(_raw_shard("lists", L), b)
        _hold(f"lists L{L} d{direction}", b, out, vec_of, held)
        for x, y in zip(out, _rescore(_raw_shard("flat", L), b)):
            np.testing.assert_array_equal(x, y)
        b = S.null_batch(5, 7, L, direction, S.list_batch(L, direction))
        nul = _rescore_dev_without_docword(_raw_shard("lists", L), b)
        _hold(f"lists NULL doc/word L{L} d{direction}", b, nul, vec_of, held)


@DIRECTIONS
def test_two_range_shards_each_answer_for_their_own_rows_around_the_cut(direction):
    for L in (2, 10, 33):
        b = S.cut_batch(L, direction)
        total = np.zeros((35, 2, 768), np.float32)
        for lo, hi in ((0, S.CUT), (S.CUT, S.N_ROWS)):
            out = _rescore(_raw_shard("flat", L, lo, hi), b)
            _hold(f"cut [{lo},{hi}) L{L} d{direction}", b, out, *S.flat_lookup(lo, hi))
            mine = (b.ids - S.ID_BASE >= lo) & (b.ids - S.ID_BASE < hi)
            assert mine.any() and (~mine).any() and not out[3][~mine].any()
            total += out[3]
        # summed over the shards (what the ranks of a sharded job do) every candidate's own vector is there exactly once
        np.testing.assert_array_equal(total[:, 0], O.int8_to_float(S.raw_rows()[b.ids - S.ID_BASE]))


# ------------------------------------------------------------------------------------------------- PQ shards
@DIRECTIONS
@pytest.mark.parametrize("variant,groups", [("m96", False), ("m96_bare", False), ("m48_sparse", False), ("m128_plain", False),
                                            ("m64_offset", True), ("m64_offset", False)])
def test_pq_shard_windows_of_reconstructions_and_their_unrotated_vectors(variant, groups, direction):
    """M = 96 contiguous, with its OPQ matrix and without (then the vectors are the reconstructions bit for bit) | M = 48, ids 3 i + 7, three emptied lists | M = 128, codes of the vectors themselves, a bias, a
    transform that is no rotation | M = 64, ids from 5e9 with and without an id group; L up to 70 (the position lookup serves
    64 slots at a time).  Ownership is the direct map's: a candidate the index holds gets its vectors (include/dph.h)."""
    v = S.pq_variant(variant)
    s = _pq_shard(variant, groups)
    assert s.ntotal == len(v.ids)
    np.testing.assert_array_equal(s.transform(), np.eye(768, dtype=np.float32) if v.A is None else v.A)
    look = S.pq_lookup(v)
    for L in S.PQ_L:
        for n_q, k in S.PQ_SHAPES:
            b = S.pq_batch(v, n_q, k, L, direction)
            out = _rescore(s, b)
            r = _hold(f"pq {variant}{'+groups' if groups else ''} {n_q}x{k} L{L} d{direction}", b, out, *look, A=v.A)
            if n_q * k == 35:
                assert r.is_held.sum() >= 25 and out[3][r.is_held][:, 0].any(1).all()      # what the index holds gets its own vector
                assert not out[3][~r.is_held].any()


@DIRECTIONS
def test_pq_shard_looks_doc_and_word_up_when_none_are_passed(direction):
    v = S.pq_variant("m96")
    s = _pq_shard("m96")
    for L in (10, 65):
        b = S.pq_null_batch(v, L, direction)
        d2, w2 = s.id2docword(b.ids)
        np.testing.assert_array_equal(d2, b.doc)
        np.testing.assert_array_equal(w2, b.word)
        out = _rescore_dev_without_docword(s, b)
        _hold(f"pq m96 NULL doc/word L{L} d{direction}", b, out, *S.pq_lookup(v), A=v.A)
