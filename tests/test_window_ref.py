"""The float64 restatement of the window re-score (tests/_window_ref.py) without a GPU: pinned to the oracle that the
reference's goldens pin, and run over every input set of tests/test_window_direct.py to show that it decides the arg-max
of (almost) every candidate by itself -- the share it leaves out is a condition on the inputs, not a measurement."""
import numpy as np
import pytest

from oracle import mips_oracle as O
from tests import _window_sets as S
from tests._golden import load_toy_docs
from tests._window_ref import window_ref


@pytest.mark.parametrize("direction,name", [(0, "end"), (1, "start")])
def test_restatement_equals_the_oracle_on_the_toy_dump(direction, name):
    docs = load_toy_docs()
    index = O.build_index_from_docs(docs)
    order = sorted(index.docs)
    doc_ids = np.asarray(order, np.int32)
    f2o = [np.asarray(index.docs[d].f2o_start) for d in order]
    f2o_off = np.concatenate([[0], np.cumsum([len(a) for a in f2o])])
    vec = O.int8_to_float(index.xb)
    rng = np.random.default_rng(9 + direction)
    B, k = 5, 7
    ids = rng.integers(0, index.ntotal, B * k)
    ids[:4] = 0, index.ntotal - 1, 3, index.ntotal - 4              # windows that run off both ends
    doc, word = O.get_idxs(index, ids)
    first = rng.normal(50, 5, B * k).astype(np.float32)
    q = rng.normal(0, 0.5, (B, 768)).astype(np.float32)
    for L in (1, 3, 10, 20):
        r = window_ref(lambda i: vec[i] if 0 <= i < index.ntotal else None, lambda i: 0 <= i < index.ntotal,
                       doc_ids, f2o_off, np.concatenate(f2o), q, ids, doc, word, first, k, L, direction)
        pred, best, scores, vecs, am = O.window_rescore(index, np.repeat(q, k, 0), doc, word, ids, first, L, name, branch="ram")
        np.testing.assert_array_equal(r.pred_word, pred)
        np.testing.assert_array_equal(r.argslot, am)
        np.testing.assert_array_equal(r.best, best)
        np.testing.assert_array_equal(r.scores, scores)
        np.testing.assert_array_equal(r.vecs[:, 0], vecs[:, 0] if direction == 0 else vecs[:, -1])
        np.testing.assert_array_equal(r.vecs[:, 1], vecs[np.arange(B * k), am])


def _share(sets, A=None):
    seen = 0
    for name, b, vec_of, held in sets:
        r = S.run_ref(b, vec_of, held, A=A)
        left = r.left_out()
        assert len(left) <= 0.01 * len(b.ids), f"{name}: the restatement leaves {len(left)} of {len(b.ids)} candidates undecided: {left}"
        seen += 1
        yield name, b, r
    assert seen


def test_restatement_decides_99_percent_of_every_raw_dump_input_set():
    hit_L = set()
    for name, b, r in _share(S.raw_sets()):
        if name.startswith("gap"):
            # the sets exist for the edges of valid_phrase: some arg-max must sit exactly L away, and a slot L + 1 away must be masked
            tok = b.meta.f2o[b.meta.f2o_off[2]:b.meta.f2o_off[3]].astype(np.int64)
            for c in range(28):
                s = int(r.argslot[c])
                w, ww = int(b.word[c]), int(r.slot_words[c, s])
                if r.valid[c, s] and abs(int(tok[ww]) - int(tok[w])) == b.L:
                    hit_L.add((b.L, b.direction))
        if name.startswith("invalid"):
            assert not r.valid.any() and (r.best < -9e8).all() and (r.pred_word == -1).all()
    assert hit_L == {(L, d) for L in S.L_ALL if L > 1 for d in (0, 1)}, hit_L        # (L = 1: one slot, its gap is 0)


@pytest.mark.parametrize("variant", S.PQ_VARIANTS)
def test_restatement_decides_every_candidate_of_the_pq_input_sets(variant):
    v = S.pq_variant(variant)
    late = 0
    for name, b, r in _share(S.pq_sets(variant), A=v.A):
        if b.L > 64:            # arg-max slots that only the second 64-slot position lookup of window_kernel<PqCodes> serves
            late += int((r.argslot >= 64).sum())
    assert late > 0
    if variant == "m48_sparse":
        sizes = [len(l) for l in v.ivf.list_ids]
        assert sizes[0] == sizes[4] == sizes[-1] == 0 and sum(sizes) > 700
