"""The restatement of the ADC scan (tests/_adc_ref.py) and the input sets of tests/test_adc_direct.py (tests/_adc_sets.py), held
without a GPU: the restatement's top-k is the oracle's search and, on a small index, the brute force over reconstructions; its
work counts are those of a literal walk over chunks and segments; the score keys order like the scores; and every set's planted
codes are where the set claims (the builder asserts that: building a set IS the check)."""
import numpy as np
import pytest

from oracle import ivfpq_oracle as P
from tests import _adc_ref as R
from tests import _adc_sets as S
from tests._pq_build import _random_index


def test_restated_top_k_equals_the_oracles_search_and_the_brute_force_over_reconstructions():
    ix, xb, rng = _random_index(21, 1500, 8)
    q = (xb[:6] + rng.normal(0, 0.05, (6, 768))).astype(np.float32)
    for nprobe, k in ((8, 10), (3, 1), (1, 400)):
        D, I = P.search(ix, q, k, nprobe)
        rows = R.adc_rows(ix, q, nprobe)
        for r, row in enumerate(rows):
            d, i = row.topk_padded(k)
            np.testing.assert_array_equal(i, I[r])
            np.testing.assert_array_equal(d, D[r])
            assert row.probed == int(R.list_sizes(ix)[row.lists].sum()) == len(row.pos) == len(set(row.pos.tolist()))
            assert (row.kth(k) is None) == (row.probed < k) and (row.probed < k or row.kth(k) == D[r, k - 1])
    S8, J = P.brute_force(ix, P.DirectMap(ix.index), q, 10)
    for r, row in enumerate(R.adc_rows(ix, q, 8)):
        d, i = row.topk(10)
        np.testing.assert_array_equal(i, J[r])
        np.testing.assert_allclose(d, S8[r], rtol=2e-6, atol=1e-4)
    # positions: list l's codes lie at [off[l], off[l + 1]) of the code array, in list order
    off = np.concatenate([[0], np.cumsum(R.list_sizes(ix))])
    row = R.adc_rows(ix, q[:1], 8)[0]
    for l in range(8):
        sel = row.lst == l
        np.testing.assert_array_equal(row.pos[sel], np.arange(off[l], off[l + 1]))
        np.testing.assert_array_equal(row.ids[sel], np.asarray(ix.index.list_ids[l]))


def test_score_keys_order_like_the_scores_and_round_trip():
    s = np.asarray([-np.inf, -3.5, -1e-30, -0.0, 0.0, 1e-30, 2.25, 36.0, np.inf], np.float32)
    k = R.pq_key(s)
    assert (np.diff(k.astype(np.int64))[[0, 1, 2, 4, 5, 6, 7]] > 0).all() and k[3] < k[4] and (k > 0).all()
    np.testing.assert_array_equal(R.pq_unkey(k).view(np.uint32), s.view(np.uint32))


def test_work_counts_equal_a_literal_walk_over_chunks_and_segments():
    """a tiny index and a segment of 5 codes: every chunk of every (row, list) and every segment of every group written out"""
    rng = np.random.default_rng(3)
    seg = 5
    for nlist, nprobe in ((7, 7), (7, 3), (150, 150), (150, 70), (130, 65)):
        sizes = rng.choice([0, 1, 4, 5, 6, 19, 20, 21, 41], nlist)
        lists = np.stack([rng.permutation(nlist)[:nprobe] for _ in range(4)])
        pairs, units = 0, 0
        for row in lists:
            for l in row:
                for _ in range(0, int(sizes[l]), seg * R.PQ_LM_CHUNK):
                    pairs += 1
            for g0 in range(0, nprobe, R.PQ_GROUP):
                total = int(sum(sizes[l] for l in row[g0:g0 + R.PQ_GROUP]))
                for _ in range(0, total, seg):
                    units += 1
        w = R.work(sizes, lists, seg)
        assert w.pairs == pairs and w.units_lo <= units <= w.units_hi, (nlist, nprobe, w, pairs, units)
        assert (w.units_lo == w.units_hi) == (nprobe <= R.PQ_GROUP)
    # equal lists: exact whatever the grouping
    w = R.work(np.full(128, 500), np.tile(np.arange(128), (3, 1)), R.PQ_SEG)
    assert w.units_lo == w.units_hi == 3 * 2 * 3 and w.pairs == 3 * 128


def test_list_major_bound_is_the_largest_segment_k_th():
    s = S.get("list_major_128")
    row = s.ref[0]
    long_list = row.scores[row.lst == 0]
    assert len(long_list) == 8 * s.seg + 1
    for k in (1, 10):
        want = max(np.sort(row.scores[row.lst == l][a:a + s.seg])[-k] for l in range(8) for a in range(0, int(s.sizes[l]), s.seg)
                   if min(s.seg, int(s.sizes[l]) - a) >= k)
        assert row.list_major_bound(k, s.seg) == want <= row.kth(k)
    assert row.list_major_bound(1, s.seg) == row.kth(1)                   # k = 1: the best code's own segment
    assert row.list_major_bound(s.seg + 1, s.seg) is None                 # no segment holds that many: the bound word stays 0


@pytest.mark.parametrize("name", list(S.BUILDERS))
def test_every_sets_planted_codes_are_where_the_set_claims(name):
    s = S.get(name)                                                       # (asserts rank and margin of every planted code)
    assert s.by_rows == (name in S.ROW_MAJOR)
    n_planted = sum(len(p.ids) for p in s.planted)
    assert len({(l, o) for p in s.planted for l, o in p.where}) == n_planted
    for p in s.planted:
        if p.kind == "ladder":
            assert len(p.ids) <= 1024
    if name == "sampled":
        # the ladder and three single winners fill the last 1023 keys of the unit; a sample at i * floor(n / 1024) sees none of them
        n = S.SAMPLED_N
        tail = {o for p in s.planted for _, o in p.where if o >= n - 1023}
        assert tail == set(range(n - 1023, n)) and max(np.arange(1024) * (n // 1024)) < n - 1023
        assert len({int(v) for v in (np.arange(1024) * n) // 1024} & tail) > 100
    if name == "list_major_rows":
        assert [p.row for p in s.planted] == list(S.ROW_NUMBERS) and len(s.ref) == 12
        for p in s.planted:
            (l0, o0), (l1, o1) = p.where
            assert o0 // (4 * s.seg) == 1 and o1 // (4 * s.seg) == 2


def test_small_m_sets_are_searchable_by_the_oracle():
    for M in (16, 32):
        v = S.small_m(M, True)
        D, I = P.search(v.ix, v.q, 10, 8)
        assert (I >= 0).all() and v.ix.index.M == M and v.ix.index.pq_centroids.shape == (M, 256, 768 // M)
