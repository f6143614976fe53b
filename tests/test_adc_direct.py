"""The ADC scan of a PQ index called directly (csrc/dph_pq.hip: pq_pairs_kernel / pq_units_kernel, pq_adc_kernel, pq_adc_rows_kernel,
pq_segment_finish, pq_final_kernel) against the restatement of tests/_adc_ref.py, on the input sets of tests/_adc_sets.py: the best
codes of a query row are PLANTED on both sides of every place where the scan cuts the code array -- segments, chunks of four
segments, units of a group of 64 probed lists, the 1024-thread stride and its pairing, list boundaries, empty slots -- so a cut
that loses, doubles or mis-addresses one code loses a member of the top-k.  Beyond the results, what the pass leaves behind
(debug_pq_pass) is held to the restatement: the work records, the candidates appended per row, and the row's running BOUND -- the
scan's soundness argument is that it never exceeds the row's true k-th score.  Scores and bounds are compared with the tolerance
of tests/test_pq.py (kernel and oracle sum x' and the tables in float64 in different orders), nothing wider."""
import functools

import numpy as np
import pytest

from oracle import ivfpq_oracle as P
from tests import _adc_ref as R
from tests import _adc_sets as S
from tests._pq_build import _shard

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _set_shard(name):
    return _shard(S.get(name).ix)


def _search_dev(sh, x, k, nprobe):
    """dph_search_ivf_dev on device tensors -> (D, I, status) as numpy"""
    import torch
    dev = torch.device("cuda", 0)
    xd = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev)
    n = x.shape[0]
    D = torch.empty((n, k), dtype=torch.float32, device=dev)
    I = torch.empty((n, k), dtype=torch.int64, device=dev)
    st = torch.full((n,), -7, dtype=torch.int32, device=dev)
    sh.search_ivf_dev(xd.data_ptr(), n, k, nprobe, D.data_ptr(), I.data_ptr(), st.data_ptr(), stream=torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    return D.cpu().numpy(), I.cpu().numpy(), st.cpu().numpy()


def _close(a, b):
    return abs(float(a) - float(b)) <= R.RTOL * abs(float(b)) + R.ATOL


def _same_as_ref(s, rows, k, D, I):
    """the batch rows that have a restated answer: same top-k (tests/test_pq.py::_same_topk)"""
    have = [j for j, r in enumerate(rows) if r in s.ref]
    assert have
    ref = [s.ref[rows[j]].topk_padded(k) for j in have]
    R.same_topk(D[have], I[have], np.stack([d for d, _ in ref]), np.stack([i for _, i in ref]))


def _check_pass(s, sh, rows, k, may_overflow=()):
    """what the last pass -- the rows `rows` of the set's batch, k -- left in the scan's bookkeeping"""
    from tests.test_pq_hooks import _scan_workgroups
    n_q = len(rows)
    info, per_row = sh.debug_pq_pass(n_q)
    lists = R.probe_lists(s.ix, s.q[rows], s.nprobe)
    w = R.work(s.sizes, lists, s.seg)
    print(s.name, "k", k, "rows", n_q, info, "restated", vars(w))
    if s.by_rows:
        assert info["pairs"] == 0 and w.units_lo <= info["units"] <= w.units_hi, (info, vars(w))
        assert info["items_taken"] - info["units"] == _scan_workgroups(), info
    else:
        assert info["units"] == 0 and info["pairs"] == w.pairs, (info, vars(w))
        assert info["items_taken"] - info["pairs"] == _scan_workgroups(), info
    groups = (lists.shape[1] + R.PQ_GROUP - 1) // R.PQ_GROUP
    for j, r in enumerate(rows):
        appended, overflow, word = (int(v) for v in per_row[j])
        probed = int(s.sizes[lists[j]].sum())
        if j in may_overflow:
            continue
        assert overflow == 0, (s.name, k, r)
        assert min(k, probed) <= appended <= min(probed, info["cand_cap"]), (s.name, k, r, appended, probed, info["cand_cap"])
        row = s.ref.get(r)
        if row is None:
            continue
        assert row.probed == probed
        if probed < k:
            assert word == 0, (s.name, k, r, word)
            continue
        bound, kth = (float(R.pq_unkey([word])[0]) if word else None), float(row.kth(k))
        print("  row", r, "bound", bound, "k-th", kth, "appended", appended)
        if bound is not None:
            assert bound <= kth + R.RTOL * abs(kth) + R.ATOL, (s.name, k, r, bound, kth)       # a LOWER bound of the true k-th
        if s.by_rows:
            # (some group holds >= k codes as soon as the row probes k per group, and its first unit min(seg, those) of them)
            if probed >= k * groups:
                assert word != 0, (s.name, k, r)
        else:
            want = row.list_major_bound(k, s.seg)
            if want is None:
                assert word == 0, (s.name, k, r, word)
            else:
                assert bound is not None and _close(bound, want), (s.name, k, r, bound, float(want))


def _search(s, sh, rows, k):
    D, I = sh.search_ivf(s.q[rows], k, s.nprobe)
    assert sh.stats()["uncertified"] == 0
    _same_as_ref(s, rows, k, D, I)
    return D, I


# ------------------------------------------------------------------------------------------------- planted winners
@pytest.mark.parametrize("name", S.PLANTED_SETS)
def test_planted_winners_on_both_sides_of_every_cut_are_found(name):
    """Single winners: every row's top-1 is the code planted at its cut position, for k = 1 and k = 10 (the sampled-bound set: also
    k = 128, the last sampled k, and k = 129, the first exact one).  Ladder: the E planted codes of the ladder row are exactly its
    top-E.  k ascends: the scratch a shard keeps is sized by the largest k it has served, and the small k must meet the small one."""
    s, sh = S.get(name), _set_shard(name)
    assert s.by_rows == (name in S.ROW_MAJOR)
    rows = list(range(len(s.planted)))                     # the single-winner rows and the ladder row, one batch
    singles = S.chains(s)
    for k in (1, 10, 128, 129) if name == "sampled" else (1, 10):
        D, I = _search(s, sh, rows, k)
        got, want = I[[p.row for p in singles], 0], np.asarray([p.ids[0] for p in singles])
        assert (got == want).all(), (name, k, [(p.where, int(g)) for p, g in zip(singles, got) if g != p.ids[0]])
        _check_pass(s, sh, rows, k)
    lad = S.ladder(s)
    E = len(lad.ids)
    D, I = _search(s, sh, [lad.row], E)
    missing = sorted(set(lad.ids.tolist()) - set(I[0].tolist()))
    assert not missing, (name, [w for w, i in zip(lad.where, lad.ids) if int(i) in missing])
    assert len(set(I[0].tolist())) == E
    _check_pass(s, sh, [lad.row], E)


def test_list_major_pair_records_keep_row_numbers_up_to_1023_next_to_the_chunk():
    """A full pass of 1024 query rows over a list of three chunks (pair record: row | chunk << 10).  Rows 0, 511, 512 and 1023 have
    their best code in chunk 1 and their second best in chunk 2; eight other rows are compared too.  pairs = every row x every
    chunk of every list."""
    s, sh = S.get("list_major_rows"), _set_shard("list_major_rows")
    rows = list(range(1024))
    D, I = _search(s, sh, rows, 2)
    for p in s.planted:
        assert (I[p.row] == p.ids).all(), (p.row, I[p.row], p.ids)
    _check_pass(s, sh, rows, 2)
    assert sh.debug_pq_pass(1)[0]["pairs"] == 1024 * (3 + 1 + 2 + 1 + 1 + 0 + 1 + 1)


# ------------------------------------------------------------------------------------------------- M = 16, 32
@pytest.mark.parametrize("M,by_residual", [(16, True), (16, False), (32, True), (32, False)])
def test_small_m_takes_the_generic_table_kernel_and_short_code_loads(M, by_residual):
    """M = 16 / 32 (dph_index_create_pq accepts them): pq_lut_kernel<0> with 48- / 24-dimensional sub-vectors, one / two 16-byte loads
    per code.  Same top-k as the oracle, reconstruct bit for bit."""
    v = S.small_m(M, by_residual)
    sh = _shard(v.ix)
    try:
        for k, nprobe in ((10, 8), (1, 32), (100, 1)):
            D, I = sh.search_ivf(v.q, k, nprobe)
            Dr, Ir = P.search(v.ix, v.q, k, nprobe)
            R.same_topk(D, I, Dr, Ir)
            assert sh.stats()["uncertified"] == 0
        dm = P.DirectMap(v.ix.index)
        for i in (0, 17, 2999, 5999):
            np.testing.assert_array_equal(sh.reconstruct(i), P.reconstruct(v.ix, dm, i))
    finally:
        sh.close()


# ------------------------------------------------------------------------------------------------- ties
TIE_SETS = ("ties_list_major", "ties_row_major")
B9, B11, B99, B101, BLARGE, BOVER = range(6)              # the block rows of a tie set; rows 6, 7, 8 are ordinary, row 9 is all zeros
ORDINARY = [6, 7, 8]


@pytest.mark.parametrize("name", TIE_SETS)
def test_tie_blocks_straddling_k_come_back_in_id_order(name):
    """Byte-identical best codes inside one list, ids shuffled: blocks of k - 1, k + 1 and 400 (row-major: 200) for k = 10 and 100.
    Status 0, the block's scores all equal, its smallest ids in ascending order, the rest of the row as restated."""
    s, sh = S.get(name), _set_shard(name)
    for k, blocks in ((10, (B9, B11, BLARGE)), (100, (B99, B101, BLARGE))):
        rows = list(blocks) + ORDINARY
        D, I, st = _search_dev(sh, s.q[rows], k, s.nprobe)
        assert (st == 0).all(), (name, k, st)
        _same_as_ref(s, rows, k, D, I)
        for j, b in enumerate(blocks):
            ids = np.sort(s.planted[b].ids)
            m = min(k, len(ids))
            assert (D[j, :m] == D[j, 0]).all() and (m == k or D[j, m] < D[j, 0]), (name, k, b)
            np.testing.assert_array_equal(I[j, :m], ids[:m])
        _check_pass(s, sh, rows, k)


@pytest.mark.parametrize("name", TIE_SETS)
def test_a_tie_block_beyond_the_final_selections_capacity_is_reported_not_answered(name):
    """5000 identical best codes (> PQ_FINAL_CAP = 4096).  Pinned (include/dph.h): the device form gives that row status 1 and every
    other row of the batch its exact answer with status 0; the host form raises DPH_E_UNCERTIFIED and counts one uncertified row."""
    from densephrases_amd._lib import DPH_E_UNCERTIFIED, DphError
    s, sh = S.get(name), _set_shard(name)
    rows = [B9, BOVER] + ORDINARY
    D, I, st = _search_dev(sh, s.q[rows], 10, s.nprobe)
    assert st.tolist() == [0, 1, 0, 0, 0], (name, st)
    assert sh.stats()["uncertified"] == 1
    keep = [0, 2, 3, 4]
    _same_as_ref(s, [rows[j] for j in keep], 10, D[keep], I[keep])
    _check_pass(s, sh, rows, 10, may_overflow=(1,))
    with pytest.raises(DphError) as e:
        sh.search_ivf(s.q[rows], 10, s.nprobe)
    assert e.value.code == DPH_E_UNCERTIFIED, e.value
    assert sh.stats()["uncertified"] == 1


@pytest.mark.parametrize("name", TIE_SETS)
def test_an_all_zero_query_row_ties_every_probed_code_and_never_gets_a_wrong_answer(name):
    """x = 0 on an index without a bias: x' = 0, every table entry and every <x', centroid> is 0, every probed code scores 0.0.  The row
    is either answered as restated (the k smallest ids) or comes back with status 1; never status 0 with anything else.  The other
    rows of the batch are exact.  The host form raises DPH_E_UNCERTIFIED exactly when the device form reported the row."""
    from densephrases_amd._lib import DPH_E_UNCERTIFIED, DphError
    s, sh = S.get(name), _set_shard(name)
    assert s.ix.chain[0].b is None and not s.q[s.zero_row].any()
    rows = [ORDINARY[0], s.zero_row] + ORDINARY[1:]
    D, I, st = _search_dev(sh, s.q[rows], 10, s.nprobe)
    print(name, "status of the all-zero row:", int(st[1]))
    assert st[[0, 2, 3]].tolist() == [0, 0, 0] and int(st[1]) in (0, 1), (name, st)
    zD, zI = s.ref[s.zero_row].topk_padded(10)
    assert (zD == 0.0).all() and (np.diff(zI) > 0).all()
    if st[1] == 0:
        np.testing.assert_array_equal(I[1], zI)
        np.testing.assert_array_equal(D[1], zD)
    keep = [0, 2, 3]
    _same_as_ref(s, [rows[j] for j in keep], 10, D[keep], I[keep])
    _check_pass(s, sh, rows, 10, may_overflow=(1,))
    if st[1] == 0:
        Dh, Ih = sh.search_ivf(s.q[rows], 10, s.nprobe)
        np.testing.assert_array_equal(Ih[1], zI)
    else:
        with pytest.raises(DphError) as e:
            sh.search_ivf(s.q[rows], 10, s.nprobe)
        assert e.value.code == DPH_E_UNCERTIFIED, e.value
        assert sh.stats()["uncertified"] == 1
