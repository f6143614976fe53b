"""The measurement and debug hooks of a PQ index (csrc/dph_pq.hip): the event pairs around the coarse filter's dominant launches
(profile_enable / profile_read / profile_read_each) and the bookkeeping a pass leaves behind (debug_pq_pass).  bench.py,
tools/pq_timing.py and the failure path of tests/test_fuzz_gpu.py are their only other callers.  Every expected count follows from the
launch structure (dph_launch_coarse_filter, pq_units_kernel, pq_pairs_kernel); none is a measured figure."""
import numpy as np
import pytest

from oracle import ivfpq_oracle as P
from tests.test_pq import _index_from_list_numbers, _shard


def _scan_workgroups():
    """workgroups of the ADC scan: one per CU, at most 256"""
    import torch
    return min(int(torch.cuda.get_device_properties(0).multi_processor_count), 256)


def _uniform_index(seed, nlist, n, M=96):
    rng = np.random.default_rng(seed)
    cent = rng.normal(0, 0.5, (nlist, 768)).astype(np.float32)
    lists = rng.integers(0, nlist, n)
    ix, _ = _index_from_list_numbers(rng, nlist, M, lists, cent)
    return ix, rng


@pytest.fixture(scope="module")
def long_quantizer_shard():
    """65536 lists: the smallest quantizer that reaches the filter"""
    ix, rng = _uniform_index(83, 65536, 12000)
    s = _shard(ix)
    yield s, rng
    s.close()


@pytest.mark.gpu
def test_pq_profile_brackets_every_launch_of_the_coarse_filters_dominant_kernel(long_quantizer_shard):
    """One event pair per launch of the filter's dominant kernel: the scan launches once per 128 query rows, or once for the whole
    pass when the groups run as teams (300 rows: 4 groups); the bf16x3 chain alone brackets nothing.  Every read hands the pairs back:
    a second read finds none."""
    s, rng = long_quantizer_shard
    k, nprobe = 5, 16
    q100 = rng.normal(0, 0.5, (100, 768)).astype(np.float32)
    q300 = rng.normal(0, 0.5, (300, 768)).astype(np.float32)

    def launches_then_none():
        ms, n = s.profile_read()
        assert s.profile_read() == (0.0, 0)
        assert n == 0 or ms > 0.0
        return n

    try:
        s.profile_enable(True)
        s.profile_read()                                    # (whatever an earlier user of the shard left)
        s.search_ivf(q100, k, nprobe)
        each = s.profile_read_each(0)
        assert each.shape == (1,) and each[0] > 0.0, each
        assert s.profile_read_each(0).size == 0
        s.search_ivf(q300, k, nprobe)                       # default tuning: 4 groups in ONE teams launch
        assert launches_then_none() == 1
        s.set_tuning("coarse_teams", 0)                     # one scan launch per 128 rows: 128 + 128 + 44
        s.search_ivf(q300, k, nprobe)
        assert launches_then_none() == 3
        s.set_tuning("coarse_teams", 1)
        s.set_tuning("coarse_filter", 0)                    # the bf16x3 chain alone: no filter, nothing bracketed
        s.search_ivf(q300, k, nprobe)
        assert launches_then_none() == 0
        s.set_tuning("coarse_filter", 5)
        s.profile_enable(False)
        s.search_ivf(q300, k, nprobe)
        assert launches_then_none() == 0
    finally:
        s.set_tuning("coarse_teams", 1)
        s.set_tuning("coarse_filter", 5)
        s.profile_enable(False)


@pytest.mark.gpu
def test_pq_coarse_filter_key_accepts_0_1_and_5_and_rejects_the_removed_forms():
    """Tuning key coarse_filter: 0 = the chain alone, 1 = the filter in front of it, 5 = the old spelling of 1.  The GEMM forms of the
    filter are gone and a request for 2 .. 4 fails with DPH_E_ARG and a message that names the accepted values -- as does any other value --
    instead of being served by the scan; a rejected value leaves the setting where it was (same D and I)."""
    from densephrases_amd._lib import DphError
    ix, rng = _uniform_index(87, 64, 64 * 200)
    s = _shard(ix)
    try:
        q = rng.normal(0, 0.5, (7, 768)).astype(np.float32)
        for v in (0, 1, 5):
            s.set_tuning("coarse_filter", v)
        D0, I0 = s.search_ivf(q, 10, 8)
        for v in (2, 3, 4, 6, -1):
            with pytest.raises(DphError) as e:
                s.set_tuning("coarse_filter", v)
            assert e.value.code == -1, (v, e.value)         # DPH_E_ARG
            assert all(name in str(e.value) for name in ("coarse_filter", "0 (", "1 (", "5 (")), (v, e.value)
            D, I = s.search_ivf(q, 10, 8)
            assert np.array_equal(I, I0) and np.array_equal(D, D0), v
    finally:
        s.close()


def _probed_codes(ix, q, nprobe):
    """codes in the probed lists of every query row"""
    sizes = np.asarray([len(i) for i in ix.index.list_ids], dtype=np.int64)
    lists, _ = P.coarse_probe(P.apply_chain(ix.chain, q), ix.index.centroids, nprobe)
    return sizes[lists].sum(1)


@pytest.mark.gpu
def test_pq_debug_pass_reports_the_row_major_scans_bookkeeping():
    """Many short lists (mean 187 codes): the work is grouped by query row.  nprobe = 8 is one group per row and its codes are one
    segment, so there is one unit per row that probes any code; every scan workgroup pops the queue once past its end."""
    n_q, k, nprobe = 9, 10, 8
    ix, rng = _uniform_index(85, 32, 6000)
    s = _shard(ix)
    try:
        q = rng.normal(0, 0.5, (n_q, 768)).astype(np.float32)
        s.search_ivf(q, k, nprobe)
        info, rows = s.debug_pq_pass(n_q)
        probed = _probed_codes(ix, q, nprobe)
        n_units = int((probed > 0).sum())
        assert n_units == n_q
        assert info["pairs"] == 0
        assert info["units"] == n_units
        assert info["items_taken"] - info["units"] == _scan_workgroups()
        assert info["scratch_rows"] == n_q
        assert info["unit_cap"] >= info["units"]
        assert info["cand_cap"] >= 4 * k + 64
        assert rows.shape == (n_q, 3)
        for r in range(n_q):
            appended, overflow = int(rows[r, 0]), int(rows[r, 1])
            assert overflow == 0, r
            assert k <= appended <= int(probed[r]), (r, appended, int(probed[r]))
    finally:
        s.close()


@pytest.mark.gpu
def test_pq_debug_pass_reports_the_list_major_scans_bookkeeping():
    """Few long lists (mean 2500 codes): one pair per query row and probed list -- every list is shorter than one chunk of 4 x 12288
    codes -- and no units."""
    n_q, k, nprobe = 5, 10, 2
    ix, rng = _uniform_index(87, 4, 10000)
    assert max(len(i) for i in ix.index.list_ids) < 4 * 12288 and min(len(i) for i in ix.index.list_ids) > 0
    s = _shard(ix)
    try:
        q = rng.normal(0, 0.5, (n_q, 768)).astype(np.float32)
        s.search_ivf(q, k, nprobe)
        info, _ = s.debug_pq_pass(n_q)
        assert info["units"] == 0
        assert info["pairs"] == n_q * nprobe == 10
        assert info["items_taken"] - info["pairs"] == _scan_workgroups()
    finally:
        s.close()
