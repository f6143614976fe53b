"""CPU: the float64 restatement of the add step (tests/_pq_encode_ref.py, sequential sums) is pinned to oracle.ivfpq_oracle.add_with_ids
(BLAS sums) -- same lists, same codes, same per-list id order, exactly -- on the four input sets, and its exempt set (near-ties below
2^-40 relative, where two float64 summation orders may disagree) stays under 0.1 % of the rows and of the cells; on these sets it is empty,
so the GPU tests (tests/test_pq_encode_gpu.py) demand equality outright."""
import numpy as np
import pytest

from tests import _pq_encode_ref as R


@pytest.mark.parametrize("i", range(len(R.SETS)))
def test_restatement_equals_the_oracle_add_with_ids(i):
    ix, trained, xb, ref = R.input_set(i)
    s = R.SETS[i]
    ivf = ix.index
    assert trained.ntotal == 0 and ix.ntotal == s["n"]
    assert (ref["lists"] >= 0).all()
    codes, ids = R.build_lists(ref["lists"], ref["codes"], np.arange(s["n"], dtype=np.int64), s["nlist"])
    for l in range(s["nlist"]):
        np.testing.assert_array_equal(ids[l], np.asarray(ivf.list_ids[l]), err_msg=f"list {l}: members / order")
        np.testing.assert_array_equal(codes[l], np.asarray(ivf.list_codes[l]), err_msg=f"list {l}: codes")


@pytest.mark.parametrize("i", range(len(R.SETS)))
def test_exempt_set_is_capped_and_empty_on_these_sets(i):
    _, _, _, ref = R.input_set(i)
    rows, cells = ref["exempt_rows"], ref["exempt_cells"]
    print(f"set {i}: exempt rows {int(rows.sum())} / {rows.size}, exempt cells {int(cells.sum())} / {cells.size}")
    assert rows.mean() <= R.EXEMPT_CAP and cells.mean() <= R.EXEMPT_CAP
    assert not rows.any() and not cells.any()


def test_the_sets_hold_the_degenerate_cases_the_gpu_tests_rely_on():
    """set 2: duplicated codewords (exact ties between cells' two best distances), duplicated centroids, empty lists; set 4: a few"""
    def tied_cells(i):
        ix, trained, xb, ref = R.input_set(i)
        ivf = trained.index
        pqc = np.asarray(ivf.pq_centroids)
        dup = np.zeros((ivf.M, 256), bool)                 # codeword j of m has an identical twin
        for m in range(ivf.M):
            _, inv, cnt = np.unique(pqc[m], axis=0, return_inverse=True, return_counts=True)
            dup[m] = cnt[inv.ravel()] > 1
        return int(dup[np.arange(ivf.M)[None, :], ref["codes"]].sum()), int((np.bincount(ref["lists"], minlength=ivf.nlist) == 0).sum())
    t2, e2 = tied_cells(1)
    t4, e4 = tied_cells(3)
    print(f"set 2: {t2} tied cells, {e2} empty lists; set 4: {t4} tied cells, {e4} empty lists")
    assert t2 > 1000 and e2 > 0 and t4 > 0 and e4 > 0


def test_non_finite_rows_get_no_list_and_zero_codes():
    _, trained, xb, ref = R.input_set(2)
    x = np.array(xb[:6])
    x[1, 5] = np.nan
    x[4, 700] = np.inf
    got = R.encode(trained, x)
    assert got["lists"][1] == -1 and got["lists"][4] == -1 and not got["codes"][[1, 4]].any()
    keep = [0, 2, 3, 5]
    np.testing.assert_array_equal(got["lists"][keep], ref["lists"][keep])
    np.testing.assert_array_equal(got["codes"][keep], ref["codes"][keep])
