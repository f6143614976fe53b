"""dph_search_bounded_dev called directly on flat shards -- plain, with outlier rows, forced to aux rows of 4 and 16 bytes, under a
non-default codec -- and held to its contract (include/dph.h) on the input sets of tests/_certificate_sets.py, whose rows press
against every term of the bound (tests/test_certificate_ref.py shows, without a GPU, that each of seven mutations of the bound is
broken by some pair of them).  Per query row:

  soundness   max over the rows of the WHOLE shard that are not in I of S64(row) <= bound.  S64 = sum_j q_j x32(n_j) in float64; nothing
              of the restated formula enters.  Tolerance: the float64 summation error of S64 alone, 768 * 2^-53 * sum_j |q_j x32(n_j)|.
  tightness   |bound - restated bound| <= tol,  tol = 4 * 768 * 2^-53 * sum |term| + 1e-9 (|b| + 1): every term of the bound is a
              reduction over at most 768 products (relative error <= 768 * 2^-53 of the sum of magnitudes, whatever the order); the
              kernel reduces per thread, per wave, over four waves and then combines the terms -- four stages whose orders differ from
              numpy's -- and adds the slack 1e-9 (|b| + 1) itself.  Where the bound handed out is a re-scored row's score (status 0)
              the summation error of that score joins.
  I           equals the restatement's; exact ties in id order; padding -1.
  D           equals fp32(S64) up to one fp32 rounding: the kernel's fixed-order float64 sum and numpy's differ by at most
              2 * 768 * 2^-53 * sum_j |q_j x32(n_j)|, far below an fp32 ulp, so the two fp32 roundings are equal or neighbours:
              tol = ulp32(|S64|) + that.  Equal rows give equal bits.
  status      equals the restatement's (0 or 2) unless |S64_k - bound| is inside tol (test_certificate_ref.py: at most 2 % of a set);
              wherever it is 0 the row is the oracle's top-k.
A second test sends the same rows through dph_search_dev (default ladder, default retry chain)."""
import functools

import numpy as np
import pytest

from oracle import mips_oracle as O
from tests import _certificate_ref as R
from tests import _certificate_sets as S

pytestmark = pytest.mark.gpu

SET_NAMES = ["e_aligned", "one_signed", "lut_default", "lut_wide_codec", "q2_filtered", "fewer_than_k", "random_130", "outlier_in_pool",
             "under_the_cut", "radix_cut", "q2_filtered_aux4", "q2_filtered_aux16"]


@functools.lru_cache(maxsize=None)
def _set(name):
    _, sets = S.build()
    s = {x.name: x for x in sets}[name]
    return s, s.certify()


@functools.lru_cache(maxsize=None)
def _oracle(name):
    s, _ = _set(name)
    return O.flat_ip_search(s.x, s.shard.xb, s.k, offset=s.shard.codec[0], factor=s.shard.codec[1])


@functools.lru_cache(maxsize=None)
def _gpu_shard(name):
    from densephrases_amd import Shard
    h = S.build()[0][name]
    s = Shard(h.xb.shape[0], device=0)
    if h.codec != S.CODEC_DEFAULT:
        s.set_codec(*h.codec)
    s.upload(h.xb)
    s.finalize()
    if h.aux:
        s.set_tuning("aux", h.aux)
    return s


def _abs_dot(s, c, rows):
    """sum_j |q_j x32(n_j)| of the given rows: what the summation error of their S64 scales with"""
    lut = np.abs(R.lut32(*s.shard.codec))
    return lut[s.shard.xb[rows].astype(np.int64) + 128] @ np.abs(c["q"]["x64"])


def _bounded(s):
    import torch
    dev = torch.device("cuda", 0)
    g = _gpu_shard(s.shard.name)
    n_q, k = s.x.shape[0], s.k
    xd = torch.from_numpy(s.x).to(dev)
    tau = torch.from_numpy(s.tau).to(dev)
    D = torch.full((n_q, k), 7.0, dtype=torch.float32, device=dev)
    I = torch.full((n_q, k), -7, dtype=torch.int64, device=dev)
    st = torch.full((n_q,), -7, dtype=torch.int32, device=dev)
    bd = torch.full((n_q,), 7.0, dtype=torch.float64, device=dev)
    g.search_bounded_dev(xd.data_ptr(), n_q, k, tau.data_ptr(), D.data_ptr(), I.data_ptr(), st.data_ptr(), bd.data_ptr(),
                         stream=torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    return g, D.cpu().numpy(), I.cpu().numpy(), st.cpu().numpy(), bd.cpu().numpy()


@pytest.mark.parametrize("name", ["plain", "codec", "outlier", "aux4", "aux16"])
def test_shard_constants_equal_their_restatement(name):
    """What finalize measures, from shard_stats / debug_mu / aux_layout alone: mu, rmax, rmax_all, the outlier count
    (= #{||n - mu||^2 >= rmax^2} <= 1024; none and rmax = rmax_all on the shards that set no row aside), the aux layout and its norm unit."""
    h = S.build()[0][name]
    g = _gpu_shard(name)
    np.testing.assert_array_equal(g.debug_mu(), h.mu)
    st = g.shard_stats()
    assert st["rmax_all"] ** 2 == pytest.approx(float(h.n2.max()), rel=1e-14)
    if name == "outlier":
        assert st["n_outliers"] == int((h.n2 >= round(st["rmax"] ** 2)).sum()) == h.outliers.size and 0 < st["n_outliers"] <= 1024
        assert st["rmax"] == h.rmax < st["rmax_all"]
    else:
        assert st["n_outliers"] == 0 and st["rmax"] == st["rmax_all"] == h.rmax_all
    lay = g.aux_layout()
    if h.aux:
        np.testing.assert_array_equal(lay, h.layout)
        assert g.debug_aux()[2]["unit"] == h.unit
    else:
        assert lay[0] == 0


@pytest.mark.parametrize("name", SET_NAMES)
def test_bounded_search_keeps_its_contract(name, capsys):
    s, ref = _set(name)
    g, D, I, st, bd = _bounded(s)
    n_rows, k = s.shard.xb.shape[0], s.k
    np.testing.assert_array_equal(g.debug_lmax(s.x.shape[0]), [c["q"]["lmax"] for c in ref])
    _, Ir, D64 = _oracle(name)
    tight, exempt = np.inf, 0
    for r, c in enumerate(ref):
        S64 = c["S64"]
        # ---- soundness over the whole shard
        ids = I[r][I[r] >= 0]
        assert len(set(ids.tolist())) == ids.size and (ids < n_rows).all()
        left = np.ones(n_rows, bool)
        left[ids] = False
        worst = int(np.argmax(np.where(left, S64, -np.inf)))
        err_worst = 768.0 * 2.0 ** -53 * float(_abs_dot(s, c, [worst])[0])
        print(f"{name} q{r}: status {st[r]} bound {bd[r]:.9g} max S64(not returned) {S64[worst]:.9g} (row {worst}) slack {bd[r] - S64[worst]:.3e}")
        assert S64[worst] <= bd[r] + err_worst, f"q{r}: row {worst} was not returned and scores {S64[worst]!r} > bound {bd[r]!r}"
        tight = min(tight, bd[r] - S64[worst])
        # ---- not looser than documented
        tol = R.bound_tol(c["terms"], c["bound_cert"])
        err_k = 2 * 768.0 * 2.0 ** -53 * float(_abs_dot(s, c, c["rescored"]).max())
        assert abs(bd[r] - c["bound"]) <= tol + (err_k if c["bound"] != c["bound_cert"] else 0.0), (r, bd[r], c["bound"], tol)
        # ---- I, D
        np.testing.assert_array_equal(I[r], c["I"], err_msg=f"q{r}")
        got = I[r] >= 0
        assert (D[r][~got] == -O.FLT_MAX).all()
        want = c["D64"][got]
        np.testing.assert_array_less(np.abs(D[r][got].astype(np.float64) - want.astype(np.float32).astype(np.float64)),
                                     np.spacing(np.abs(want).astype(np.float32)).astype(np.float64) + err_k + 1e-300, err_msg=f"q{r}")
        rows = s.shard.xb[I[r][got]]
        for j in range(1, int(got.sum())):
            if np.array_equal(rows[j], rows[j - 1]):
                assert D[r][j] == D[r][j - 1] and I[r][j] > I[r][j - 1], f"q{r}: equal rows, different bits or out of id order"
        # ---- status
        assert st[r] in (0, 2)
        if c["n_cand"] >= k and abs(c["D64"][k - 1] - c["bound_cert"]) <= tol + err_k:
            exempt += 1
        else:
            assert st[r] == c["status"], (r, st[r], c["status"], c["D64"][k - 1], c["bound_cert"])
        if st[r] == 0:
            ok, msg = O.topk_equivalent(D[r:r + 1], I[r:r + 1], D64[r:r + 1], Ir[r:r + 1])
            assert ok, (r, msg)
    assert exempt <= 0.02 * len(ref)
    with capsys.disabled():
        print(f"\n  set {name}: smallest bound - max S64(not returned) = {tight:.3e}, {exempt} status comparisons exempt")


@pytest.mark.parametrize("name", SET_NAMES)
def test_the_same_rows_through_the_default_search(name):
    """dph_search_dev on the same shards: default ladder, default retry chain.  Every row of status 0 is the oracle's top-k, and the
    planted rows come back wherever they belong to it."""
    import torch
    dev = torch.device("cuda", 0)
    s, _ = _set(name)
    g = _gpu_shard(s.shard.name)
    n_q, k = s.x.shape[0], s.k
    xd = torch.from_numpy(s.x).to(dev)
    D = torch.full((n_q, k), 7.0, dtype=torch.float32, device=dev)
    I = torch.full((n_q, k), -7, dtype=torch.int64, device=dev)
    st = torch.full((n_q,), -7, dtype=torch.int32, device=dev)
    g.search_dev(xd.data_ptr(), n_q, k, D.data_ptr(), I.data_ptr(), st.data_ptr(), stream=torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    D, I, st = D.cpu().numpy(), I.cpu().numpy(), st.cpu().numpy()
    _, Ir, D64 = _oracle(name)
    assert set(st.tolist()) <= {0, 1}
    assert (st == 0).sum() >= n_q - 1, st                  # (the chain ends in an exact scan: a row stays open only on boundary ties)
    for r in range(n_q):
        if st[r] == 0:
            ok, msg = O.topk_equivalent(D[r:r + 1], I[r:r + 1], D64[r:r + 1], Ir[r:r + 1])
            assert ok, (r, msg)
    for r, row in s.planted.items():
        pos = np.nonzero(Ir[r] == row)[0]
        if st[r] == 0 and pos.size and D64[r, pos[0]] > D64[r, k - 1] + 1e-5:
            assert row in I[r], f"q{r}: planted row {row} belongs to the top-{k} and did not come back"
