"""The sharded search's own kernels called directly and held to the restatement of tests/_shard_merge_ref.py on the input sets of
tests/_shard_merge_sets.py (tests/test_shard_merge_ref.py shows, without a GPU, that the sets have teeth).  Integers and copied floats are
compared EXACTLY.

  merge      dph_merge_topk_dev and dph_merge_records_dev, dense arrays and the packed record of dist.RecordLayout (part_stride_bytes): D / I /
             src / best / pred bit for bit, outputs pre-filled with sentinels.  Ids within a row are unique -- duplicate ids are undefined
             input for the kernel (two candidates would claim one rank) and are not tested.
  verdict    status_out of dph_merge_records_dev over the table of verdict_sets(), with bound_parts and with NULL.  No bound sits closer to
             the restated kth = D_k - |D_k| 1.2e-7 than 2^-40 relative: the device compiler may contract that multiply-subtract to an FMA,
             which moves kth by at most an ulp (2^-52 relative) -- 4096 ulps clear of every case, and far inside an fp32 ulp.  (Exempt: kth
             = 0 and kth = -1e300, which involve no rounding at all and meet equal bounds on purpose.)
  union      dph_union_bounds_dev for 1 .. 64 parts.
  sample     dph_search_sample_dev on flat shards uploaded as they are, under explicit and derived ladders, 1 .. 300 query rows: `top` as a
             sorted multiset; the closed form for nesting ladders; union_bound(own top, 1) = the shard's own bound.
  protocol   sample -> union -> bounded -> dph_merge_records_dev with bound_parts over 2, 3 and 5 range shards of one dump on one device."""
import functools

import numpy as np
import pytest

from oracle import mips_oracle as O
from tests import _shard_merge_ref as M
from tests import _shard_merge_sets as S

pytestmark = pytest.mark.gpu


def _dev():
    import torch
    return torch.device("cuda", 0)


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _stream():
    import torch
    return torch.cuda.current_stream(_dev()).cuda_stream


def _grid():
    """scan workgroups of this device (csrc/dph_scan.hip, dph_scan_grid): one per CU, at most 256"""
    import torch
    return min(torch.cuda.get_device_properties(0).multi_processor_count, 256)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


# ---------------------------------------------------------------------------------------------------------------- merge
def _merge_inputs(c, P, n, k, packed):
    """device tensors of the six fields [P, ...] and the part stride: dense per-field arrays, or views into one packed buffer"""
    import torch
    from densephrases_amd.dist import RecordLayout
    names = ("D", "I", "best", "pred", "status", "bound")
    if not packed:
        return {f: _t(c[f]) if c[f].size else torch.zeros(8, dtype=_t(c[f]).dtype, device=_dev()) for f in names}, 0
    lay = RecordLayout(n, k)
    buf = torch.full((P, max(lay.nbytes, 8)), 0x5A, dtype=torch.uint8, device=_dev())
    v = lay.views(buf[:, :lay.nbytes]) if lay.nbytes else None
    if v is None:
        return {f: buf for f in names}, 8
    for f in names:
        v[f].copy_(_t(c[f]))
    assert all(v[f].data_ptr() % 8 == 0 for f in names) and lay.nbytes % 8 == 0
    v["_buf"] = buf
    return v, lay.nbytes


def _merge_outputs(n, k):
    import torch
    dev, m = _dev(), max(n, 1)
    return {"D": torch.full((m, k), 7.0, dtype=torch.float32, device=dev), "I": torch.full((m, k), -7, dtype=torch.int64, device=dev),
            "src": torch.full((m, k), -7, dtype=torch.int32, device=dev), "best": torch.full((m, k), 7.0, dtype=torch.float64, device=dev),
            "pred": torch.full((m, k), -7, dtype=torch.int32, device=dev), "status": torch.full((m,), -7, dtype=torch.int32, device=dev)}


@pytest.mark.parametrize("packed", [False, True], ids=["dense", "packed"])
@pytest.mark.parametrize("P,n,k", S.MERGE_SHAPES + [(3, 0, 4)])
def test_merge_equals_its_restatement_bit_for_bit(P, n, k, packed):
    import torch
    from densephrases_amd import _lib
    c = S.merge_case(P, n, k)
    want = M.merge(c["D"], c["I"], k, c["best"], c["pred"])
    want_status = M.merged_status(want["D"][:, k - 1], want["nvalid"], k, c["status"], c["bound"])
    v, stride = _merge_inputs(c, P, n, k, packed)
    # ---- dph_merge_topk_dev
    o = _merge_outputs(n, k)
    _lib.merge_topk_dev(0, v["D"].data_ptr(), v["I"].data_ptr(), P, n, k, o["D"].data_ptr(), o["I"].data_ptr(), src_ptr=o["src"].data_ptr(),
                        stream=_stream(), part_stride_bytes=stride)
    torch.cuda.synchronize()
    for f in ("D", "I", "src"):
        np.testing.assert_array_equal(_bits(o[f].cpu().numpy()[:n]), _bits(want[f]), err_msg=f"topk {f}")
    assert (o["best"] == 7.0).all() and (o["status"] == -7).all()
    # ---- dph_merge_records_dev
    o = _merge_outputs(n, k)
    _lib.merge_records_dev(0, v["D"].data_ptr(), v["I"].data_ptr(), v["best"].data_ptr(), v["pred"].data_ptr(), v["status"].data_ptr(), P, n, k,
                           o["D"].data_ptr(), o["I"].data_ptr(), o["best"].data_ptr(), o["pred"].data_ptr(), o["status"].data_ptr(),
                           stream=_stream(), part_stride_bytes=stride, bound_ptr=v["bound"].data_ptr())
    torch.cuda.synchronize()
    for f in ("D", "I", "best", "pred"):
        np.testing.assert_array_equal(_bits(o[f].cpu().numpy()[:n]), _bits(want[f]), err_msg=f"records {f}")
    np.testing.assert_array_equal(o["status"].cpu().numpy()[:n], want_status)
    if n == 0:
        assert (o["D"] == 7.0).all() and (o["status"] == -7).all()       # nothing to merge: nothing is written


# ---------------------------------------------------------------------------------------------------------------- merge verdict
@pytest.mark.parametrize("bounds", [True, False], ids=["bounds", "null"])
@pytest.mark.parametrize("name", list(S.KTH_SCORES) + ["kth_zero", "rounds_up"])
def test_merge_verdict_equals_its_restatement(name, bounds):
    import torch
    from densephrases_amd import _lib
    s = S.verdict_sets()[name]
    P, k, n = S.VERDICT_P, s.k, s.kth.size
    # the inputs keep their distance from the restated kth (see the module docstring)
    kth = s.kth[None, :]
    exact = (kth == 0.0) | (kth == M.NO_KTH)
    assert (((s.bound == kth) & exact) | (np.abs(s.bound - kth) >= np.abs(kth) * 2.0 ** -41)).all()
    want = s.verdict(bounds=bounds)
    o = _merge_outputs(n, k)
    best, pred = _t(np.zeros((P, n, k))), _t(np.zeros((P, n, k), np.int32))
    D, I, st, bd = _t(s.D), _t(s.I), _t(s.status), _t(s.bound)
    _lib.merge_records_dev(0, D.data_ptr(), I.data_ptr(), best.data_ptr(), pred.data_ptr(), st.data_ptr(), P, n, k, o["D"].data_ptr(),
                           o["I"].data_ptr(), o["best"].data_ptr(), o["pred"].data_ptr(), o["status"].data_ptr(), stream=_stream(),
                           part_stride_bytes=0, bound_ptr=bd.data_ptr() if bounds else 0)
    torch.cuda.synchronize()
    got = o["status"].cpu().numpy()
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, [(int(r), int(got[r]), int(want[r]), s.status[:, r].tolist(), s.bound[:, r].tolist(), s.kth[r], s.row_info[r]) for r in bad[:5]]
    np.testing.assert_array_equal(_bits(o["D"].cpu().numpy()), _bits(s.merged["D"]))
    np.testing.assert_array_equal(o["I"].cpu().numpy(), s.merged["I"])


# ---------------------------------------------------------------------------------------------------------------- union bound
@pytest.mark.parametrize("n", S.UNION_ROWS)
@pytest.mark.parametrize("P", S.UNION_PARTS)
def test_union_bound_equals_its_restatement(P, n):
    import torch
    from densephrases_amd import _lib
    top, _ = S.union_case(P, n)
    td = _t(top)
    tau = torch.full((n,), 12345, dtype=torch.int32, device=_dev())
    _lib.union_bounds_dev(0, td.data_ptr(), P, n, tau.data_ptr(), _stream())
    torch.cuda.synchronize()
    np.testing.assert_array_equal(tau.cpu().numpy().astype(np.int64), M.union_bounds(top))


# ---------------------------------------------------------------------------------------------------------------- sample
@functools.lru_cache(maxsize=None)
def _gpu_sample_shard(name):
    from densephrases_amd import Shard
    h = S.sample_shards()[name]
    g = Shard(h.xb.shape[0], device=0)
    g.upload(h.xb)
    g.finalize()
    st = g.shard_stats()
    assert g.aux_layout()[0] == 0 and st["n_outliers"] == h.shard.outliers.size and st["rmax"] == h.shard.rmax
    np.testing.assert_array_equal(g.debug_mu(), h.shard.mu)
    return g


@pytest.mark.parametrize("name,explicit,n_q", S.SAMPLE_CASES, ids=[f"{a}-{'x'.join(map(str, b)) or 'default'}-{c}" for a, b, c in S.SAMPLE_CASES])
def test_sample_equals_the_restated_ladder(name, explicit, n_q):
    import torch
    from densephrases_amd import _lib
    h = S.sample_shards()[name]
    g = _gpu_sample_shard(name)
    g.set_tuning("ladder", *explicit)                       # (no value: the derived default)
    want, log = h.sample(n_q, _grid(), explicit)
    xd = _t(h.x[:n_q])
    top = torch.full((n_q, 16), 777, dtype=torch.int32, device=_dev())
    try:
        g.search_sample_dev(xd.data_ptr(), n_q, top.data_ptr(), _stream())
        torch.cuda.synchronize()
    finally:
        g.set_tuning("ladder")
    got = np.sort(top.cpu().numpy().astype(np.int64), axis=1)[:, ::-1]
    np.testing.assert_array_equal(g.debug_lmax(n_q), h.keys()[2][:n_q])
    bad = np.nonzero((got != want).any(1))[0]
    assert bad.size == 0, [(int(r), got[r].tolist(), want[r].tolist()) for r in bad[:3]]
    # nesting ladders: the 16 best non-outlier keys of the tiles the last level visits -- nothing of the restated kp enters
    key = h.keys()[0]
    for q0, nq, strides, _, _ in log:
        if strides and M.nests(strides):
            np.testing.assert_array_equal(got[q0:q0 + nq], M.sample_top_closed_form(key[q0:q0 + nq], h.shard.outliers, strides[-1]))
        if not strides:
            assert (got[q0:q0 + nq] == M.INT_MIN).all()
    # the shard's own bound: union_bound(own top, 1) = (16-th of own top) - 1
    tau = torch.full((n_q,), 12345, dtype=torch.int32, device=_dev())
    _lib.union_bounds_dev(0, top.data_ptr(), 1, n_q, tau.data_ptr(), _stream())
    torch.cuda.synchronize()
    own = np.where(got[:, 15] == M.INT_MIN, M.INT_MIN, got[:, 15] - 1)
    np.testing.assert_array_equal(tau.cpu().numpy().astype(np.int64), own)
    np.testing.assert_array_equal(own, M.union_bounds(want[None]))


# ---------------------------------------------------------------------------------------------------------------- the whole protocol
@functools.lru_cache(maxsize=None)
def _gpu_range_shard(lo, hi):
    from densephrases_amd import Shard
    g = Shard(hi - lo, device=0, id_base=lo)
    g.upload(S.dump().xb[lo:hi])
    g.finalize()
    assert g.aux_layout()[0] == 0
    return g


@pytest.mark.parametrize("name,P,k", S.PROTOCOL_SETS)
def test_protocol_through_the_raw_entry_points(name, P, k, capsys):
    import torch
    from densephrases_amd import _lib
    from densephrases_amd.dist import RecordLayout
    d = S.dump()
    run = d.run(P, k, _grid())
    cuts, n, dev = S.CUTS[P], d.x.shape[0], _dev()
    shards = [_gpu_range_shard(cuts[p], cuts[p + 1]) for p in range(P)]
    for g, h in zip(shards, d.shards(P)):
        assert g.shard_stats()["n_outliers"] == h.outliers.size
    fin = np.nonzero(~run["nonfinite"])[0]
    xd = _t(d.x)
    st = _stream()
    # phase 1 and the union bound
    top = torch.full((P, n, 16), 777, dtype=torch.int32, device=dev)
    for p, g in enumerate(shards):
        g.search_sample_dev(xd.data_ptr(), n, top[p].data_ptr(), st)
    tau = torch.full((n,), 12345, dtype=torch.int32, device=dev)
    _lib.union_bounds_dev(0, top.data_ptr(), P, n, tau.data_ptr(), st)
    # phase 2 into one packed record per shard, then the merge with the shards' bounds
    lay = RecordLayout(n, k)
    buf = torch.zeros((P, lay.nbytes), dtype=torch.uint8, device=dev)
    v = lay.views(buf)
    v["D"].fill_(7.0), v["I"].fill_(-7), v["status"].fill_(-7), v["bound"].fill_(7.0)
    v["best"].copy_(_t(np.arange(P * n * k, dtype=np.float64).reshape(P, n, k)))
    v["pred"].copy_(_t(np.arange(P * n * k, dtype=np.int32).reshape(P, n, k)))
    for p, g in enumerate(shards):
        g.search_bounded_dev(xd.data_ptr(), n, k, tau.data_ptr(), v["D"][p].data_ptr(), v["I"][p].data_ptr(), v["status"][p].data_ptr(),
                             v["bound"][p].data_ptr(), st)
    o = {"D": torch.full((n, k), 7.0, dtype=torch.float32, device=dev), "I": torch.full((n, k), -7, dtype=torch.int64, device=dev),
         "best": torch.full((n, k), 7.0, dtype=torch.float64, device=dev), "pred": torch.full((n, k), -7, dtype=torch.int32, device=dev),
         "status": torch.full((n,), -7, dtype=torch.int32, device=dev)}
    _lib.merge_records_dev(0, v["D"].data_ptr(), v["I"].data_ptr(), v["best"].data_ptr(), v["pred"].data_ptr(), v["status"].data_ptr(), P, n, k,
                           o["D"].data_ptr(), o["I"].data_ptr(), o["best"].data_ptr(), o["pred"].data_ptr(), o["status"].data_ptr(),
                           stream=st, part_stride_bytes=lay.nbytes, bound_ptr=v["bound"].data_ptr())
    torch.cuda.synchronize()
    top, tau = top.cpu().numpy().astype(np.int64), tau.cpu().numpy().astype(np.int64)
    parts = {f: v[f].cpu().numpy() for f in ("D", "I", "status", "bound", "best", "pred")}
    got = {f: t.cpu().numpy() for f, t in o.items()}
    # ---- the integers of phases 1 and 2 (finite rows)
    np.testing.assert_array_equal(np.sort(top, axis=2)[:, fin, ::-1], run["top"][:, fin])
    np.testing.assert_array_equal(tau[fin], run["tau"][fin])
    # ---- the merge is the merge of what the shards returned, verdict included
    m = M.merge(parts["D"], parts["I"], k, parts["best"], parts["pred"])
    for f in ("D", "I", "best", "pred"):
        np.testing.assert_array_equal(_bits(got[f]), _bits(m[f]), err_msg=f)
    np.testing.assert_array_equal(got["status"], M.merged_status(m["D"][:, k - 1], m["nvalid"], k, parts["status"], parts["bound"]))
    # ---- the contract
    ex = M.status_exemptions(run, k)
    assert ex.sum() <= 0.02 * n
    used = []
    for r in range(n):
        if ex[r]:
            used.append(r)
            continue
        assert (parts["status"][:, r] == run["status_parts"][:, r]).all(), (name, r, parts["status"][:, r], run["status_parts"][:, r])
        assert got["status"][r] == run["status"][r], (name, r, got["status"][r], run["status"][r])
    nf = S.Q_NONFINITE
    assert got["status"][nf] == 3 and (got["I"][nf] == -1).all() and (got["D"][nf] == -O.FLT_MAX).all() and (parts["status"][:, nf] == 3).all()
    _, Ir, D64 = O.flat_ip_search(d.x[fin], d.xb, k)
    for j, r in enumerate(fin):
        if got["status"][r] == 0:
            np.testing.assert_array_equal(got["I"][r], Ir[j], err_msg=f"{name} q{r}")
            ok, msg = O.topk_equivalent(got["D"][r:r + 1], got["I"][r:r + 1], D64[j:j + 1], Ir[j:j + 1])
            assert ok, (name, r, msg)
    if k > 16:                                              # reported, never answered: exactly the rows the restatement leaves open
        np.testing.assert_array_equal(np.nonzero(got["status"] == 1)[0], np.nonzero(run["status"] == 1)[0])
        assert (got["status"] == 1).sum() >= 1
    else:
        assert (got["status"][fin] == 0).all()
    with capsys.disabled():
        print(f"\n  {name}: status {got['status'].tolist()}, {len(used)} status comparisons exempt {used}")
