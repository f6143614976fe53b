"""dph_ivf_assign_dev / dph_index_assign_dev / dph_kmeans_step_dev (dph_assign_fused_kernel, csrc/dph_ivf.hip; csrc/dph_kmeans.hip)
against float64: the arg-max, the GAP to the runner-up and the per-list BIAS.  `gap` is the only reason the GPU list assignment equals
the float64 assignment -- the callers (densephrases_amd/ivf.py) re-check in float64 every row whose gap lies inside the fp32 error
band -- and `bias` = -||c||^2 / 2 is the L2 assignment of `train_centroids` and of the non-spherical `train_centroids_resident`.

Tolerance (derived, not measured): the callers' band, band = 4 * 1.5 * 768 * 5.97e-8 * ||x|| * max||c|| (the fp32 bound of two scores
is a third of it), plus 2 ulp_fp32(max(|s|, |bias|, |s + bias|)) for the bias add and the subtraction.

Measured on an MI355X (printed by the tests, `-s`): worst |gap - gap64| / tol = 0.72 % over all shapes, bias forms and row forms of
the assignment calls (0.55 % at 2 lists .. 0.72 % at 129), 0.56 % / 1.0 % in the non-spherical / spherical k-means step.  The
tolerance stays the derived one."""
import numpy as np
import pytest

from oracle import mips_oracle as O

BAND_REL = 4.0 * 1.5 * 768.0 * 5.97e-8

# (best, runner-up): the runner-up is a 0.999 x copy of the best list, which is the row's own vector.  dph_assign_fused_kernel keeps
# the best two per thread over the lists l with the same wave (l / 32 % 4) and lane half ((l % 32) >> 2 & 1), merges the two lane halves,
# then the four waves; a workgroup walks the 128-list tiles in order.  Both orders of each stage:
_PAIRS = [(0, 1), (9, 8),              # same wave, same lane half: one thread sees both
          (2, 6), (21, 17),            # the other lane half
          (10, 42), (75, 11),          # another wave
          (20, 148), (150, 22),        # another 128-list tile
          (50, 290), (291, 52),        # the last, partial tile (nlist = 300) against the first
          (270, 280), (285, 275)]      # both inside the partial tile
_DUP = (5, 13)                         # centroid 13 = centroid 5 = row 30's own vector: an exact tie at the top, lower id wins
_DUP_ROW = 30


def _rows(n):
    rng = np.random.default_rng(12)
    centres = rng.normal(0.0, 0.5, (40, 768)).astype(np.float32)
    x = centres[rng.integers(0, 40, n)] + rng.normal(0.0, 0.25, (n, 768)).astype(np.float32)
    return O.float_to_int8(x)


def _centroids(xb, x32, nlist):
    """centroids drawn from the rows (clustered data: many rows with a small gap), the planted pairs and the duplicate"""
    rng = np.random.default_rng(100 + nlist)
    cent = x32[rng.choice(np.arange(64, xb.shape[0]), nlist, replace=False)].copy()
    pairs = [p for p in _PAIRS if max(p) < nlist]
    if nlist == 2:
        pairs = [(1, 0)]                              # the best list comes AFTER the runner-up in the one thread that sees both
    if nlist == 129:
        pairs.append((128, 30))                       # the partial tile holds one list, and it is the best
    for i, (a, b) in enumerate(pairs):                # row i <-> pair i
        cent[a] = x32[i]
        cent[b] = x32[i] * np.float32(0.999)
    if nlist > max(_DUP):
        cent[_DUP[0]] = cent[_DUP[1]] = x32[_DUP_ROW]
    return cent, pairs


def _bias(form, cent):
    nlist = cent.shape[0]
    if form == "none":
        return None
    if form == "l2":
        return (-0.5 * (cent.astype(np.float64) ** 2).sum(1)).astype(np.float32)
    b = np.random.default_rng(nlist).normal(0.0, 3.0, nlist).astype(np.float32)
    b[nlist - 1] += np.float32(600.0)                 # the last list wins every row, whatever its score
    return b


def _reference(x32, cent, bias):
    """float64 scores -> (argmax, runner-up list, gap64, tol) per row; a duplicate of the best is the runner-up (gap 0)"""
    raw = x32.astype(np.float64) @ cent.astype(np.float64).T
    b64 = np.zeros(cent.shape[0]) if bias is None else bias.astype(np.float64)
    s = raw + b64
    best = np.argmax(s, 1)                            # first maximum: ties to the lowest list id
    rows = np.arange(len(s))
    if cent.shape[0] > 1:
        s2 = s.copy()
        s2[rows, best] = -np.inf
        second = np.argmax(s2, 1)
        gap = s[rows, best] - s[rows, second]
    else:
        second, gap = best, np.full(len(s), np.inf)
    xn = np.sqrt((x32.astype(np.float64) ** 2).sum(1))
    cmax = np.sqrt((cent.astype(np.float64) ** 2).sum(1).max())
    band = BAND_REL * xn * cmax
    mag = np.zeros(len(s))
    for l in (best, second):
        mag = np.maximum(mag, np.maximum(np.abs(raw[rows, l]), np.maximum(np.abs(b64[l]), np.abs(s[rows, l]))))
    tol = band + 2.0 * np.spacing(mag.astype(np.float32)).astype(np.float64)
    return s, best, second, gap, tol, band


def _check(best_g, gap_g, s, best, second, gap, tol, pairs, what):
    """the assertions of one kernel run over rows [0, n); returns the worst |gap - gap64| / tol"""
    n, nlist = len(best_g), s.shape[1]
    s, best, second, gap, tol = s[:n], best[:n], second[:n], gap[:n], tol[:n]
    assert ((best_g >= 0) & (best_g < nlist)).all(), what
    if nlist == 1:
        assert (best_g == 0).all() and (gap_g > 1e30).all(), (what, "one list: best 0 and a gap no band reaches (no runner-up)")
        return 0.0
    err = np.abs(gap_g.astype(np.float64) - gap)
    bad = np.nonzero(err > tol)[0]
    assert bad.size == 0, (what, f"{bad.size} gaps off, first row {int(bad[0])}: gap {float(gap_g[bad[0]])!r} float64 {float(gap[bad[0]])!r} "
                           f"tol {float(tol[bad[0]])!r}, best {int(best_g[bad[0]])} float64 {int(best[bad[0]])} / {int(second[bad[0]])}")
    clear = gap > tol
    assert (best_g[clear] == best[clear]).all(), (what, np.nonzero(clear & (best_g != best))[0][:8])
    differ = best_g != best
    assert (gap_g[differ] <= tol[differ]).all(), (what, "a row assigned differently from float64 must show a gap inside the band")
    # exact duplicates at the top: gap == 0 and the lower list id
    rows = np.arange(n)
    tie = (gap == 0.0) & (s[rows, best] - np.partition(s, nlist - 3, axis=1)[:, nlist - 3] > tol if nlist >= 3 else gap == 0.0)
    assert (gap_g[tie] == 0.0).all() and (best_g[tie] == best[tie]).all(), (what, "exact tie", np.nonzero(tie)[0][:8])
    for i, (a, b) in enumerate(pairs):
        if i < n and what[2] == "none":                # (under a bias the planted pair is one more near-tie: the general rules above)
            assert best[i] == a and second[i] == b and gap[i] > tol[i], (what, "planted pair not on top in float64", i, a, b)
            assert best_g[i] == a, (what, i, a, b, int(best_g[i]))
    return float((err / tol).max())


_NS = (1, 127, 128, 129, 20011)


@pytest.mark.gpu
@pytest.mark.parametrize("nlist", [1, 2, 127, 128, 129, 300])
def test_assign_best_gap_and_bias_equal_float64(nlist):
    """fp32 rows (dph_ivf_assign_dev) and the resident int8 rows of a shard (dph_index_assign_dev, de-quantised through the LUT), n = 1 /
    127 / 128 / 129 / 20011 rows, bias NULL / -||c||^2/2 / an arbitrary bias that makes the last list win: for every row
    |gap - gap64| <= tol; best = float64 arg-max wherever gap64 > tol; where they differ the reported gap is <= tol (what the callers'
    re-check relies on); exact duplicates give gap == 0 and the lower list id; the planted (best, 0.999 x runner-up) pairs -- one per
    merge stage of the kernel, both orders -- are found."""
    import torch
    from densephrases_amd import Shard
    from densephrases_amd.ivf import _assign_dev, dequant
    dev = torch.device("cuda", 0)
    n_all = max(_NS)
    xb = _rows(n_all)
    x32 = dequant(xb)
    cent, pairs = _centroids(xb, x32, nlist)
    shard = Shard(n_all, device=0)
    shard.upload(xb)
    xd = torch.from_numpy(x32).to(dev)
    cd = torch.from_numpy(cent).to(dev)
    worst = 0.0
    for form in ("none", "l2", "far"):
        bias = _bias(form, cent)
        ref = _reference(x32, cent, bias)
        s, best, second, gap, tol, band = ref
        if form == "far" and nlist > 1:
            assert (best == nlist - 1).all()
        if form == "none" and nlist > max(_DUP):
            assert best[_DUP_ROW] == _DUP[0] and gap[_DUP_ROW] == 0.0
            assert ((gap > 0.0) & (gap <= tol)).sum() >= 10          # near-ties inside the band are part of the data
        bd = None if bias is None else torch.from_numpy(bias).to(dev)
        for n in _NS:
            bg, gg = _assign_dev(xd[:n].contiguous(), cd, bias=bd)
            torch.cuda.synchronize()
            worst = max(worst, _check(bg.cpu().numpy(), gg.cpu().numpy(), s, best, second, gap, tol, pairs, (nlist, n, form, "fp32 rows")))
            b2 = torch.full((n,), -1, dtype=torch.int32, device=dev)
            g2 = torch.full((n,), float("nan"), dtype=torch.float32, device=dev)
            shard.assign_lists_dev(cd.data_ptr(), nlist, b2.data_ptr(), g2.data_ptr(), row0=0, n=n,
                                   bias_ptr=bd.data_ptr() if bd is not None else 0, stream=torch.cuda.current_stream(dev).cuda_stream)
            torch.cuda.synchronize()
            worst = max(worst, _check(b2.cpu().numpy().astype(np.int64), g2.cpu().numpy(), s, best, second, gap, tol, pairs,
                                      (nlist, n, form, "resident int8 rows")))
    # a window of the resident rows that does not start at row 0 nor at a multiple of 128
    if nlist > 1:
        s, best, second, gap, tol, band = _reference(x32, cent, None)
        r0, n = 1000 + 77, 300
        b2 = torch.empty(n, dtype=torch.int32, device=dev)
        g2 = torch.empty(n, dtype=torch.float32, device=dev)
        shard.assign_lists_dev(cd.data_ptr(), nlist, b2.data_ptr(), g2.data_ptr(), row0=r0, n=n, stream=torch.cuda.current_stream(dev).cuda_stream)
        torch.cuda.synchronize()
        _check(b2.cpu().numpy().astype(np.int64), g2.cpu().numpy(), s[r0:r0 + n], best[r0:r0 + n], second[r0:r0 + n], gap[r0:r0 + n],
               tol[r0:r0 + n], [], (nlist, n, "window", "resident int8 rows"))
    print(f"assign nlist {nlist}: worst |gap - gap64| / tol = {worst:.3e}")
    shard.close()


# ------------------------------------------------------------------------------------------------- D: the k-means step
@pytest.mark.gpu
@pytest.mark.parametrize("spherical", [False, True])
def test_kmeans_step_with_l2_bias_and_a_second_trip_of_the_accumulate_grid(spherical):
    """dph_kmeans_step_dev over m = 70 000 sample rows -- the accumulate kernel's grid is min(m, 65 536) workgroups, so rows 65 536 ..
    69 999 are the second trip of its grid-stride loop -- non-spherical with bias = -||c||^2 / 2 (the L2 Lloyd step of the non-spherical
    `train_centroids_resident`) and spherical without bias: the assignment is the float64 arg-min of the L2 distance (arg-max inner
    product) on every clear row (gap64 above the band), counts = bincount of the assignment, every centroid = the mean of its members
    from exact integer sums (tolerances of test_kmeans_step_on_the_device_equals_the_host_computation), empty lists untouched."""
    import torch
    from densephrases_amd import Shard
    from densephrases_amd.ivf import dequant
    dev = torch.device("cuda", 0)
    m, nlist = 70000, 37
    xb = _rows(m)
    x32 = dequant(xb)
    rng = np.random.default_rng(5)
    c0 = x32[rng.choice(m, nlist, replace=False)].copy()
    if spherical:
        c0 /= np.linalg.norm(c0, axis=1, keepdims=True)
    else:
        c0 *= rng.uniform(0.6, 1.4, (nlist, 1)).astype(np.float32)          # lengths differ: the bias matters
    c0[9] = c0[4]                                                           # list 9 stays empty (ties go to the lower id)
    bias = None if spherical else _bias("l2", c0)
    s, best, second, gap64, tol, band = _reference(x32, c0, bias)
    if not spherical:                                                       # the bias decides rows: without it the arg-max is another list
        d2 = ((x32[:400, None, :].astype(np.float64) - c0[None].astype(np.float64)) ** 2).sum(2)
        clear = gap64[:400] > tol[:400]
        np.testing.assert_array_equal(np.argmin(d2, 1)[clear], best[:400][clear])
        assert (np.argmax(x32.astype(np.float64) @ c0.astype(np.float64).T, 1) != best).mean() > 0.05
    shard = Shard(1024, device=0)                                           # the handle lends its codec and scratch; the rows are the caller's
    shard.upload(xb[:1024])
    rows = torch.from_numpy(xb).to(dev)
    c = torch.from_numpy(c0.copy()).to(dev)
    assign = torch.full((m,), -1, dtype=torch.int32, device=dev)
    gap = torch.empty(m, dtype=torch.float32, device=dev)
    counts = torch.empty(nlist, dtype=torch.int32, device=dev)
    bd = None if bias is None else torch.from_numpy(bias).to(dev)
    shard.kmeans_step_dev(rows.data_ptr(), m, c.data_ptr(), nlist, assign.data_ptr(), gap.data_ptr(), counts.data_ptr(),
                          bias_ptr=bd.data_ptr() if bd is not None else 0, spherical=spherical)
    torch.cuda.synchronize()
    got, gg = assign.cpu().numpy().astype(np.int64), gap.cpu().numpy()
    worst = _check(got, gg, s, best, second, gap64, tol, [], (nlist, m, "l2" if bias is not None else "none", "k-means step"))
    cnt = counts.cpu().numpy()
    np.testing.assert_array_equal(cnt, np.bincount(got, minlength=nlist))
    assert cnt.sum() == m and cnt[9] == 0
    newc = c.cpu().numpy()
    np.testing.assert_array_equal(newc[9], c0[9])
    for l in range(nlist):
        if cnt[l] == 0:
            continue
        mean = (xb[got == l].astype(np.int64).sum(0) / cnt[l]) / 20.0 - 2.0          # exact integer sums, then the codec
        if spherical:
            mean = mean / np.linalg.norm(mean)
        np.testing.assert_allclose(newc[l], mean, rtol=1e-6, atol=1e-7)
    print(f"k-means step spherical={spherical}: worst |gap - gap64| / tol = {worst:.3e}")
    shard.close()


@pytest.mark.gpu
def test_gather_rows_with_indices_outside_the_shard_gives_zero_rows():
    """dph_index_gather_rows_dev (dph.h): an index below 0 or >= the stored rows, among valid ones, yields an all-zero row; the valid
    indices yield their rows."""
    import torch
    from densephrases_amd import Shard
    dev = torch.device("cuda", 0)
    n = 1000
    xb = _rows(n)
    xb[xb == 0] = 1                                                         # no stored code is 0: a zero row can only be the kernel's
    s = Shard(n, device=0)
    s.upload(xb)
    idx = np.asarray([5, -1, 3, n, n + 7, -(1 << 40), 0, n - 1, 1 << 40, 999, -2, 17] + list(range(200, 260)), dtype=np.int64)
    out = torch.full((len(idx), 768), 55, dtype=torch.int8, device=dev)
    s.gather_rows_dev(torch.from_numpy(idx).to(dev).data_ptr(), len(idx), out.data_ptr())
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    valid = (idx >= 0) & (idx < n)
    assert valid.sum() == len(idx) - 6
    np.testing.assert_array_equal(got[valid], xb[idx[valid]])
    assert (got[~valid] == 0).all()
    s.close()
