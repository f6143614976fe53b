"""The train step of the reference's index on the GPU: ``index.train`` behind
IndexPreTransform(OPQMatrix(768, M), IndexIVFPQ(IndexFlatIP, 768, nlist, M, 8, METRIC_INNER_PRODUCT)) (the reference's
build_phrase_index.py:96-142, fed by sample_data, :60-93).  Input: the dump's rows; output: an EMPTY, trained index
(densephrases_amd.faiss_io.PreTransformIndex) that ``faiss_io.write_index`` stores as ``trained.faiss`` and ``pq_build.add_with_ids_resident`` /
``MIPS(pq={"trained": ...})`` fill.  DESIGN.md section 5.9.

  1. sample      the coarse trainer's size rule (ivf.kmeans_sample_size); the OPQ / PQ training set is a seeded random subset of at most
                 65 536 (FAISS: 256 points per codeword x 256 codewords) of those rows, de-quantised through the exact table ivf._lut_dev
  2. OPQ         FAISS' OPQMatrix.train on the raw vectors of the set (no centring, no bias): A_0 a seeded random orthonormal matrix; per
                 iteration x' = fp32(x A^T) (float64, one rounding), Lloyd steps of the M sub-space quantisers hot-started from the previous
                 codebooks (dph_pq_train_step_dev; the first iteration starts from 256 seeded distinct training points per sub-space), decode,
                 C = Y^T X in float64 on the device, U S V^T = svd(C) in numpy float64 on the host, A = fp32(U V^T)
  3. centroids   ``centroids=`` as given (they ARE the quantizer's vectors, in the rotated space), or ivf.train_centroids_resident over the
                 int8 rows followed by c' = fp32(c A^T).  FAISS clusters x' itself; for an orthogonal A the two are equal in exact arithmetic
                 (inner products, norms and means commute with a rotation) -- the deviation of this trainer
  4. residual PQ x' of the set, list by dph_ivf_assign_dev, r = fp32(x' - c'[list]), ``final_pq_iters`` Lloyd steps from a seeded start
  5. empty codewords after every step: the rule of ivf.split_empty_lists per sub-space (``split_empty_codewords``)

Determinism: every Lloyd step is a pure function of its inputs (float64 sums in ascending row order, csrc/dph_pq_train.hip), the seeds are
drawn on the host from ``numpy.random.default_rng(seed)``: two runs on one machine give the same bytes."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import _lib

OPQ_SET_ROWS = 256 * 256            # FAISS: OPQMatrix.max_train_points = 256 * 256, ProductQuantizer's ClusteringParameters 256 points per codeword
KSUB = 256


def random_orthonormal(d: int, rng) -> np.ndarray:
    """a seeded random rotation: Q of a QR factorisation, signs fixed by the diagonal of R, fp32"""
    q, r = np.linalg.qr(rng.normal(size=(d, d)))
    return (q * np.sign(np.diag(r))[None, :]).astype(np.float32)


def draw_seeds(seed: int, n_set: int, M: int) -> dict:
    """everything random of a training run over a set of ``n_set`` rows, drawn on the host: A_0 [768,768] fp32 and, per sub-space, the 256
    distinct rows of the set the OPQ codebooks (``init_opq`` int64 [M,256]) and the residual codebooks (``init_pq``) start from"""
    if n_set < KSUB:
        raise ValueError(f"PQ training: {n_set} training rows for {KSUB} codewords per sub-space")
    rng = np.random.default_rng(seed)
    A0 = random_orthonormal(_lib.DIM, rng)
    init_opq = np.stack([rng.choice(n_set, KSUB, replace=False) for _ in range(M)]).astype(np.int64)
    init_pq = np.stack([rng.choice(n_set, KSUB, replace=False) for _ in range(M)]).astype(np.int64)
    return {"A0": A0, "init_opq": init_opq, "init_pq": init_pq}


def split_empty_codewords(pqc, counts, eps: float = 1.0 / 1024.0) -> int:
    """ivf.split_empty_lists for every sub-space at once: pqc [M,256,dsub] fp32 and counts [M,256] are torch tensors on one device, pqc is
    modified in place.  Inside a sub-space the k-th empty codeword (ascending j) takes the k-th largest codeword (a STABLE order: ties to
    the lowest j) as long as that one has more than one member; the two copies are perturbed by -+eps on alternating components.  Returns
    the number of codewords split."""
    import torch
    empty = counts == 0
    if not bool(empty.any()):
        return 0
    cnt = counts.to(torch.int64)
    order = torch.argsort(cnt, dim=1, descending=True, stable=True)                 # [M,256] donors, largest first
    rank = torch.cumsum(empty.to(torch.int64), dim=1) - 1                           # k of the k-th empty codeword
    donor = torch.gather(order, 1, rank.clamp_min(0))
    ok = empty & (torch.gather(cnt, 1, donor) > 1)
    m_idx, j_idx = torch.nonzero(ok, as_tuple=True)
    if m_idx.numel() == 0:
        return 0
    d_idx = donor[m_idx, j_idx]
    sign = torch.ones(pqc.shape[2], dtype=pqc.dtype, device=pqc.device)
    sign[1::2] = -1.0
    base = pqc[m_idx, d_idx].clone()
    pqc[m_idx, j_idx] = base * (1.0 + eps * sign)
    pqc[m_idx, d_idx] = base * (1.0 - eps * sign)
    return int(m_idx.numel())


def train_step_dev(x, pqc, update: bool = True, want_err: bool = True):
    """one dph_pq_train_step_dev over torch tensors on one GPU: x [n,768] fp32, pqc [M,256,dsub] fp32 (replaced in place when ``update``)
    -> (codes uint8 [n,M], counts int32 [M,256], row_err float64 [n] or None), all under the INPUT codebooks"""
    import torch
    n, M = int(x.shape[0]), int(pqc.shape[0])
    if not (x.is_contiguous() and pqc.is_contiguous() and x.dtype == torch.float32 and pqc.dtype == torch.float32):
        raise ValueError("train_step_dev: contiguous fp32 tensors")
    dev = x.device
    codes = torch.empty((n, M), dtype=torch.uint8, device=dev)
    counts = torch.empty((M, KSUB), dtype=torch.int32, device=dev)
    err = torch.empty(n, dtype=torch.float64, device=dev) if want_err else None
    vp = C.c_void_p
    _lib._chk(_lib.lib.dph_pq_train_step_dev(dev.index, vp(x.data_ptr()), n, M, vp(pqc.data_ptr()), vp(codes.data_ptr()), vp(counts.data_ptr()),
                                             vp(err.data_ptr()) if want_err else None, 1 if update else 0,
                                             vp(torch.cuda.current_stream(dev).cuda_stream)))
    return codes, counts, err


def decode_dev(codes, pqc):
    """y [n,768] fp32 = concat_m pqc[m][codes[:, m]] (dph_pq_decode_dev)"""
    import torch
    n, M = int(codes.shape[0]), int(pqc.shape[0])
    y = torch.empty((n, _lib.DIM), dtype=torch.float32, device=codes.device)
    vp = C.c_void_p
    _lib._chk(_lib.lib.dph_pq_decode_dev(codes.device.index, vp(codes.data_ptr()), n, M, vp(pqc.data_ptr()), vp(y.data_ptr()),
                                         vp(torch.cuda.current_stream(codes.device).cuda_stream)))
    return y


def rotate_dev(x, A):
    """x' = fp32(x A^T): float64 accumulation, one rounding (torch tensors on one device, A [768,768] fp32)"""
    import torch
    return (x.to(torch.float64) @ A.to(torch.float64).T).to(torch.float32).contiguous()


def init_codebooks_dev(x, init):
    """pqc [M,256,dsub]: sub-space m starts from the slices of rows init[m] (int64 [M,256], torch or numpy)"""
    import torch
    M = int(init.shape[0])
    dsub = _lib.DIM // M
    idx = torch.as_tensor(init, device=x.device).to(torch.int64)
    xs = x.reshape(x.shape[0], M, dsub)
    return torch.stack([xs[idx[m], m] for m in range(M)]).contiguous()


def lloyd_dev(x, pqc, steps: int):
    """``steps`` Lloyd steps in place, empty codewords split after each; then the assignment under the codebooks as they stand.
    -> (codes, mean row error of that assignment, [mean row error under the codebooks every step started from], codewords split)"""
    errs, splits = [], 0
    for _ in range(int(steps)):
        _, counts, err = train_step_dev(x, pqc, update=True)
        errs.append(float(err.sum()) / x.shape[0])
        splits += split_empty_codewords(pqc, counts)
    codes, _, err = train_step_dev(x, pqc, update=False)
    return codes, float(err.sum()) / x.shape[0], errs, splits


def opq_iteration_dev(x, A, pqc, steps: int):
    """one iteration of the OPQ alternation over the raw set x [n,768] (device): rotate by A, ``steps`` Lloyd steps on pqc (in place),
    decode, Procrustes.  -> dict(xp, codes, err (mean row error behind the Lloyd steps), C float64 [768,768] (device), A_new fp32 numpy)"""
    import torch
    xp = rotate_dev(x, A)
    codes, err, _, splits = lloyd_dev(xp, pqc, steps)
    y = decode_dev(codes, pqc)
    Cm = y.to(torch.float64).T @ x.to(torch.float64)
    U, _, Vt = np.linalg.svd(Cm.cpu().numpy())
    return {"xp": xp, "codes": codes, "err": err, "C": Cm, "A_new": (U @ Vt).astype(np.float32), "splits": splits}


def _pick_rows(n: int, m: int, seed: int, dev):
    """m of n row numbers, ascending, without replacement (the draw of ivf.train_centroids_resident)"""
    import torch
    if m >= n:
        return torch.arange(n, dtype=torch.int64, device=dev)
    g = torch.Generator(device=dev).manual_seed(int(seed))
    if n <= (1 << 28):
        return torch.randperm(n, generator=g, device=dev)[:m].sort().values
    step = n / m
    return (torch.arange(m, dtype=torch.float64, device=dev) * step
            + torch.rand(m, generator=g, device=dev, dtype=torch.float64) * step).to(torch.int64).clamp_(max=n - 1)


def train_index_resident(rows, nlist: int, M: int = 96, opq_iters: int = 10, pq_iters_first: int = 40, pq_iters: int = 4,
                         final_pq_iters: int = 25, train_rows: Optional[int] = None, centroids=None, seed: int = 0, device: int = 0,
                         return_info: bool = False, offset: float = -2.0, scale: float = 20.0, coarse_iters: int = 10):
    """``rows``: a resident FLAT ``Shard`` (int8 rows of the dump's codec ``offset`` / ``scale``) or fp32 [n,768] (numpy / torch).  Returns the
    trained, empty index: ``is_trained``, ntotal 0, by_residual, nprobe 1, direct-map type 2 (module docstring for the stages; the defaults
    are FAISS': OPQMatrix.niter 10 as the reference sets it, niter_pq_0 40, niter_pq 4, ProductQuantizer niter 25).  ``centroids``
    [nlist,768] are taken as the coarse quantizer's vectors as they are (rotated space); without them the coarse k-means runs over the
    int8 rows of the shard (``coarse_iters`` iterations) and its centroids are rotated, c' = fp32(c A^T) -- FAISS clusters the rotated
    vectors, which is the same in exact arithmetic for an orthogonal A.  fp32 rows need ``centroids``.  With ``return_info`` also a dict: set size, per-iteration OPQ
    error, per-step residual-PQ error, final error, codewords split, seconds per stage.  A row with a NaN / Inf element raises ValueError."""
    import time
    import torch
    from . import faiss_io
    from .ivf import _dequant_dev, _lut_dev, kmeans_sample_size, train_centroids_resident
    dev = torch.device("cuda", int(device))
    torch.cuda.set_device(dev)
    D = _lib.DIM
    nlist, M = int(nlist), int(M)
    if M <= 0 or D % M or M % 16 or M > 128:
        raise ValueError("train_index_resident: M must be a multiple of 16 that divides 768, M <= 128")
    flat = rows if isinstance(rows, _lib.Shard) else None
    if flat is not None:
        if getattr(flat, "pq", None) is not None or flat.device != int(device):
            raise ValueError("train_index_resident: `rows` must be a flat int8 shard on the same device")
        n = flat.n_rows
    else:
        if not isinstance(rows, torch.Tensor):
            rows = np.asarray(rows)
        if rows.ndim != 2 or rows.shape[1] != D or str(rows.dtype).split(".")[-1] != "float32":
            raise ValueError("train_index_resident: rows must be fp32 [n, 768]")
        n = int(rows.shape[0])
        if centroids is None:
            raise ValueError("train_index_resident: fp32 rows need `centroids` (the coarse k-means runs over a resident int8 shard)")
    if centroids is not None:
        centroids = np.array(centroids, dtype=np.float32, order="C")                # (a copy: torch wants a writable array)
        if centroids.shape != (nlist, D):
            raise ValueError(f"train_index_resident: centroids must be [{nlist}, {D}]")
    secs = {}
    t0 = time.perf_counter()

    def lap(name):
        nonlocal t0
        torch.cuda.synchronize(dev)
        t1 = time.perf_counter()
        secs[name] = secs.get(name, 0.0) + t1 - t0
        t0 = t1

    # 1. the training set
    n_set = min(kmeans_sample_size(n, nlist, train_rows), OPQ_SET_ROWS)
    pick = _pick_rows(n, n_set, seed, dev)
    if flat is not None:
        raw = torch.empty((n_set, D), dtype=torch.int8, device=dev)
        flat.gather_rows_dev(pick.data_ptr(), n_set, raw.data_ptr(), stream=torch.cuda.current_stream(dev).cuda_stream)
        x = _dequant_dev(raw, _lut_dev(offset, scale, dev)).contiguous()
        del raw
    elif isinstance(rows, torch.Tensor):
        x = rows[pick.to(rows.device)].to(dev).contiguous()
    else:
        x = torch.from_numpy(np.ascontiguousarray(rows[pick.cpu().numpy()])).to(dev)
    bad = torch.nonzero(~torch.isfinite(x).all(dim=1)).flatten()
    if bad.numel():
        raise ValueError(f"train_index_resident: row {int(pick[bad[0]])} holds a NaN / Inf element ({int(bad.numel())} such rows in the training set)")
    seeds = draw_seeds(seed, n_set, M)
    lap("sample")
    # 2. OPQ
    A = torch.from_numpy(seeds["A0"]).to(dev)
    pqc, opq_err, opq_secs, splits = None, [], [], 0
    for it in range(int(opq_iters)):
        t_it = time.perf_counter()
        if pqc is None:
            pqc = init_codebooks_dev(rotate_dev(x, A), seeds["init_opq"])
        out = opq_iteration_dev(x, A, pqc, pq_iters_first if it == 0 else pq_iters)
        opq_err.append(out["err"])
        splits += out["splits"]
        A = torch.from_numpy(out["A_new"]).to(dev)
        del out
        opq_secs.append(time.perf_counter() - t_it)
    lap("opq")
    # 3. the coarse quantizer
    if centroids is not None:
        cent = torch.from_numpy(centroids).to(dev)
    else:
        c = train_centroids_resident(flat, nlist, iters=int(coarse_iters), train_rows=train_rows, seed=seed, offset=offset, scale=scale)
        cent = rotate_dev(torch.from_numpy(c).to(dev), A)
    lap("coarse")
    # 4. the PQ of the residuals
    from .ivf import _assign_dev
    xp = rotate_dev(x, A)
    lists, _ = _assign_dev(xp, cent.contiguous())
    res = (xp - cent[lists]).contiguous()
    del xp
    pqc = init_codebooks_dev(res, seeds["init_pq"])
    _, final_err, pq_err, s = lloyd_dev(res, pqc, final_pq_iters)
    splits += s
    lap("residual_pq")
    ivf_ix = faiss_io.IVFPQIndex(D, nlist, M, 8, cent.cpu().numpy(), pqc.cpu().numpy(), [np.zeros((0, M), np.uint8) for _ in range(nlist)],
                                 [np.zeros(0, np.int64) for _ in range(nlist)], True, faiss_io.METRIC_INNER_PRODUCT, 1, 2)
    index = faiss_io.PreTransformIndex([faiss_io.LinearTransform(A.cpu().numpy())], ivf_ix, D, True)
    if return_info:
        return index, {"set_rows": n_set, "rows": pick.cpu().numpy(), "opq_err": opq_err, "pq_err": pq_err, "final_err": final_err,
                       "codewords_split": splits, "seconds": secs, "opq_seconds_per_iter": opq_secs}
    return index
