"""IVF and OPQ + IVFPQ search at FULL size (170 M rows / codes) against exact restatements that run on the device
(tests/_fullsize.py), and those restatements against the numpy oracles on the CPU.

CPU (no GPU needed; each a few seconds):
  test_ivfpq_restatement_matches_the_numpy_oracle    -- gpu_ivfpq_search_synthetic vs oracle/ivfpq_oracle.search: ~60 k codes, 512
                                                        lists, M 48 / 96, list sizes "" / zipf, k beyond the probed codes, nprobe = nlist
  test_ivf_restatement_matches_the_numpy_oracle      -- gpu_ivf_flat_search_regenerated vs oracle.mips_oracle.ivf_flat_search: 30 k rows
                                                        of the mixture dump, 64 lists, nprobe 1 / 8 / 64
GPU (-m gpu, one MI355X):
  test_full_size_ivfpq[skew]   -- synthetic_pq_shard(170 M codes, 2^20 lists, M 96), skew "" and "zipf": ~20 GB of HBM, ~15 s to build;
                                  four calls (64 x k 10 x nprobe 256, 1025 x 200 x 256 with a NaN row, 1 x 1024 x 1024, 512 x 10 x 1),
                                  every row against the restatement; host and device forms equal bit for bit.
  test_full_size_ivf_4096      -- the mixture dump (170 M rows) built list-major in HBM with 4096 lists: 2 x 130 GB while the builder
                                  runs (skips below that, naming the free bytes), ~30 s to build; five calls under the masked scan and
                                  the unit scan, every row against the restatement (one float64 sweep over the regenerated rows per
                                  call: ~130 TFLOP at 512 rows), the two scans against each other, every list probed against the exact
                                  search.
Every search is followed by tests/_fullsize.check_stats (the rows of a call add up)."""
import time

import numpy as np
import pytest

from oracle import mips_oracle as O
from tests._fullsize import FLT_MAX, check_stats, gpu_ivf_flat_search_regenerated, gpu_ivfpq_search_synthetic, same_up_to_kth_ties


def _pq_index(parts, n):
    """the IVFPQIndex the parts describe, built the way synthetic_pq_shard uploads it (chunks of the rolled code block)"""
    from densephrases_amd import faiss_io as F
    sizes, A, cent, pqc, block = parts
    nb = block.shape[0]
    codes = np.concatenate([np.roll(block, pos // nb % 97, axis=0)[:min(nb, n - pos)] for pos in range(0, n, nb)])
    cut = np.cumsum(sizes)[:-1]
    ivf = F.IVFPQIndex(768, len(sizes), pqc.shape[0], 8, cent, pqc, np.split(codes, cut), np.split(np.arange(n, dtype=np.int64), cut),
                       True, 0, 1, 2)
    return F.PreTransformIndex([F.LinearTransform(A)], ivf, 768, True)


def _pq_queries(rng, A, cent, n_q):
    """half the rows A^T (u c_l) + noise for a random list l and u in [0.3, 1] (x' = u c_l + noise: near list l), half N(0, 0.5)"""
    x = rng.normal(0, 0.5, (n_q, 768)).astype(np.float32)
    near = rng.integers(0, len(cent), n_q // 2)
    u = rng.uniform(0.3, 1.0, (len(near), 1)).astype(np.float32)
    x[:len(near)] = ((cent[near] * u) @ A).astype(np.float32) + x[:len(near)] * np.float32(0.2)
    return x


@pytest.mark.parametrize("M,skew,block", [(48, "", 1 << 20), (96, "zipf", 1 << 20), (96, "", 4096)])
def test_ivfpq_restatement_matches_the_numpy_oracle(M, skew, block):
    """(block 4096: a short code block, so that positions pass it several times and the roll (p >> log2 block) % 97 is exercised)"""
    from densephrases_amd.synth import synthetic_pq_parts
    from oracle import ivfpq_oracle as P
    from tests.test_pq import _same_topk
    n, nlist = 60_000, 512
    sizes, A, cent, pqc, blk = synthetic_pq_parts(n, nlist, M, seed=3, skew=skew)
    parts = (sizes, A, cent, pqc, blk[:block])
    ix = _pq_index(parts, n)
    rng = np.random.default_rng(M + block)
    for n_q, k, nprobe in ((12, 10, 16), (5, 1024, 1), (3, 100, nlist), (6, 200, 64)):
        x = _pq_queries(rng, A, cent, n_q)
        D, I, lists = gpu_ivfpq_search_synthetic(x, parts, k, nprobe, device="cpu", code_budget=20_000)
        Dr, Ir = P.search(ix, x, k, nprobe)
        assert lists.shape == (n_q, min(nprobe, nlist))
        if nprobe == 1:
            assert (I[:, -1] == -1).all() and (D[:, -1] == -FLT_MAX).all()         # k beyond the probed codes: padding
        _same_topk(D, I, Dr, Ir)
        np.testing.assert_array_equal(I, Ir)                                    # (same arithmetic: no near-tie swaps expected here)


@pytest.mark.parametrize("nprobe", [1, 8, 64])
def test_ivf_restatement_matches_the_numpy_oracle(nprobe):
    import torch
    from densephrases_amd.synth import synthetic_rows
    n, nlist = 30_000, 64
    xb = synthetic_rows(0, n, seed=5, kind=3)
    rng = np.random.default_rng(nprobe)
    cent = (O.int8_to_float(xb[rng.choice(n, nlist, replace=False)]) + rng.normal(0, 0.1, (nlist, 768))).astype(np.float32)
    assign = np.argmax(O.int8_to_float(xb).astype(np.float64) @ cent.astype(np.float64).T, 1)
    x = np.concatenate([O.int8_to_float(xb[rng.integers(0, n, 8)]) + rng.normal(0, 0.25, (8, 768)),
                        rng.normal(0, 0.5, (6, 768))]).astype(np.float32)
    for k in (10, 100):
        D, I, D64 = gpu_ivf_flat_search_regenerated(x, cent, torch.from_numpy(assign), lambda r0, m: torch.from_numpy(xb[r0:r0 + m]),
                                                    n, nprobe, k, chunk=8192, block=3000, device="cpu")
        Dr, Ir, D64r = O.ivf_flat_search(x, xb, cent, assign, nprobe, k)
        ok, msg = O.topk_equivalent(D, I, D64r, Ir)
        assert ok, (nprobe, k, msg)
        np.testing.assert_array_equal(I, Ir)


# ----------------------------------------------------------------------------------------------------------------- GPU: IVFPQ
def _dev_search(s, x, k, nprobe):
    import torch
    dev = torch.device("cuda", 0)
    xd = torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    Dd = torch.empty((len(x), k), dtype=torch.float32, device=dev)
    Id = torch.empty((len(x), k), dtype=torch.int64, device=dev)
    sd = torch.full((len(x),), -7, dtype=torch.int32, device=dev)
    s.search_ivf_dev(xd.data_ptr(), len(x), k, nprobe, Dd.data_ptr(), Id.data_ptr(), sd.data_ptr())
    torch.cuda.synchronize()
    return Dd.cpu().numpy(), Id.cpu().numpy(), sd.cpu().numpy()


def check_pq_call(s, parts, x, k, nprobe, bad, where, coarse_note):
    """one call on a PQ handle, host and device forms: statuses, statistics, the NaN rows' padding, every row against the
    restatement (tests/test_pq.py::_same_topk), the two forms bit for bit.  Returns the probed lists of every row."""
    from tests.test_pq import _same_topk
    n_q = len(x)
    D, I = s.search_ivf(x, k, nprobe)
    st = s.stats()
    check_stats(st, n_q, where)
    assert st["uncertified"] == 0 and st["nonfinite"] == len(bad), (where, st)
    failed_over = s.debug_pq_coarse()[0]
    if failed_over:
        coarse_note.append(f"{where}: the coarse filter failed over to the bf16x3 chain")
    Dd, Id, status = _dev_search(s, x, k, nprobe)
    check_stats(s.stats(), n_q, where)
    assert s.stats()["nonfinite"] == len(bad) and s.stats()["uncertified"] == 0, (where, s.stats())
    np.testing.assert_array_equal(Id, I, err_msg=where)
    np.testing.assert_array_equal(Dd, D, err_msg=where)
    good = np.setdiff1d(np.arange(n_q), bad)
    assert (status[good] == 0).all() and (status[bad] == 3).all(), (where, np.bincount(status[status >= 0], minlength=4))
    assert (I[bad] == -1).all() and (D[bad] == -FLT_MAX).all(), where
    t0 = time.perf_counter()
    Dr, Ir, lists = gpu_ivfpq_search_synthetic(x, parts, k, nprobe)
    print(f"{where}: restatement {time.perf_counter() - t0:.1f} s; {' '.join(coarse_note)}")
    try:
        _same_topk(D[good], I[good], Dr[good], Ir[good])
    except AssertionError as e:
        raise AssertionError(f"{where}: {e}; {' '.join(coarse_note)}") from None
    return lists[good]


@pytest.mark.gpu
@pytest.mark.parametrize("skew", ["", "zipf"])
def test_full_size_ivfpq(skew):
    """The reference's own index type at its size: OPQ + IVFPQ, 2^20 lists, M 96, 170 M codes -- the bf16 coarse filter as a teams
    scan over 2^20 centroids, long lists cut into units by code count (zipf: the longest list ~800 k codes), candidate buffers of 2^20
    entries.  Four calls on one handle, larger then smaller requests on its scratch."""
    import torch
    from densephrases_amd.synth import synthetic_pq_shard
    n = 170_000_000
    t0 = time.perf_counter()
    s, A, cent, sizes, pqc, block = synthetic_pq_shard(n, 1 << 20, 96, return_parts=True, doc_len=100, skew=skew)
    print(f"IVFPQ n {n} skew {skew!r}: built in {time.perf_counter() - t0:.1f} s")
    parts = (sizes, A, cent, pqc, block)
    rng = np.random.default_rng(17 + len(skew))
    longest = np.argsort(sizes)[::-1][:3]
    hot_rows, notes = 0, []
    try:
        for n_q, k, nprobe in ((64, 10, 256), (1025, 200, 256), (1, 1024, 1024), (512, 10, 1)):
            x = _pq_queries(rng, A, cent, n_q)
            bad = np.zeros(0, np.int64)
            if n_q == 1025:
                bad = np.asarray([int(rng.integers(0, n_q))])
                x[bad[0], int(rng.integers(0, 768))] = np.nan
            where = f"IVFPQ n {n} skew {skew!r} n_q {n_q} k {k} nprobe {nprobe}"
            lists = check_pq_call(s, parts, x, k, nprobe, bad, where, notes)
            hot_rows += int(np.isin(lists, longest).any(1).sum())
        if skew == "zipf":
            assert hot_rows >= 16, (f"only {hot_rows} rows probed one of the three longest lists", sizes[longest])
        print(f"IVFPQ skew {skew!r}: {hot_rows} rows probed one of the three longest lists ({sizes[longest].tolist()} codes)")
    finally:
        s.close()
        del s
        torch.cuda.empty_cache()


# -------------------------------------------------------------------------------------------------------------------- GPU: IVF
def check_ivf_calls(s, x, k, nprobe, nlist, want, where):
    """one (queries, k, nprobe) on a list-major IVF handle under the masked scan and the unit scan: every row against the
    restatement ``want`` = (D, I, D64) under topk_equivalent, the two scans against each other; with every list probed, also
    against the exact search of the same handle.  The device form's statuses are all 0."""
    got = {}
    for units in (0, 1):
        s.set_tuning("ivf_units", units)
        D, I = s.search_ivf(x, k, nprobe)
        st = s.stats()
        check_stats(st, len(x), f"{where} units {units}")
        assert st["uncertified"] == 0, (where, units, st)
        ok, msg = O.topk_equivalent(D, I, want[2], want[1])
        assert ok, f"{where} units {units}: {msg}"
        got[units] = (D, I)
    s.set_tuning("ivf_units", -1)
    same_up_to_kth_ties(got[1][0], got[1][1], got[0][0], got[0][1], f"{where}: unit scan vs masked scan")
    Dd, Id, status = _dev_search(s, x, k, nprobe)
    check_stats(s.stats(), len(x), where)
    assert (status == 0).all(), (where, np.bincount(status[status >= 0], minlength=4))
    same_up_to_kth_ties(Dd, Id, got[1][0], got[1][1], f"{where}: device form vs host form")
    if nprobe >= nlist:
        De, Ie = s.search(x, k)
        check_stats(s.stats(), len(x), where)
        assert s.stats()["uncertified"] == 0, where
        same_up_to_kth_ties(got[0][0], got[0][1], De, Ie, f"{where}: every list probed vs the exact search")


@pytest.mark.gpu
def test_full_size_ivf_4096():
    """BASELINE configs[3] at full size, the recipe of bench.py's also_ivf: the mixture dump (kind 3) generated in HBM, k-means lists
    trained on a sample, every row assigned, the list-major shard built in HBM (byte offsets of the rows pass 2^32), groups of 128 and
    256 query rows against lists of ~41 k rows."""
    import gc
    import torch
    from densephrases_amd import Shard
    from densephrases_amd.ivf import make_list_major_resident
    from densephrases_amd.synth import synthetic_rows
    from tests._fullsize import regenerated_rows
    n, nlist, seed, kind = 170_000_000 // 32 * 32, 4096, 42, 3
    gc.collect()
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info(0)
    if free < 2 * n * 768 + (12 << 30):
        pytest.skip(f"the list builder needs 2 x {n * 768} + 12 GiB bytes of free HBM; {free} bytes are free")
    t0 = time.perf_counter()
    s = Shard(n, device=0)
    try:
        s.fill_synthetic(seed=seed, kind=kind)
        cent, assign = make_list_major_resident(s, nlist)
        s.finalize()
        torch.cuda.synchronize()
        print(f"IVF n {n} nlist {nlist}: built in {time.perf_counter() - t0:.1f} s")
        rng = np.random.default_rng(23)
        # the assignment: the float64 arg-max over the centroids of the host replica's rows
        pick = rng.integers(0, n, 4096)
        rows = np.stack([synthetic_rows(int(r), 1, seed=seed, kind=kind)[0] for r in pick])
        want = np.argmax(O.int8_to_float(rows).astype(np.float64) @ cent.astype(np.float64).T, 1)
        np.testing.assert_array_equal(assign[torch.from_numpy(pick).cuda()].cpu().numpy(), want)
        rows_fn = regenerated_rows(seed, kind)
        for n_q, k, nprobe in ((256, 10, 256), (512, 200, 256), (1, 1024, 16), (64, 10, 1), (64, 10, nlist)):
            half = n_q // 2 + (n_q % 2)
            base = np.stack([synthetic_rows(int(r), 1, seed=seed, kind=kind)[0] for r in rng.integers(0, n, half)])
            x = np.concatenate([O.int8_to_float(base) + rng.normal(0, 0.25, (half, 768)),
                                rng.normal(0, 0.5, (n_q - half, 768))]).astype(np.float32)
            where = f"IVF n {n} nlist {nlist} n_q {n_q} k {k} nprobe {nprobe}"
            t1 = time.perf_counter()
            ref = gpu_ivf_flat_search_regenerated(x, cent, assign, rows_fn, n, nprobe, k)
            print(f"{where}: restatement {time.perf_counter() - t1:.1f} s")
            check_ivf_calls(s, x, k, nprobe, nlist, ref, where)
    finally:
        s.close()
        del s
        gc.collect()
        torch.cuda.empty_cache()
