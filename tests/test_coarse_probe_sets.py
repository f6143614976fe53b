"""The probed SET of the coarse quantizer (csrc/dph_ivf.hip), looked at directly.  dph.h promises that the lists a query row probes
are the float64 oracle's, in (score desc, list id asc) order; every other IVF / IVFPQ test sees the probe set only through the final
top-k, where a list wrongly swapped in or out at the nprobe-th place almost never holds a top-10 row.  Here the index holds exactly
ONE row (one PQ code) per list and k = min(nprobe, nlist): the returned ids are the probed lists (tests/_coarse_sets.py), and they
are held against ``np.lexsort((list id, -float64 score))[:k]`` row by row -- through the radix select, the one-pass estimate /
collect path (nlist >= 8192), the fp32 error band and the float64 band re-rank with its list-id tie rule (flat-IVF path), and through
the fp32 chain, the bf16x3 chain and the filter of the PQ path."""
import numpy as np
import pytest

from oracle import mips_oracle as O
from tests import _coarse_sets as CS


# ------------------------------------------------------------------------------------------------- CPU: the reveal holds for the oracle
def test_one_row_per_list_reveals_the_probe_set_of_the_oracle():
    """``O.ivf_flat_search`` over a one-row-per-list index with k = min(nprobe, nlist) returns exactly the float64 (score desc, list
    id asc) probe set -- with 40 exact copies of one centroid and 40 one-ulp variants of another on the probe boundary."""
    nlist = 600
    rng = np.random.default_rng(3)
    cent, src, block = CS.centroid_set("dup", nlist, seed=5)
    cent2, src2, block2 = CS.centroid_set("ulp", nlist, seed=6)
    free = np.setdiff1d(np.arange(nlist), np.concatenate([block, [src]]))
    tgt = rng.choice(free, len(block2) + 1, replace=False)             # the one-ulp block next to the copies, in one centroid set
    cent[tgt] = cent2[np.concatenate([[src2], block2])]
    xb = O.float_to_int8(rng.normal(0.0, 0.6, (nlist, 768)).astype(np.float32))
    x = rng.normal(0.0, 0.5, (6, 768)).astype(np.float32)
    x[0], x[1], x[2] = cent[src], cent[tgt[0]], cent[src] * 0.5 + cent[tgt[0]] * 0.5
    s64, order = CS.float64_order(x, cent)
    assert CS.band_occupancy(s64, order, 41, x, cent).max() < CS.CS_BAND_CAP
    for nprobe in (1, 2, 20, 40, 41, 42, 43, 81, 82, 83, 300, 599, 600, 700):
        k = min(nprobe, nlist)
        D, I, _ = O.ivf_flat_search(x, xb, cent, np.arange(nlist), nprobe, k)
        assert (I >= 0).all()
        for r in range(x.shape[0]):
            assert set(I[r].tolist()) == set(order[r, :k].tolist()), (nprobe, r, CS.explain(I[r], order[r], s64[r], k, block, src))


# ------------------------------------------------------------------------------------------------- GPU helpers
def _one_row_per_list_shard(cent, seed, id_base=0):
    """a list-major shard with one (random) row in every list: build_list_major accepts any assignment, the rows need not be near
    their centroids"""
    from densephrases_amd import Shard
    from densephrases_amd.ivf import build_list_major
    nlist = cent.shape[0]
    xb = O.float_to_int8(np.random.default_rng(seed).normal(0.0, 0.6, (nlist, 768)).astype(np.float32))
    stored, row_ids, tile_list = build_list_major(xb, np.arange(nlist), nlist, id_base=id_base)
    s = Shard(stored.shape[0], device=0, id_base=id_base)
    s.upload(stored)
    s.set_row_ids(row_ids, nlist)
    s.set_ivf(cent, tile_list)
    s.finalize()
    return s


def _search_ivf_dev(s, x, k, nprobe):
    """dph_search_ivf_dev on device tensors -> (D, I, status) as numpy"""
    import torch
    dev = torch.device("cuda", 0)
    xd = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev)
    n = x.shape[0]
    D = torch.empty((n, k), dtype=torch.float32, device=dev)
    I = torch.empty((n, k), dtype=torch.int64, device=dev)
    st = torch.full((n,), -7, dtype=torch.int32, device=dev)
    s.search_ivf_dev(xd.data_ptr(), n, k, nprobe, D.data_ptr(), I.data_ptr(), st.data_ptr(), stream=torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    return D.cpu().numpy(), I.cpu().numpy(), st.cpu().numpy()


def _assert_probe_sets(I, order, s64, k, block, src, id_base, what):
    assert (I >= 0).all(), (what, "padding ids among the results: a probed list is missing")
    got = np.sort(I - id_base, axis=1)
    want = np.sort(order[:I.shape[0], :k], axis=1)
    bad = np.nonzero((got != want).any(1))[0]
    assert bad.size == 0, (what, f"{bad.size} rows differ, first {int(bad[0])}",
                           CS.explain(got[bad[0]], order[bad[0]], s64[bad[0]], k, block, src))


# ------------------------------------------------------------------------------------------------- A: the flat-IVF path
# (nlist, centroid set, id_base): 8192 = CS_FAST_MIN where the one-pass candidate path starts, 8191 the last size below it,
# 128 / 129 the edge of the GEMM's 128-list tile, 20000 a score row of twenty radix trips
_FLAT_CASES = [(37, "random", 0), (37, "dup", 9000), (128, "ulp", 0), (129, "dup", 0), (129, "long", 500),
               (4096, "random", 0), (4096, "dup", 0), (4096, "ulp", 1 << 33), (4096, "long", 0),
               (8191, "dup", 0), (8191, "ulp", 0), (8192, "random", 0), (8192, "dup", 77), (8192, "ulp", 0),
               (20000, "random", 0), (20000, "dup", 0), (20000, "ulp", 0), (20000, "long", 123456)]
_NPROBES = (1, 2, 31, 256, 1024)
_NQS = (1, 127, 128, 129, 700)


@pytest.mark.gpu
@pytest.mark.parametrize("nlist,kind,id_base", _FLAT_CASES)
def test_flat_ivf_probe_sets_equal_the_float64_order(nlist, kind, id_base):
    """dph_search_ivf on a one-row-per-list shard (fp32 MFMA GEMM + select + float64 band re-rank): for every query row the returned
    ids are the float64 probe set.  nprobe 1 / 2 / 31 / 256 / 1024, one value >= nlist, and -- with a block of copies or one-ulp
    variants on top -- the values that cut before, inside, at the end of and just past the block; batches of 1 / 127 / 128 / 129 / 700
    query rows; the masked scan and the unit scan (ivf_units 0 / 1).  Every nprobe runs under both scans, the batch sizes rotate.
    Precondition (asserted): fewer than CS_BAND_CAP lists inside the error band of the nprobe-th score -- above that the flat-IVF
    path cuts the band by design (dph_coarse_select_kernel), which is not what is tested here."""
    cent, src, block = CS.centroid_set(kind, nlist, seed=nlist + len(kind))
    x = CS.query_rows(cent, src, block, kind, max(_NQS), seed=nlist + 1)
    s64, order = CS.float64_order(x, cent)
    s = _one_row_per_list_shard(cent, seed=nlist + 2, id_base=id_base)
    nprobes = sorted({p for p in _NPROBES if p <= min(nlist, 1024)} | ({nlist + 5} if nlist <= 1024 else set()) |
                     (set(CS.block_nprobes(block, nlist)) if kind in ("dup", "ulp") else set()))
    worst_occ = 0
    for i, nprobe in enumerate(nprobes):
        k = min(nprobe, nlist)                           # (the library caps k at 1024: nprobe beyond it cannot be revealed this way)
        occ = int(CS.band_occupancy(s64, order, k, x, cent).max())
        worst_occ = max(worst_occ, occ)
        assert occ < CS.CS_BAND_CAP, (nprobe, occ)
        for units in (0, 1):
            n_q = _NQS[(i + 2 * units) % len(_NQS)]
            s.set_tuning("ivf_units", units)
            D, I = s.search_ivf(x[:n_q], k, nprobe)
            what = (nlist, kind, nprobe, n_q, units)
            _assert_probe_sets(I, order, s64, k, block, src, id_base, what)
            assert s.stats()["uncertified"] == 0, (what, s.stats())
    print(f"flat probe sets {nlist} {kind}: nprobes {nprobes}, worst band occupancy {worst_occ}")
    s.close()


@pytest.mark.gpu
def test_flat_ivf_with_nprobe_beyond_8192_lists_is_the_exact_search():
    """nprobe >= nlist at 8192 lists (the one-pass path with every list a candidate): every list is probed, so the 1024 results are
    the flat oracle's over the 8192 rows -- the reveal itself needs k = nlist <= 1024 and is part of the test above (nlist + 5)."""
    nlist, k = 8192, 1024
    cent, src, block = CS.centroid_set("dup", nlist, seed=nlist)
    x = CS.query_rows(cent, src, block, "dup", 129, seed=4)
    s = _one_row_per_list_shard(cent, seed=5)
    xb = O.float_to_int8(np.random.default_rng(5).normal(0.0, 0.6, (nlist, 768)).astype(np.float32))      # the shard's rows
    Dr, Ir, D64 = O.flat_ip_search(x, xb, k)
    for units in (0, 1):
        s.set_tuning("ivf_units", units)
        for nprobe in (nlist, nlist + 100):
            D, I = s.search_ivf(x, k, nprobe)
            ok, msg = O.topk_equivalent(D, I, D64, Ir)
            assert ok, (units, nprobe, msg)
            assert s.stats()["uncertified"] == 0
    s.close()


@pytest.mark.gpu
def test_flat_ivf_probe_sets_through_the_device_entry_point_and_the_nprobe_tuning_key():
    """The same reveal through dph_search_ivf_dev (status all 0) and through plain dph_search with the tuning key "nprobe", on a
    shard with id_base != 0 and the one-ulp block on the boundary."""
    nlist, id_base = 8192, 70000
    cent, src, block = CS.centroid_set("ulp", nlist, seed=81)
    x = CS.query_rows(cent, src, block, "ulp", 129, seed=82)
    s64, order = CS.float64_order(x, cent)
    s = _one_row_per_list_shard(cent, seed=83, id_base=id_base)
    for nprobe in (len(block) // 2, len(block) + 2, 256):
        assert CS.band_occupancy(s64, order, nprobe, x, cent).max() < CS.CS_BAND_CAP
        D, I, st = _search_ivf_dev(s, x, nprobe, nprobe)
        assert (st == 0).all(), st
        _assert_probe_sets(I, order, s64, nprobe, block, src, id_base, ("dev", nprobe))
        s.set_tuning("nprobe", nprobe)
        D2, I2 = s.search(x, nprobe)
        _assert_probe_sets(I2, order, s64, nprobe, block, src, id_base, ("tuning key", nprobe))
        assert s.stats()["uncertified"] == 0
        s.set_tuning("nprobe", 0)
    s.close()


# ------------------------------------------------------------------------------------------------- B: the PQ path
def _one_code_per_list_index(cent, seed, M=96):
    """IndexPreTransform(identity) -> IndexIVFPQ with one (random) code in every list, id = list number: x' = x exactly"""
    from densephrases_amd import faiss_io as F
    rng = np.random.default_rng(seed)
    nlist = cent.shape[0]
    pqc = rng.normal(0, 0.1, (M, 256, 768 // M)).astype(np.float32)
    codes = rng.integers(0, 256, (nlist, M), dtype=np.uint8)
    ids = np.arange(nlist, dtype=np.int64)
    ivf = F.IVFPQIndex(768, nlist, M, 8, cent, pqc, [codes[i:i + 1] for i in range(nlist)], [ids[i:i + 1] for i in range(nlist)],
                       True, 0, 1, 2)
    return F.PreTransformIndex([F.LinearTransform(np.eye(768, dtype=np.float32))], ivf, 768, True)


def _pq_shard(ix):
    from densephrases_amd import Shard
    s = Shard.from_faiss_index(ix, device=0)
    n = s.ntotal
    s.set_idx2id(np.zeros(n, np.int32), np.arange(n, dtype=np.int32))
    s.set_f2o(np.zeros(1, np.int32), np.asarray([0, n], np.int64), np.arange(n, dtype=np.int32))
    s.finalize()
    return s


def _oracle_probe(ix, x, nprobe, chunk=64):
    """the oracle's coarse_probe on apply_chain(ix.chain, x), in chunks of rows (its lexsort is over whole score rows)"""
    from oracle import ivfpq_oracle as P
    xp = P.apply_chain(ix.chain, x)
    return np.concatenate([P.coarse_probe(xp[r0:r0 + chunk], ix.index.centroids, nprobe)[0] for r0 in range(0, len(xp), chunk)])


# (filter, teams, (n_q, nprobe) ...): the filter with both team settings and the chain alone, every n_q and every nprobe of the
# issue at least once; the order statistics of the filter depend on nprobe, the team launch on n_q > 128.  (The combinations the
# removed GEMM forms of the filter ran are kept: those of more than 128 rows under both team settings.)
_PQ_RANDOM_RUNS = [(1, 1, ((1024, 256), (129, 1024), (5, 1), (129, 40), (1024, 1), (129, 1), (129, 256), (1024, 1024), (5, 1024), (5, 256))),
                   (1, 0, ((1024, 40), (129, 256), (129, 40), (1024, 1), (129, 1), (1024, 1024), (5, 40))),
                   (0, 1, ((129, 1024), (5, 40)))]


@pytest.mark.gpu
@pytest.mark.parametrize("nlist", [4096, 65536])
@pytest.mark.parametrize("kind", ["random", "dup", "ulp"])
def test_pq_probe_sets_equal_the_oracles_coarse_probe(nlist, kind):
    """dph_search_ivf on an IVFPQ handle with one code per list: the returned ids are the lists of ``coarse_probe(apply_chain(q))``.
    4096 lists take the fp32 chain; 65536 lists the bf16x3 chain (coarse_filter 0) and the filter in front of it (with and without
    teams), which must not fail over on these centroid sets.  Random centroids: 5 / 129 / 1024 query rows x nprobe 1 / 40 / 256 /
    1024.  Copies / one-ulp variants: 129 rows, nprobe cutting before, inside, at the end of and just past the block, and 40 / 256."""
    cent, src, block = CS.centroid_set(kind, nlist, seed=nlist // 7 + len(kind))
    ix = _one_code_per_list_index(cent, seed=nlist + 3)
    s = _pq_shard(ix)
    n_all = 1024 if kind == "random" else 129
    x = CS.query_rows(cent, src, block, kind, n_all, seed=nlist + 4)
    pmax = 1024 if kind == "random" else 256
    lists = _oracle_probe(ix, x, pmax)                     # best first: the probe set of a smaller nprobe is its prefix
    if kind == "random":
        runs = _PQ_RANDOM_RUNS
    else:
        combos = tuple((129, p) for p in sorted(set(CS.block_nprobes(block, nlist)) | {40, 256}))
        runs = [(f, t, combos) for f, t in ((1, 1), (1, 0), (0, 1))]
    if nlist < 65536:                                      # no filter images below CG_BF16X3_MIN lists: one setting is all there is
        runs = [(1, 1, tuple(sorted({c for _, _, cs in runs for c in cs})))]
    for filt, teams, combos in runs:
        s.set_tuning("coarse_filter", filt)
        s.set_tuning("coarse_teams", teams)
        for n_q, nprobe in combos:
            k = nprobe
            D, I, st = _search_ivf_dev(s, x[:n_q], k, nprobe)
            what = (nlist, kind, filt, teams, n_q, nprobe)
            assert (st == 0).all(), (what, np.nonzero(st)[0][:8], st[st != 0][:8])
            assert (I >= 0).all(), what
            got, want = np.sort(I, axis=1), np.sort(lists[:n_q, :k], axis=1)
            bad = np.nonzero((got != want).any(1))[0]
            if bad.size:
                r = int(bad[0])
                extra, missing = set(got[r].tolist()) - set(want[r].tolist()), set(want[r].tolist()) - set(got[r].tolist())
                blk = set(block.tolist()) | {src}
                sc = (x[r].astype(np.float64) @ cent.astype(np.float64).T)
                rank = {int(l): i for i, l in enumerate(np.lexsort((np.arange(nlist), -sc)).tolist())}
                raise AssertionError((what, f"{bad.size} rows differ, first {r}",
                                      "extra (list, f64 rank, score, in block)", [(l, rank[l], float(sc[l]), l in blk) for l in sorted(extra)[:8]],
                                      "missing", [(l, rank[l], float(sc[l]), l in blk) for l in sorted(missing)[:8]]))
            if filt and nlist >= 65536:
                failed_over, emitted = s.debug_pq_coarse()
                assert failed_over is False and emitted >= nprobe * n_q, (what, failed_over, emitted)
    s.close()
