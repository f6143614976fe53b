"""Exact restatements of the IVFPQ and IVF searches in plain torch (test infrastructure), for indexes too large for the numpy oracles:
  gpu_ivfpq_search_synthetic       -- oracle/ivfpq_oracle.search over the index densephrases_amd.synth.synthetic_pq_parts describes, its
                                      codes regenerated from the parts (never read back from what the upload wrote);
  gpu_ivf_flat_search_regenerated  -- oracle.mips_oracle.ivf_flat_search over rows a callable regenerates chunk by chunk (never the
                                      list-major shard, so neither the builder nor row_ids can hide a bug).
Both run on any torch device; tests/test_full_size_ivf_pq.py holds them against the numpy oracles on the CPU.  Also the checks every
full-size test shares: the statistics of a call add up, and two answers of one exact search agree up to ties at the k-th place."""
import numpy as np

FLT_MAX = np.float32(3.4028234663852886e38)
ROLL = 97                                          # code of position p = block[(p % 2^20 - (p >> 20) % 97) mod 2^20] (synth.py)


def check_stats(st, n=None, where=""):
    """dph_search_stats of the last call: every field >= 0, the rows split into certified_fast + certified_wide + exact_fallback +
    uncertified + nonfinite, and the in-pass re-selects are a part of certified_wide"""
    assert all(v >= 0 for v in st.values()), (where, st)
    assert st["rows"] == (st["certified_fast"] + st["certified_wide"] + st["exact_fallback"] + st["uncertified"]
                          + st["nonfinite"]), (where, "the rows do not add up", st)
    assert st["certified_reselect"] <= st["certified_wide"], (where, st)
    if n is not None:
        assert st["rows"] == n, (where, st)


def same_up_to_kth_ties(D, I, Dw, Iw, where=""):
    """Two answers of one exact search, row by row: both put in (D desc, id asc) order, the scores equal bit for bit, and the ids
    equal except at an exact fp32 tie with the k-th score (a shard orders by the exact fp64 score, D is its fp32 rounding: rows of
    one fp32 score may come in either id order, and a tie ACROSS the k-th place may keep either row)."""
    assert D.shape == Dw.shape, where
    for r in range(D.shape[0]):
        a = np.lexsort((I[r], -D[r].astype(np.float64)))
        b = np.lexsort((Iw[r], -Dw[r].astype(np.float64)))
        np.testing.assert_array_equal(D[r][a], Dw[r][b], err_msg=f"{where} row {r}")
        diff = I[r][a] != Iw[r][b]
        assert not diff.any() or (D[r][a][diff] == D[r][a][-1]).all(), f"{where} row {r}: ids differ away from a tie at the k-th place"


def _ordered_topk(torch, s, ids, k):
    """the k best of one row's candidates by (score desc, id asc), exactly (torch.topk leaves the order of equal scores open)"""
    kk = min(k, s.numel())
    if kk == 0:
        return s[:0], ids[:0]
    kth = torch.topk(s, kk).values[-1]
    sel = torch.nonzero(s >= kth).flatten()
    sv, si = s[sel], ids[sel]
    o = torch.argsort(si)
    sv, si = sv[o], si[o]
    o = torch.sort(sv, descending=True, stable=True).indices[:kk]
    return sv[o], si[o]


def pq_coarse(x, parts, nprobe, device="cuda:0", rows=64):
    """(x' fp32 torch [n,768], probed lists int64 torch [n,nprobe] best first, dis0 fp32 torch [n,nprobe]) of the oracle's coarse step:
    x' = A x in float64 rounded once, float64 scores, (score desc, list asc)"""
    import torch
    dev = torch.device(device)
    sizes, A, cent, _, _ = parts[:5]
    x64 = torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(dev).to(torch.float64)
    xp = (x64 @ torch.from_numpy(A).to(dev).to(torch.float64).T).to(torch.float32)
    c64 = torch.from_numpy(cent).to(dev).to(torch.float64)
    nprobe = min(nprobe, c64.shape[0])
    lists, dis0 = [], []
    for r0 in range(0, xp.shape[0], rows):
        s = xp[r0:r0 + rows].to(torch.float64) @ c64.T
        o = torch.sort(s, dim=1, descending=True, stable=True).indices[:, :nprobe]      # (stable: equal scores keep list order)
        lists.append(o)
        dis0.append(torch.gather(s, 1, o).to(torch.float32))
    del c64
    return xp, torch.cat(lists), torch.cat(dis0)


def gpu_ivfpq_search_synthetic(x, parts, k, nprobe, device="cuda:0", code_budget=1 << 24, coarse=None):
    """oracle/ivfpq_oracle.search restated in torch for the index of ``synthetic_pq_parts(n, nlist, M, seed, skew)`` (by_residual,
    no bias): parts = (sizes, A, centroids, codebooks, block).  Position p of the list-major code array holds code
    block[(p % 2^20 - (p >> 20) % 97) mod 2^20] and id p; list l covers positions cumsum(sizes)[l-1] .. cumsum(sizes)[l].
    The oracle's arithmetic exactly: x' and the coarse scores as in ``pq_coarse``, each LUT entry a float64 sum rounded once to fp32,
    a code's score the SEQUENTIAL fp32 sum dis0 + LUT[0][c0] + LUT[1][c1] + ... (a loop over m of elementwise fp32 adds -- each an
    exact IEEE operation, so the order is the oracle's), top-k by (score desc, id asc) with -1 / -FLT_MAX padding.  Rows are
    scored together until their probed codes reach ``code_budget``.  Rows with a NaN / Inf element get the padding.
    Returns (D fp32 [n,k], I int64 [n,k], lists int64 [n,nprobe]: the probed lists best first)."""
    import torch
    dev = torch.device(device)
    sizes, A, cent, pqc, block = parts[:5]
    x = np.ascontiguousarray(x, np.float32)
    n, M = x.shape[0], pqc.shape[0]
    ksub, dsub = pqc.shape[1], 768 // pqc.shape[0]
    good = np.isfinite(x).all(1)
    xz = np.where(good[:, None], x, np.float32(0))
    xp, lists, dis0 = coarse if coarse is not None else pq_coarse(xz, parts, nprobe, device)
    nprobe = lists.shape[1]
    lut = torch.einsum("nmt,mjt->nmj", xp.to(torch.float64).reshape(n, M, dsub),
                       torch.from_numpy(pqc).to(dev).to(torch.float64)).to(torch.float32).reshape(n, M * ksub)
    sz = torch.from_numpy(np.asarray(sizes, np.int64)).to(dev)
    off = torch.cumsum(sz, 0) - sz
    blk = torch.from_numpy(block).to(dev)
    nb = blk.shape[0]
    D = np.full((n, k), -FLT_MAX, np.float32)
    I = np.full((n, k), -1, np.int64)
    per_row = sz[lists].sum(1).cpu().numpy()
    rows = [int(r) for r in np.nonzero(good)[0]]
    i = 0
    while i < len(rows):
        batch = [rows[i]]
        tot = int(per_row[rows[i]])
        i += 1
        while i < len(rows) and tot + int(per_row[rows[i]]) <= code_budget:
            tot += int(per_row[rows[i]])
            batch.append(rows[i])
            i += 1
        b = torch.tensor(batch, dtype=torch.int64, device=dev)
        ls = lists[b].flatten()                                         # [len(batch) * nprobe], row-major: a row's lists best first
        lens = sz[ls]
        start = torch.repeat_interleave(off[ls], lens)
        first = torch.repeat_interleave(torch.cumsum(lens, 0) - lens, lens)
        pos = start + torch.arange(start.numel(), device=dev) - first
        row_of = torch.repeat_interleave(torch.arange(len(batch), device=dev).repeat_interleave(nprobe), lens)
        codes = blk[torch.remainder(torch.remainder(pos, nb) - torch.div(pos, nb, rounding_mode="floor") % ROLL, nb)]
        acc = torch.repeat_interleave(dis0[b].flatten(), lens)
        base = (b[row_of] * (M * ksub))
        for m in range(M):
            acc = acc + lut.view(-1)[base + m * ksub + codes[:, m].to(torch.int64)]
        del codes, start, first, base
        cnt = sz[lists[b]].sum(1).cpu().numpy()
        seg = np.concatenate([[0], np.cumsum(cnt)])
        for j, r in enumerate(batch):
            sv, si = _ordered_topk(torch, acc[seg[j]:seg[j + 1]], pos[seg[j]:seg[j + 1]], k)
            D[r, :sv.numel()] = sv.cpu().numpy()
            I[r, :si.numel()] = si.cpu().numpy()
        del acc, pos, row_of
    return D, I, lists.cpu().numpy()


def gpu_ivf_flat_search_regenerated(x, centroids, assign, rows_fn, n, nprobe, k, id_base=0, chunk=1 << 22, block=1 << 17,
                                    device="cuda:0", offset=-2.0, factor=20.0):
    """oracle.mips_oracle.ivf_flat_search restated in torch float64 over rows REGENERATED chunk by chunk: ``rows_fn(r0, m)`` -> int8
    torch [m,768] on ``device`` (rows r0 .. r0+m-1 in id order), ``assign`` the product's row -> list assignment (torch int, length n,
    on ``device``).  Coarse: float64 scores over the centroids, the nprobe best lists by (score desc, list asc); in-list: float64 inner
    products of the fp32 de-quantised rows, selected block by block (at most ``block`` rows) with the GEMM and re-scored row by row
    (tests/_devdata._block_candidates), the running top-k kept by (score desc, id asc).  Returns (D fp32, I int64, D64) like the oracle."""
    import torch
    from oracle import mips_oracle as O
    from tests._devdata import _block_candidates
    dev = torch.device(device)
    lut = torch.from_numpy(O.dequant_lut(offset, factor).astype(np.float64)).to(dev)
    q = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev).to(torch.float64)
    n_q = q.shape[0]
    c64 = torch.from_numpy(np.ascontiguousarray(centroids, np.float32)).to(dev).to(torch.float64)
    cs = q @ c64.T
    probe = torch.sort(cs, dim=1, descending=True, stable=True).indices[:, :min(nprobe, c64.shape[0])]
    mask = torch.zeros((n_q, c64.shape[0]), dtype=torch.bool, device=dev)
    mask.scatter_(1, probe, True)
    best_q = torch.zeros(0, dtype=torch.int64, device=dev)
    best_i = torch.zeros(0, dtype=torch.int64, device=dev)
    best_s = torch.zeros(0, dtype=torch.float64, device=dev)
    for r0 in range(0, n, chunk):
        rows = rows_fn(r0, min(chunk, n - r0))
        for b0 in range(0, rows.shape[0], block):
            blk = rows[b0:b0 + block]
            allowed = mask[:, assign[r0 + b0:r0 + b0 + blk.shape[0]].to(torch.int64)]
            if not bool(allowed.any()):
                continue
            qi, ci, sc = _block_candidates(q, lut[blk.to(torch.int64) + 128], k, allowed, numpy=False)
            # running top-k of every query row by (score desc, id asc): three stable sorts give (row, -score, id) order
            aq, ai, asc = torch.cat([best_q, qi]), torch.cat([best_i, ci + (r0 + b0)]), torch.cat([best_s, sc])
            o = torch.argsort(ai, stable=True)
            o = o[torch.sort(asc[o], descending=True, stable=True).indices]
            o = o[torch.sort(aq[o], stable=True).indices]
            aq, ai, asc = aq[o], ai[o], asc[o]
            first = torch.searchsorted(aq, aq, right=False)
            keep = (torch.arange(aq.numel(), device=dev) - first) < k
            best_q, best_i, best_s = aq[keep], ai[keep], asc[keep]
        del rows
    D64 = np.full((n_q, k), -np.inf)
    I = np.full((n_q, k), -1, dtype=np.int64)
    bq, bi, bs = best_q.cpu().numpy(), best_i.cpu().numpy(), best_s.cpu().numpy()
    first = np.searchsorted(bq, bq)
    col = np.arange(bq.size) - first
    D64[bq, col] = bs
    I[bq, col] = bi + id_base
    D = np.where(I >= 0, D64, -np.float64(O.FLT_MAX)).astype(np.float32)
    return D, I, D64


def regenerated_rows(seed, kind, device=0):
    """rows_fn of ``gpu_ivf_flat_search_regenerated`` for the synthetic dump `kind`: libdph's generator on a throw-away shard
    (tests/test_gpu_search.py::test_synthetic_fill_matches_host_generator holds it to its numpy replica byte for byte)"""
    import torch
    from densephrases_amd import Shard
    from tests._devdata import _DevRows

    def rows_fn(r0, m):
        s = Shard(m, device=device, id_base=r0)
        try:
            s.fill_synthetic(seed=seed, kind=kind)
            torch.cuda.synchronize(device)
            return torch.as_tensor(_DevRows(s.rows_dev_ptr(), m), device=torch.device("cuda", device)).clone()
        finally:
            s.close()
    return rows_fn
