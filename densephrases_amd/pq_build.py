"""The add step of the reference's index on the GPU: ``index.add_with_ids`` behind a TRAINED
IndexPreTransform(OPQMatrix) -> IndexIVFPQ (the reference's build_phrase_index.py:145-153, fed by add_to_index, :156-279).

Input: a parsed trained index (densephrases_amd.faiss_io.read_index of ``trained.faiss``: OPQ matrix, coarse centroids, codebooks, empty
lists) and the dump's rows; output: a resident, searchable PQ ``Shard`` -- the rows never leave HBM as fp32, their codes are built
where they lie (csrc/dph_pq_encode.hip).  The trained index itself: densephrases_amd/pq_train.py."""
from __future__ import annotations

from typing import Optional

import numpy as np

from . import _lib


def add_with_ids_resident(trained_index, rows, ids=None, device: int = 0, block: int = 1 << 20, offset: float = -2.0,
                          scale: float = 20.0) -> "_lib.Shard":
    """``rows``: a resident FLAT ``Shard`` (its int8 rows are de-quantised block by block through the exact table of
    ``ivf._lut_dev`` for the dump's codec ``offset`` / ``scale``), or an fp32 numpy / torch array [n,768].  ``ids`` (int64 [n], default ``arange(n)``: the reference's
    ``arange + offset + start_total`` with offset 0, build_phrase_index.py:149).  Every block goes through dph_pq_encode_dev into
    device staging arrays, one dph_index_fill_pq_dev builds the lists.  Returns the PQ shard with its lists set; the caller sets
    idx2id / f2o and finalizes.  A row with a NaN / Inf element raises ValueError."""
    import torch
    from .ivf import _dequant_dev, _lut_dev
    dev = torch.device("cuda", int(device))
    torch.cuda.set_device(dev)
    flat = rows if isinstance(rows, _lib.Shard) else None
    if flat is not None:
        if getattr(flat, "pq", None) is not None or flat.device != int(device):
            raise ValueError("add_with_ids_resident: `rows` must be a flat int8 shard on the same device")
        n = flat.n_rows

        class _Rows:
            __cuda_array_interface__ = {"shape": (n, _lib.DIM), "typestr": "|i1", "data": (flat.rows_dev_ptr(), False), "version": 2}
        src = torch.as_tensor(_Rows(), device=dev)
        lut = _lut_dev(offset, scale, dev)
    else:
        if isinstance(rows, torch.Tensor):
            src = rows
        else:
            import warnings
            with warnings.catch_warnings():                 # (a read-only array is fine: the rows are only read)
                warnings.simplefilter("ignore", UserWarning)
                src = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.float32))
        if src.ndim != 2 or src.shape[1] != _lib.DIM or src.dtype != torch.float32:
            raise ValueError("add_with_ids_resident: rows must be fp32 [n, 768]")
        n = int(src.shape[0])
    if n <= 0:
        raise ValueError("add_with_ids_resident: no rows")
    if ids is None:
        ids_dev = torch.arange(n, dtype=torch.int64, device=dev)
    else:
        ids_dev = torch.as_tensor(np.ascontiguousarray(ids, dtype=np.int64)).to(dev)
        if ids_dev.shape != (n,):
            raise ValueError("add_with_ids_resident: one id per row")
    shard = _lib.Shard.pq_from_trained(trained_index, n, device=device)
    try:
        M = shard.pq["M"]
        lists = torch.empty(n, dtype=torch.int32, device=dev)
        codes = torch.empty((n, M), dtype=torch.uint8, device=dev)
        st = torch.cuda.current_stream(dev).cuda_stream
        for r0 in range(0, n, int(block)):
            m = min(int(block), n - r0)
            x = _dequant_dev(src[r0:r0 + m], lut) if flat is not None else src[r0:r0 + m].to(dev).contiguous()
            shard.pq_encode_dev(x.data_ptr(), m, lists[r0:].data_ptr(), codes[r0:].data_ptr(), stream=st)
            torch.cuda.current_stream(dev).synchronize()        # x is released below: the kernels that read it have finished
            del x
        bad = torch.nonzero(lists < 0).flatten()
        if bad.numel():
            raise ValueError(f"add_with_ids_resident: row {int(bad[0])} holds a NaN / Inf element ({int(bad.numel())} such rows)")
        shard.pq_fill_dev(n, lists.data_ptr(), codes.data_ptr(), ids_dev.data_ptr(), stream=st)
    except BaseException:
        shard.close()
        raise
    return shard
