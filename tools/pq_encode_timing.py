#!/usr/bin/env python3
"""Timing of the add step of the OPQ + IVFPQ index on the GPU (csrc/dph_pq_encode.hip, densephrases_amd/pq_build.py).

A synthetic int8 flat shard resident in HBM (--kind, default 3: the mixture of 4096 Gaussians) is compressed behind a SYNTHETIC trained
index -- a random rotation, coarse centroids = de-quantised rows of the shard drawn at random (a k-means initialisation), codewords =
sub-vectors of residuals of other random rows; codebook TRAINING is not part of the library -- block by block through
dph_pq_encode_dev, then one dph_index_fill_pq_dev.  Per stage, HIP events (the handle's profiler, dph_profile_read_each(which = 2)):
transform, list estimate (fused MFMA assignment), list re-decision (float64, rows inside the error band), codes; torch events around
the de-quantisation of a block and around the fill.  One configuration per --nlist value.

For scale: oracle.ivfpq_oracle.add_with_ids (numpy / BLAS float64) over the first --cpu_rows rows on this machine's CPUs, and the fp32
matrix peak the codes kernel is priced against (157.3 TFLOP/s: 2 * 768 * 256 FLOP per row).

Writes ONE JSON file (--out, default profiles/pq_encode_timing.json) and prints it."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FP32_MATRIX_PEAK = 157.3e12


def synthetic_trained_index(flat, nlist, M, seed, offset=-2.0, scale=20.0):
    import torch
    from densephrases_amd import faiss_io as F
    from densephrases_amd.ivf import _dequant_dev, _lut_dev
    from oracle.ivfpq_oracle import random_rotation
    rng = np.random.default_rng(seed)
    dev = torch.device("cuda", flat.device)
    n, dsub = flat.n_rows, 768 // M

    def rows_at(idx):
        idx_t = torch.from_numpy(np.ascontiguousarray(idx, dtype=np.int64)).to(dev)
        out = torch.empty((len(idx), 768), dtype=torch.int8, device=dev)
        flat.gather_rows_dev(idx_t.data_ptr(), len(idx), out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
        return _dequant_dev(out, _lut_dev(offset, scale, dev))
    A = random_rotation(768, rng)
    At = torch.from_numpy(A.T.copy()).to(dev)
    cent = (rows_at(rng.integers(0, n, nlist)) @ At).cpu().numpy()
    # residuals of 4096 other rows against their best of 4096 of the centroids: where the codewords come from
    xs = rows_at(rng.integers(0, n, 4096)) @ At
    csub = torch.from_numpy(cent[rng.integers(0, nlist, min(nlist, 4096))]).to(dev)
    res = (xs - csub[(xs @ csub.T).argmax(1)]).cpu().numpy()
    pqc = np.stack([res[rng.integers(0, len(res), 256), m * dsub:(m + 1) * dsub] for m in range(M)]).astype(np.float32)
    ivf = F.IVFPQIndex(768, nlist, M, 8, cent.astype(np.float32), pqc, [np.zeros((0, M), np.uint8) for _ in range(nlist)],
                       [np.zeros(0, np.int64) for _ in range(nlist)], True, 0, 1, 2)
    return F.PreTransformIndex([F.LinearTransform(A)], ivf, 768, True)


def run(rows, nlist, M, block, kind, seed, cpu_rows):
    import torch
    from densephrases_amd import Shard
    from densephrases_amd.ivf import _dequant_dev, _lut_dev, dequant
    from densephrases_amd.synth import synthetic_rows
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    st = stream.cuda_stream
    flat = Shard(rows, device=0)
    flat.fill_synthetic(seed=seed, kind=kind)
    trained = synthetic_trained_index(flat, nlist, M, seed + 1)
    shard = Shard.pq_from_trained(trained, rows, device=0)
    shard.profile_enable(True)

    class _Rows:
        __cuda_array_interface__ = {"shape": (rows, 768), "typestr": "|i1", "data": (flat.rows_dev_ptr(), False), "version": 2}
    src = torch.as_tensor(_Rows(), device=dev)
    lut = _lut_dev(-2.0, 20.0, dev)
    lists = torch.empty(rows, dtype=torch.int32, device=dev)
    codes = torch.empty((rows, M), dtype=torch.uint8, device=dev)
    ids = torch.arange(rows, dtype=torch.int64, device=dev)
    # warm-up on a small block: first launches, LDS allowances, the scratch allocation
    x = _dequant_dev(src[:4096], lut)
    shard.pq_encode_dev(x.data_ptr(), 4096, lists.data_ptr(), codes.data_ptr(), stream=st)
    torch.cuda.synchronize(dev)
    shard.profile_read_each(2, cap=1 << 16)
    stages = {"dequant": 0.0, "transform": 0.0, "list_estimate": 0.0, "list_redecide": 0.0, "codes": 0.0}
    per_block = []
    t0 = time.perf_counter()
    for r0 in range(0, rows, block):
        m = min(block, rows - r0)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        x = _dequant_dev(src[r0:r0 + m], lut)
        e1.record(stream)
        shard.pq_encode_dev(x.data_ptr(), m, lists[r0:].data_ptr(), codes[r0:].data_ptr(), stream=st)
        torch.cuda.synchronize(dev)
        ms = shard.profile_read_each(2, cap=1 << 16).reshape(-1, 4).sum(0)
        blk = {"rows": m, "dequant": e0.elapsed_time(e1), "transform": float(ms[0]), "list_estimate": float(ms[1]),
               "list_redecide": float(ms[2]), "codes": float(ms[3])}
        per_block.append(blk)
        for k in stages:
            stages[k] += blk[k]
        del x
    encode_wall = time.perf_counter() - t0
    bad = int((lists < 0).sum())
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    t0 = time.perf_counter()
    shard.pq_fill_dev(rows, lists.data_ptr(), codes.data_ptr(), ids.data_ptr(), stream=st)
    e1.record(stream)
    torch.cuda.synchronize(dev)
    fill_wall = time.perf_counter() - t0
    sizes = shard.pq_list_sizes()
    out = {"rows": rows, "nlist": nlist, "M": M, "block": block, "kind": kind, "stage_ms": {k: round(v, 3) for k, v in stages.items()},
           "fill_ms": round(e0.elapsed_time(e1), 3), "fill_wall_s": round(fill_wall, 4), "encode_wall_s": round(encode_wall, 4),
           "rows_per_s": round(rows / (encode_wall + fill_wall), 1), "non_finite_rows": bad,
           "codes_rows_per_s": round(rows / (stages["codes"] * 1e-3), 1),
           "codes_fraction_of_fp32_matrix_peak": round(rows * 2.0 * 768 * 256 / (stages["codes"] * 1e-3) / FP32_MATRIX_PEAK, 4),
           "list_estimate_tflops": round(rows * 2.0 * 768 * nlist / (stages["list_estimate"] * 1e-3) / 1e12, 2),
           "lists_non_empty": int((sizes > 0).sum()), "longest_list": int(sizes.max()), "per_block": per_block}
    if cpu_rows:
        from oracle import ivfpq_oracle as P
        import copy
        xb = dequant(synthetic_rows(0, cpu_rows, seed=seed, kind=kind))
        t = copy.copy(trained)
        t.index = copy.copy(trained.index)
        t.index.list_codes, t.index.list_ids = list(t.index.list_codes), list(t.index.list_ids)
        t0 = time.perf_counter()
        P.add_with_ids(t, xb, np.arange(cpu_rows, dtype=np.int64))
        cpu_s = time.perf_counter() - t0
        got_l, got_c = lists[:cpu_rows].cpu().numpy(), codes[:cpu_rows].cpu().numpy()
        want_l = np.full(cpu_rows, -1, np.int64)
        want_c = np.zeros((cpu_rows, M), np.uint8)
        for l in range(nlist):
            i = np.asarray(t.index.list_ids[l])
            want_l[i] = l
            want_c[i] = np.asarray(t.index.list_codes[l])
        out["cpu_oracle"] = {"rows": cpu_rows, "seconds": round(cpu_s, 3), "rows_per_s": round(cpu_rows / cpu_s, 1),
                             "threads": int(os.environ.get("OMP_NUM_THREADS", "0")) or None,
                             "lists_differing": int((got_l != want_l).sum()), "cells_differing": int((got_c != want_c).sum())}
    shard.close()
    flat.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 22)
    ap.add_argument("--nlist", default="4096,1048576", help="comma list: one configuration each")
    ap.add_argument("--rows_long", type=int, default=1 << 18, help="rows of a configuration with more than 65536 lists (its assignment dominates)")
    ap.add_argument("--M", type=int, default=96)
    ap.add_argument("--block", type=int, default=1 << 20)
    ap.add_argument("--kind", type=int, default=3)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--cpu_rows", type=int, default=32768, help="rows the CPU oracle adds for scale (first configuration only; 0 = skip)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pq_encode_timing.json"))
    args = ap.parse_args()
    import torch
    import __graft_entry__ as g
    g.build()
    res = {"tool": "tools/pq_encode_timing.py", "device": torch.cuda.get_device_name(0), "fp32_matrix_peak_tflops": FP32_MATRIX_PEAK / 1e12, "configs": []}
    for j, nlist in enumerate(int(v) for v in args.nlist.split(",")):
        rows = args.rows if nlist <= 65536 else min(args.rows, args.rows_long)
        res["configs"].append(run(rows, nlist, args.M, args.block, args.kind, args.seed, args.cpu_rows if j == 0 else 0))
        print(json.dumps({k: v for k, v in res["configs"][-1].items() if k != "per_block"}), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:                      # (after every configuration: a later one that runs out of time loses nothing)
            json.dump(res, f, indent=1)
    print(json.dumps({"written": args.out}))


if __name__ == "__main__":
    main()
