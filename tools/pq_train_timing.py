#!/usr/bin/env python3
"""Timing of the train step of the OPQ + IVFPQ index on the GPU (csrc/dph_pq_train.hip, densephrases_amd/pq_train.py).

A synthetic int8 flat shard resident in HBM (--kind, default 3: the mixture of 4096 Gaussians) is handed to
pq_train.train_index_resident with FAISS' defaults (10 OPQ iterations of 40 / 4 Lloyd steps, 25 steps for the residual codebooks, a
65 536-point training set); wall seconds per stage (sample, OPQ, coarse k-means, residual PQ) come from the trainer's own record, and one
Lloyd step over the set is timed on its own: dph_pq_train_step_dev with and without the update, and dph_pq_decode_dev.  One configuration
per --nlist value; a configuration with more than 65 536 lists runs over --rows_long rows and --coarse_iters_long coarse iterations (its
coarse k-means is the assignment of every training row to 2^20 lists, tens of seconds per iteration: the file says how many were run).

No target is set for these times.  Writes ONE JSON file (--out, default profiles/pq_train_timing.json) and prints it."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def time_step(M, n_set, seed):
    """ms of one Lloyd step / one assignment / one decode over n_set rows (median of 5 after a warm-up)"""
    import numpy as np
    import torch
    from densephrases_amd.pq_train import decode_dev, train_step_dev
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(seed)
    x = torch.randn((n_set, 768), generator=g, device=dev, dtype=torch.float32)
    pqc = x[:256].reshape(256, M, 768 // M).permute(1, 0, 2).contiguous()
    out = {}
    for name, fn in (("step_update_ms", lambda: train_step_dev(x, pqc.clone(), update=True)),
                     ("step_assign_only_ms", lambda: train_step_dev(x, pqc, update=False)),
                     ("step_assign_only_no_err_ms", lambda: train_step_dev(x, pqc, update=False, want_err=False))):
        ts = []
        for _ in range(6):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            codes = fn()[0]
            torch.cuda.synchronize(dev)
            ts.append((time.perf_counter() - t0) * 1e3)
        out[name] = round(float(np.median(ts[1:])), 3)
    ts = []
    for _ in range(6):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        decode_dev(codes, pqc)
        torch.cuda.synchronize(dev)
        ts.append((time.perf_counter() - t0) * 1e3)
    out["decode_ms"] = round(float(np.median(ts[1:])), 3)
    return out


def run(rows, nlist, M, kind, seed, coarse_iters):
    import torch
    from densephrases_amd import Shard
    from densephrases_amd.pq_train import train_index_resident
    flat = Shard(rows, device=0)
    flat.fill_synthetic(seed=seed, kind=kind)
    flat.finalize()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    index, info = train_index_resident(flat, nlist, M=M, seed=seed, coarse_iters=coarse_iters, return_info=True)
    wall = time.perf_counter() - t0
    flat.close()
    return {"rows": rows, "nlist": nlist, "M": M, "kind": kind, "set_rows": info["set_rows"], "coarse_iters": coarse_iters,
            "wall_s": round(wall, 3), "stage_s": {k: round(v, 3) for k, v in info["seconds"].items()},
            "opq_seconds_per_iter": [round(v, 3) for v in info["opq_seconds_per_iter"]],
            "opq_err": info["opq_err"], "residual_pq_err_first_last": [info["pq_err"][0], info["final_err"]],
            "codewords_split": info["codewords_split"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 22)
    ap.add_argument("--nlist", default="4096,1048576", help="comma list: one configuration each")
    ap.add_argument("--rows_long", type=int, default=1 << 21, help="rows of a configuration with more than 65536 lists")
    ap.add_argument("--coarse_iters_long", type=int, default=2, help="coarse k-means iterations of such a configuration")
    ap.add_argument("--M", type=int, default=96)
    ap.add_argument("--kind", type=int, default=3)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pq_train_timing.json"))
    args = ap.parse_args()
    import torch
    import __graft_entry__ as g
    g.build()
    res = {"tool": "tools/pq_train_timing.py", "device": torch.cuda.get_device_name(0), "box": os.uname().nodename,
           "lloyd_step_65536_rows": time_step(args.M, 65536, args.seed), "configs": []}
    print(json.dumps(res["lloyd_step_65536_rows"]), flush=True)
    for nlist in (int(v) for v in args.nlist.split(",")):
        long_q = nlist > 65536
        res["configs"].append(run(min(args.rows, args.rows_long) if long_q else args.rows, nlist, args.M, args.kind, args.seed,
                                  args.coarse_iters_long if long_q else 10))
        print(json.dumps(res["configs"][-1]), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:                      # (after every configuration: a later one that runs out of time loses nothing)
            json.dump(res, f, indent=1)
    print(json.dumps({"written": args.out}))


if __name__ == "__main__":
    main()
