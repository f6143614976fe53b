#!/usr/bin/env python3
"""Per-launch time of the two window kernels of a PQ index at full size: window_kernel<PqCodes> (windows of reconstructions, the
reference's RAM branch) on a handle without rows, and window_kernel<DocRows> (the dump's raw int8 rows, the HDF5 branch) on a
handle with the rows of every document attached -- the same synthetic 170 M-code index of tools/pq_timing.py, documents of
100 words, B = 64, k = 10, L = 10, both directions, launches interleaved, read from the PQ profiler's event pairs
(dph_profile_read_each, which = 3).  The JSON keys keep the labels the two instantiations had as kernels of their own,
"pq_window_kernel" and "pq_window_doc_kernel", so that earlier records compare.  Timing only (parity: tests/test_window_doc_direct.py).  Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--codes", type=int, default=170_000_000)
    ap.add_argument("--nlist", type=int, default=4096)
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--L", type=int, default=10)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    import __graft_entry__ as g
    g.build()
    from densephrases_amd.synth import synthetic_pq_shard
    dev = torch.device("cuda", 0)
    n, doc_len = args.codes - args.codes % 100, 100
    plain = synthetic_pq_shard(n, args.nlist, 96, device=0, doc_len=doc_len)[0]
    rows = synthetic_pq_shard(n, args.nlist, 96, device=0, doc_len=doc_len, doc_rows=True)[0]
    torch.cuda.synchronize()
    rng = np.random.default_rng(3)
    # MIPS.search re-scores B * k candidates per direction
    q = torch.from_numpy(rng.normal(0, 0.5, (args.B, 768)).astype(np.float32)).to(dev)
    ids = torch.from_numpy(rng.integers(0, n, args.B * args.k).astype(np.int64)).to(dev)
    first = torch.from_numpy(rng.normal(50, 5, args.B * args.k).astype(np.float32)).to(dev)
    pred = torch.empty(args.B * args.k, dtype=torch.int32, device=dev)
    best = torch.empty(args.B * args.k, dtype=torch.float64, device=dev)
    arg = torch.empty(args.B * args.k, dtype=torch.int32, device=dev)
    out = {"codes": n, "doc_len": doc_len, "B": args.B, "k": args.k, "L": args.L, "steps": args.steps,
           "doc_row_bytes": n * 768, "gather_bytes_per_launch": args.B * args.k * args.L * 768, "ms_per_launch": {}}
    for s in (plain, rows):
        s.profile_enable(3)
    for step in range(args.steps + 2):
        for direction in (0, 1):
            for s in (plain, rows):                                   # interleaved: same clocks, same neighbours
                s.rescore_dev(direction, q.data_ptr(), args.B, args.k, args.L, ids.data_ptr(), 0, 0, first.data_ptr(), pred.data_ptr(),
                              best.data_ptr(), arg.data_ptr())
        if step == 1:                                                 # two warm-up rounds are dropped
            torch.cuda.synchronize()
            for s in (plain, rows):
                s.profile_read_each(3)
    torch.cuda.synchronize()
    for name, s in (("pq_window_kernel", plain), ("pq_window_doc_kernel", rows)):
        ms = s.profile_read_each(3)
        out["ms_per_launch"][name] = {"launches": int(len(ms)), "median": float(np.median(ms)), "min": float(ms.min()), "max": float(ms.max()),
                                      "direction_0_median": float(np.median(ms[0::2])), "direction_1_median": float(np.median(ms[1::2]))}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
