#!/usr/bin/env python3
"""Per-launch time of the window re-score of a flat raw-dump shard (window_kernel<FlatRows>): HIP events around
Shard.rescore_dev in both directions over a synthetic shard with documents of 100 words, B = 64, k = 10, L = 10, 20 timed
launches per direction after 2 warm-ups.  --build runs the library and package of another checkout over the same inputs
(an A/B against another commit).  Timing only (parity: tests/test_window_direct.py).  Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--build", default=ROOT, help="checkout whose densephrases_amd (and libdph.so) is run")
    ap.add_argument("--rows", type=int, default=8_000_000)
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--L", type=int, default=10)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.build))
    import torch
    from densephrases_amd import Shard
    dev = torch.device("cuda", 0)
    n, doc_len = args.rows - args.rows % 100, 100
    s = Shard(n, device=0)
    s.fill_synthetic()
    ids = np.arange(n, dtype=np.int64)
    s.set_idx2id((ids // doc_len).astype(np.int32), (ids % doc_len).astype(np.int32))
    s.set_f2o(np.arange(n // doc_len, dtype=np.int32), np.arange(0, n + doc_len, doc_len, dtype=np.int64),
              np.tile(np.arange(doc_len, dtype=np.int32), n // doc_len))
    s.finalize()
    rng = np.random.default_rng(3)
    nc = args.B * args.k
    q = torch.from_numpy(rng.normal(0, 0.5, (args.B, 768)).astype(np.float32)).to(dev)
    cand = torch.from_numpy(rng.integers(0, n, nc).astype(np.int64)).to(dev)
    first = torch.from_numpy(rng.normal(50, 5, nc).astype(np.float32)).to(dev)
    pred = torch.empty(nc, dtype=torch.int32, device=dev)
    best = torch.empty(nc, dtype=torch.float64, device=dev)
    arg = torch.empty(nc, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    events = {0: [], 1: []}
    for step in range(args.steps + 2):
        for direction in (0, 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            s.rescore_dev(direction, q.data_ptr(), args.B, args.k, args.L, cand.data_ptr(), 0, 0, first.data_ptr(), pred.data_ptr(),
                          best.data_ptr(), arg.data_ptr(), stream=stream)
            e1.record()
            if step >= 2:                                             # two warm-up rounds are dropped
                events[direction].append((e0, e1))
    torch.cuda.synchronize()
    ms = {d: np.asarray([a.elapsed_time(b) for a, b in ev]) for d, ev in events.items()}
    both = np.concatenate([ms[0], ms[1]])
    out = {"rows": n, "doc_len": doc_len, "B": args.B, "k": args.k, "L": args.L, "steps": args.steps,
           "ms_per_launch": {"launches": int(len(both)), "median": float(np.median(both)), "min": float(both.min()), "max": float(both.max()),
                             "direction_0_median": float(np.median(ms[0])), "direction_1_median": float(np.median(ms[1]))}}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
