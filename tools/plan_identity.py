#!/usr/bin/env python3
"""Identity of the PLAN between two builds, as the GPU sees it: what the host planning rules (csrc/dph_plan.h) decide -- aux layout, norm
unit, outlier cut, ladder, kp, fused stride, passes, work-queue and PQ capacities -- read back from small shards after real searches,
together with the results.  A stride or a kp that moved shows in the pair / trigger counts and the launch counts even where D and I agree.

    python tools/plan_identity.py --out head.npz [--only flat|lists|pq]             this tree's build
    python tools/plan_identity.py --build /path/to/other/tree --out parent.npz      the library and package of another checkout
    python tools/plan_identity.py --compare parent.npz head.npz [--skip parent_again.npz] --json profiles/plan_refactor_identity.json

One array per case and item.  --compare is exact (np.array_equal, dtype included); --skip names a second run of the FIRST build: an
array that differs between those two is not deterministic, it is listed and left out.  Every --out run is a few seconds per shard; run
each under a time limit of its own."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS, SIZES, AUX, BATCHES, KS = range(5), (8192, 8224, 300_000, 2_000_000), (-1, 0, 4, 16, 32), (64, 200, 300), (10, 100)


class Keeper:
    def __init__(self):
        self.arrays = {}

    def __call__(self, case, **items):
        for name, v in items.items():
            key = f"{case}/{name}"
            assert key not in self.arrays, key
            self.arrays[key] = np.asarray(v)


def _search(torch, s, x, k, nprobe=None):
    n = x.shape[0]
    D = torch.empty((n, k), dtype=torch.float32, device=x.device)
    I = torch.empty((n, k), dtype=torch.int64, device=x.device)
    st = torch.full((n,), -7, dtype=torch.int32, device=x.device)
    if nprobe is None:
        s.search_dev(x.data_ptr(), n, k, D.data_ptr(), I.data_ptr(), st.data_ptr())
    else:
        s.search_ivf_dev(x.data_ptr(), n, k, nprobe, D.data_ptr(), I.data_ptr(), st.data_ptr())
    torch.cuda.synchronize()
    return D.cpu().numpy(), I.cpu().numpy(), st.cpu().numpy()


def _shard_items(s):
    st = s.shard_stats()
    info = s.debug_aux()[2]
    return dict(aux_layout=s.aux_layout(), shard_stats=np.array([st["rmax"], st["rmax_all"], float(st["n_outliers"])]), mu=s.debug_mu(),
                aux_info=np.array([info[k] for k in ("stride", "unit", "q2max", "n_rep")], np.int64))


def _search_items(torch, s, x, k, nprobe=None):
    s.profile_read_all()                                                    # (drop what earlier calls left)
    D, I, status = _search(torch, s, x, k, nprobe)
    stats = s.stats()
    _, full, _, ladder = s.profile_read_all()
    return dict(D=D, I=I, status=status, stats=np.array([stats[f] for f in sorted(stats)], np.int64), launches=np.array([full, ladder], np.int64),
                scan_counters=np.array(s.scan_counters(), np.int64))


def _queries(torch, n, seed):
    x = np.random.default_rng(seed).normal(0, 0.6, (n, 768)).astype(np.float32)
    return torch.from_numpy(x).cuda()


def run_flat(torch, keep):
    from densephrases_amd import Shard
    xs = {b: _queries(torch, b, 100 + b) for b in BATCHES}
    for kind in KINDS:
        for n in SIZES:
            s = Shard(n, device=0)
            s.fill_synthetic(seed=7 + kind, kind=kind)
            s.finalize()
            s.profile_enable(True)
            for mode in AUX:
                s.set_tuning("aux", mode)
                case = f"flat kind{kind} n{n} aux{mode}"
                keep(case, **_shard_items(s))
                for b in BATCHES:
                    for k in KS:
                        keep(f"{case} b{b} k{k}", **_search_items(torch, s, xs[b], k))
            s.close()


def run_lists(torch, keep):
    from densephrases_amd import Shard
    from densephrases_amd import ivf
    for n, nlist in ((2_000_000, 64), (300_000, 4096)):
        s = Shard(n, device=0)
        s.fill_synthetic(seed=21, kind=1)
        s.finalize()
        cent = np.random.default_rng(nlist).normal(0, 0.6, (nlist, 768)).astype(np.float32)
        ivf.make_list_major_resident(s, nlist, centroids=cent)
        s.finalize()
        s.profile_enable(True)
        case = f"lists n{n} nlist{nlist}"
        keep(case, **_shard_items(s))
        for b in (700, 900):
            x = _queries(torch, b, 300 + b)
            for nprobe in (1, 8, 64):
                items = _search_items(torch, s, x, 10, nprobe)
                try:
                    u = s.debug_units()
                    items["units"] = np.array([u[f] for f in ("chunks", "units", "cap_error", "taken_by_full_scan")], np.int64)
                except Exception:                                           # (no unit scan on this shard: the masked scan)
                    items["units"] = np.array([-1], np.int64)
                keep(f"{case} b{b} nprobe{nprobe}", **items)
        s.close()


def run_pq(torch, keep):
    from tests import _pq_build as B
    for M in (48, 96, 128):
        # many short lists (the row-major scan) and a few long ones (the list-major scan: 2048 codes per list and more)
        for name, nlist, n in (("rows", 256, 20_000), ("lists", 4, 12_000)):
            rng = np.random.default_rng(M + nlist)
            cent = rng.normal(0, 0.5, (nlist, 768)).astype(np.float32)
            lists = np.minimum((rng.random(n) ** 2 * nlist).astype(np.int64), nlist - 1)          # skewed list sizes
            ix, _ = B._index_from_list_numbers(rng, nlist, M, lists, cent)
            s = B._shard(ix)
            for b in (64, 300):
                x = _queries(torch, b, 500 + b)
                for k in (1, 10, 200):
                    for nprobe in (1, 16, 64):
                        D, I, status = _search(torch, s, x, k, nprobe)
                        info = s.debug_pq_pass(b)[0]
                        keep(f"pq M{M} {name} b{b} k{k} nprobe{nprobe}", D=D, I=I, status=status,
                             caps=np.array([info[f] for f in ("cand_cap", "unit_cap", "pair_cap", "scratch_rows")], np.int64))
            s.close()


def compare(a_path, b_path, skip_path, json_path):
    a, b = np.load(a_path), np.load(b_path)

    def differ(p, q, n):
        return n not in p.files or n not in q.files or p[n].dtype != q[n].dtype or not np.array_equal(p[n], q[n], equal_nan=True)

    names = sorted(set(a.files) | set(b.files))
    unstable = []
    if skip_path:
        again = np.load(skip_path)
        unstable = [n for n in sorted(set(a.files) | set(again.files)) if differ(a, again, n)]
    compared = [n for n in names if n not in set(unstable)]
    differing = [n for n in compared if differ(a, b, n)]
    items = sorted({n.rsplit("/", 1)[1] for n in names})
    rec = {"cases": len({n.rsplit("/", 1)[0] for n in names}), "items": items, "arrays": len(names), "not_deterministic": unstable,
           "compared": len(compared), "identical": len(compared) - len(differing), "differing": differing}
    print(json.dumps(rec))
    if json_path:
        with open(json_path, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
    return 1 if differing else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--build", default=ROOT, help="checkout whose densephrases_amd (and libdph.so) is run")
    ap.add_argument("--out", default="")
    ap.add_argument("--only", default="", choices=("", "flat", "lists", "pq"))
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    ap.add_argument("--skip", default="", help="a second run of build A: arrays that differ from A are left out")
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare, args.skip, args.json))
    sys.path.insert(0, os.path.abspath(args.build))
    import densephrases_amd                                    # noqa: F401  (the build under test, before this tree's tests / oracle)
    sys.path.insert(1, ROOT)
    import torch
    keep = Keeper()
    for name, fn in (("flat", run_flat), ("lists", run_lists), ("pq", run_pq)):
        if args.only in ("", name):
            fn(torch, keep)
    np.savez(args.out or "plan_identity.npz", **keep.arrays)
    print(json.dumps({"out": args.out, "build": os.path.abspath(args.build), "cases": len({n.rsplit("/", 1)[0] for n in keep.arrays}), "arrays": len(keep.arrays)}))


if __name__ == "__main__":
    main()
