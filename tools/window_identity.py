#!/usr/bin/env python3
"""Identity of the window re-score between two builds: every input set of tests/_window_sets.py and tests/_window_doc_sets.py
(flat, grouped, list-major and range-split raw-dump shards, the PQ variants, the doc-row variants; both directions) through
Shard.rescore(..., want_vecs=True), its four outputs kept in one .npz.

    python tools/window_identity.py --out new.npz                        this tree's build
    python tools/window_identity.py --build /path/to/other/tree --out parent.npz    the library and package of another checkout
    python tools/window_identity.py --compare parent.npz new.npz --json profiles/window_refactor_identity.json

The input sets are always this tree's; --compare holds the files together array by array with np.array_equal."""
import argparse
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUTPUTS = ("pred_word", "best", "argslot", "vecs")


def run(out):
    from tests import _window_doc_sets as D
    from tests import _window_sets as S
    from tests.test_window_direct import _pq_shard, _raw_shard
    from tests.test_window_doc_direct import _shard as _doc_shard
    arrays = {}

    def keep(name, s, b):
        got = s.rescore(b.direction, b.q, b.k, b.L, b.ids, b.doc, b.word, b.first, want_vecs=True)
        assert name + "/best" not in arrays, name
        for key, a in zip(OUTPUTS, got):
            arrays[f"{name}/{key}"] = np.asarray(a)

    for name, b, _, _ in S.raw_sets():
        cut = re.match(r"cut \[(\d+),(\d+)\)", name)
        kind = "groups" if name.startswith("groups") else "lists" if name.startswith("lists") else "flat"
        keep(name, _raw_shard(kind, b.L, *(map(int, cut.groups()) if cut else ())), b)
    for variant in S.PQ_VARIANTS:
        for name, b, _, _ in S.pq_sets(variant):
            keep(name, _pq_shard(variant), b)
            if variant == "m64_offset":
                keep(name + " +groups", _pq_shard(variant, True), b)
    for variant in D.VARIANTS:
        for name, _, b in D.sets(variant):
            keep(name, _doc_shard(variant, b.L), b)
    np.savez(out, **arrays)
    print(json.dumps({"out": out, "sets": len(arrays) // len(OUTPUTS), "arrays": len(arrays)}))


def compare(a_path, b_path, json_path):
    a, b = np.load(a_path), np.load(b_path)
    names = sorted(set(a.files) | set(b.files))
    differing = [n for n in names if n not in a.files or n not in b.files or a[n].dtype != b[n].dtype or not np.array_equal(a[n], b[n])]
    sets = sorted({n.rsplit("/", 1)[0] for n in names})
    rec = {"sets": sets, "n_sets": len(sets), "arrays": len(names), "identical": len(names) - len(differing), "differing": differing}
    print(json.dumps({k: v for k, v in rec.items() if k != "sets"}))
    if json_path:
        with open(json_path, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
    return 1 if differing else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--build", default=ROOT, help="checkout whose densephrases_amd (and libdph.so) is run")
    ap.add_argument("--out", default="")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare, args.json))
    sys.path.insert(0, os.path.abspath(args.build))
    import densephrases_amd                                    # noqa: F401  (the build under test, before this tree's tests / oracle)
    sys.path.insert(0, ROOT)
    run(args.out or "window_identity.npz")


if __name__ == "__main__":
    main()
