#!/usr/bin/env python3
"""Write tests/golden/plan_rules.json: every host planning rule of densephrases_amd/csrc/dph_plan.h over the fixed grid of
tests/_plan.py (`table()`), computed through tests/_plan_shim.cpp.  No GPU.  tests/test_plan.py recomputes the grid and compares it
exactly, so the file is re-recorded only when a rule is MEANT to change -- never to make that test pass.

    python tools/make_golden_plan.py            write the table
    python tools/make_golden_plan.py --check    compare instead (exit 1 on a difference)"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    from tests import _plan as P
    table = json.loads(json.dumps(P.table()))
    if args.check:
        with open(P.GOLDEN) as f:
            have = json.load(f)
        bad = sorted(k for k in set(table) | set(have) if table.get(k) != have.get(k))
        print(json.dumps({"sections": len(table), "differing": bad}))
        sys.exit(1 if bad else 0)
    with open(P.GOLDEN, "w") as f:
        f.write("{\n" + ",\n".join(json.dumps(k) + ": " + json.dumps(v, separators=(",", ":")) for k, v in table.items()) + "\n}\n")
    print(json.dumps({"out": os.path.relpath(P.GOLDEN, ROOT), "sections": len(table), "bytes": os.path.getsize(P.GOLDEN)}))


if __name__ == "__main__":
    main()
