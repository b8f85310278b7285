#!/usr/bin/env python3
"""One environment form of the grouped weight-gradient GEMM (started by tests/test_wgrad_ops.py with CE_GEMM_TN or a
CE_TN3_* variable set: the launcher reads them once per process).  Runs tests/wgrad_cases.py's CHILD_CASES against fp64,
logs one line per launch to stderr and prints ONE JSON verdict line; exit status 0 only if every launch passed.

    CE_TN3_LW=0 python tests/wgrad_child.py
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    from tests.wgrad_cases import CHILD_CASES, run_case
    recs = []
    for case in CHILD_CASES:
        recs += run_case(case, seed=1, log=lambda s: print(s, file=sys.stderr, flush=True))
    failed = [r for r in recs if not r["ok"]]
    env = {k: v for k, v in os.environ.items() if k == "CE_GEMM_TN" or k.startswith("CE_TN3_")}
    print(json.dumps({"env": env, "ok": not failed and bool(recs), "launches": len(recs),
                      "kernels": sorted({r["kernel"] for r in recs}), "failed": failed}), flush=True)
    return 0 if not failed and recs else 1


if __name__ == "__main__":
    sys.exit(main())
