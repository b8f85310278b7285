#!/usr/bin/env python3
"""One environment form of the NT GEMM launcher (started by tests/test_nt_ops.py with CE_NT_* / CE_GEMM_CUS set: the launcher
reads them once per process).  Runs tests/nt_cases.py's CHILD_CASES against fp64, each launch held to the plan
``ce_gemm_nt_plan`` reports under the same environment, logs one line per launch to stderr and prints ONE JSON verdict line;
exit status 0 only if every launch passed.

    CE_NT_PGRID=24 CE_NT_CHUNK=2 python tests/nt_child.py
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    from tests.nt_cases import CHILD_CASES, run_case
    t0 = time.time()
    recs = []
    for case in CHILD_CASES:
        recs += run_case(case, seed=1, log=lambda s: print(s, file=sys.stderr, flush=True))
    failed = [r for r in recs if not r["ok"]]
    env = {k: v for k, v in os.environ.items() if k == "CE_GEMM_CUS" or k.startswith("CE_NT_")}
    forms = sorted({f"{r['form'][0]} {r['form'][1]}/{r['form'][2]}" + (" queue" if r["queue"] else "") for r in recs})
    print(json.dumps({"env": env, "ok": not failed and bool(recs), "launches": len(recs), "forms": forms,
                      "worst": max([r["worst"] for r in recs] or [0.0]), "seconds": time.time() - t0, "failed": failed}), flush=True)
    return 0 if not failed and recs else 1


if __name__ == "__main__":
    sys.exit(main())
