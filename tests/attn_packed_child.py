#!/usr/bin/env python3
"""One environment form of the packed long attention kernels (started by tests/test_attention_packed_long_ops.py with
CE_ATTN_NS_FWD, CE_ATTN_NS, CE_ATTN_NK or CE_ATTN_XCD set: the launcher reads them once per process).  Runs that module's
CHILD_CASES against fp64, logs every case's figures to stderr and prints ONE JSON verdict line; exit status 0 only if every case
passed.

    CE_ATTN_NK=2 python tests/attn_packed_child.py
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    from tests.attn_cases import summarise
    from tests.test_attention_packed_long_ops import CHILD_CASES, run_packed
    recs = [run_packed(case, log=lambda s: print(s, file=sys.stderr, flush=True))[0] for case in CHILD_CASES]
    failed = [r for r in recs if not r["ok"]]
    env = {k: v for k, v in os.environ.items() if k.startswith("CE_ATTN_")}
    print(json.dumps({"env": env, "ok": not failed and bool(recs), "cases": len(recs), "figures": summarise(recs),
                      "failed": failed}), flush=True)
    return 0 if not failed and recs else 1


if __name__ == "__main__":
    sys.exit(main())
