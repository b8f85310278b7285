#!/usr/bin/env python3
"""One environment form of the LayerNorm launchers (started by tests/test_layernorm_ops.py with CE_LN_FWD_RPW or
CE_LN_BWD_BLOCKS set: the launchers read them once per process).  Runs tests/ln_cases.py's CHILD_CASES against fp64, the
partials buffers sized from ``ce_layernorm_bwd_blocks`` under the same environment, logs one line per launch to stderr and
prints ONE JSON verdict line; exit status 0 only if every launch passed.

    CE_LN_BWD_BLOCKS=3 python tests/ln_child.py
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    from clip_event_amd._lib import lib
    from tests.ln_cases import CHILD_CASES, bwd_blocks, run_case
    t0 = time.time()
    recs = []
    for case in CHILD_CASES:
        recs += run_case(case, seed=1, log=lambda s: print(s, file=sys.stderr, flush=True))
    failed = [r for r in recs if not r["ok"]]
    env = {k: v for k, v in os.environ.items() if k.startswith("CE_LN_")}
    blocks = {f"{c.M}x{c.D}": lib().ce_layernorm_bwd_blocks(c.M, c.D) for c in CHILD_CASES}
    blocks_ok = all(n == bwd_blocks(c.M, c.D) for n, c in zip(blocks.values(), CHILD_CASES))
    ok = not failed and bool(recs) and blocks_ok
    print(json.dumps({"env": env, "ok": ok, "launches": len(recs), "blocks": blocks, "blocks_ok": blocks_ok,
                      "worst": max([max(r["worst"].values() or [0.0]) for r in recs] or [0.0]), "seconds": time.time() - t0,
                      "failed": failed}), flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
