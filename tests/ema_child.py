#!/usr/bin/env python3
"""The weight EMA on the FLAT optimiser path (started by tests/test_ema_gpu.py with CE_ADAM_TILES=0): FusedAdam with and
without ``enable_ema`` over the same four steps must leave the same bits (tests.test_ema_gpu.feedback_check).  Prints ONE JSON
verdict line; exit status 0 only if nothing differed.

    CE_ADAM_TILES=0 python tests/ema_child.py
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    from tests.test_ema_gpu import feedback_check
    tiles = os.environ.get("CE_ADAM_TILES", "1")
    ok, bad = feedback_check("adam", tiles_expected=tiles != "0")
    print(json.dumps({"env": tiles, "ok": ok, "failed": bad}), flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
