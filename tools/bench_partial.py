#!/usr/bin/env python3
"""What partial fine-tuning saves, at bench.py's shapes (ViT-B/32, B = 256, one caption per image, fresh caption tensor and host
lengths every step): ms per ``engine.train_step`` with

  all      every parameter trainable -- bench.py's step (FusedAdam's plain path);
  image    the image tower locked (LiT): a stash-free image forward, no image backward, the update over the text tower only;
  top2     both towers locked except their top 2 blocks: both backwards stop at block L - 2;

each in REPS interleaved rounds of STEPS steps (median, min - max), and the optimiser step alone in tools/bench_hbm.py's manner:
the ungrouped ``ce_adam_step_tiles`` launch against ``ce_adam_step_groups`` with one group over the same tables (cold operands are
not needed here: one call moves 4.8 GB, far more than the Infinity Cache holds), and ``ce_sumsq`` against ``ce_sumsq_segments``.

    python tools/bench_partial.py [--steps 20] [--warmup 5] [--reps 3] [--batch 256]

Prints one JSON line at the end."""
import argparse
import json
import os
import statistics
import sys
import time
from ctypes import c_float, c_int, c_long

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from clip_event_amd import distributed as D, synthetic as S
from clip_event_amd._lib import check, lib, ptr, stream
from clip_event_amd.engine import train_step
from clip_event_amd.functional import attach_lengths, host_lengths
from clip_event_amd.losses import CriterionContrastive
from clip_event_amd.optim import FusedAdam, OptimGroup

DEV = torch.device("cuda", 0)


def make(case):
    model = S.synthetic_model("vit_b32", seed=0).to(DEV)
    if case == "image":
        model.lock_image_tower()
    elif case == "top2":
        model.lock_image_tower(unlocked_layers=2)
        model.lock_text_tower(unlocked_layers=2)
    return model, FusedAdam(model, lr=1e-6, weight_decay=0.0, max_norm=1.0)


def spread(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3)}


def time_calls(fn, iters=10, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3          # us


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--batch", type=int, default=256)
    args = ap.parse_args()
    torch.cuda.set_device(DEV)
    B = args.batch
    crit = CriterionContrastive("ce")
    img = S.synthetic_images(B, 224, seed=999).to(DEV)
    txt_host = S.synthetic_tokens(B, 77, 49408, seed=999)
    txt, lens = txt_host.to(DEV), host_lengths(txt_host)
    yi, yt, ip = D.global_labels(B, 1, 0, True, device=DEV, rank_=0)
    cases = {c: make(c) for c in ("all", "image", "top2")}

    def run(case, n):
        model, opt = cases[case]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            train_step(model, crit, opt, img, attach_lengths(txt.clone(), lens), yi, yt, ip)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3

    for case in cases:
        run(case, args.warmup)
    ms = {c: [] for c in cases}
    for _ in range(args.reps):
        for case in cases:
            ms[case].append(run(case, args.steps))
    out = {"batch": B, "steps": args.steps, "reps": args.reps, "ms_per_step": {c: spread(v) for c, v in ms.items()}}
    for c, v in ms.items():
        print(f"{c:6s} {statistics.median(v):7.3f} ms/step  ({min(v):.3f} - {max(v):.3f})", flush=True)

    # the optimiser step alone: one group over the all-trainable tables, grouped against ungrouped
    model, opt = cases["all"]
    assert model._adam_tiles_ok
    plan = model.trainable_plan({}, tiles=True)
    tj, tn_, tt = model._tjobs_bwd
    seg = model._adam_segment_table()
    ss = torch.ones(1, device=DEV)
    group = (OptimGroup * 1)(OptimGroup(1e-6, 0.0, 0, 0))
    n = model._flat.numel()
    tail = (c_float(0.9), c_float(0.999), c_float(1e-8))

    def ungrouped():
        check(lib().ce_adam_step_tiles(ptr(model._flat), ptr(model._flat_grad), ptr(opt.m), ptr(opt.v), ptr(model._flat16), ptr(tj),
                                       c_int(tn_), c_int(tt), ptr(seg), c_int(seg.shape[0]), ptr(ss), c_float(1.0), c_float(1e-6), *tail,
                                       c_float(0.0), c_int(3), stream()), "ce_adam_step_tiles")

    def grouped():
        pj, pn, pt = plan.tjobs
        check(lib().ce_adam_step_groups(ptr(model._flat), ptr(model._flat_grad), ptr(opt.m), ptr(opt.v), ptr(model._flat16), ptr(pj),
                                        c_int(pn), c_int(pt), ptr(plan.segments), c_int(plan.segments.shape[0]), ptr(plan.segment_group),
                                        ptr(ss), c_float(1.0), group, c_int(1), *tail, c_int(3), stream()), "ce_adam_step_groups")

    def sumsq():
        check(lib().ce_sumsq(ptr(model._flat_grad), c_long(n), ptr(ss), stream()), "ce_sumsq")

    def sumsq_table():
        check(lib().ce_sumsq_segments(ptr(model._flat_grad), ptr(plan.chunks), c_int(plan.chunks.shape[0]), ptr(ss), stream()),
              "ce_sumsq_segments")

    us = {k: [] for k in ("adam_tiles", "adam_groups", "sumsq", "sumsq_segments")}
    for _ in range(args.reps):
        for k, fn in (("adam_tiles", ungrouped), ("adam_groups", grouped), ("sumsq", sumsq), ("sumsq_segments", sumsq_table)):
            us[k].append(time_calls(fn))
    out["optimiser_us"] = {k: spread(v) for k, v in us.items()}
    out["tables"] = {"segments": int(plan.segments.shape[0]), "ungrouped_segments": int(seg.shape[0]), "chunks": int(plan.chunks.shape[0])}
    for k, v in us.items():
        print(f"{k:15s} {statistics.median(v):8.1f} us  ({min(v):.1f} - {max(v):.1f})", flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
