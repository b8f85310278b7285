#!/usr/bin/env python3
"""What low-rank adapters cost and save (CLIP.enable_lora).

  kernels  ``ce_lora_merge`` and ``ce_lora_grad`` over every block matrix of ViT-B/32 and ViT-L/14 at rank 8 / 16 / 64, against
           ``ce_adam_step_tiles`` over the same model in the same run, in tools/bench_hbm.py's manner (the passes move hundreds
           of MB to GB per call, far more than the Infinity Cache holds: no cold-operand rotation is needed).  Merge + grad move
           about 12 bytes per adapted element plus the partial sums, the update 30: together they must stay below it.
  step     ms per ``engine.train_step`` at bench.py's shapes (ViT-B/32, B = 256) with everything trainable, with both towers
           locked except their top 2 blocks, and with rank-16 adapters on every block matrix -- REPS interleaved rounds of STEPS
           steps (median, min - max), as tools/bench_partial.py does.
  bytes    trainable parameters, optimiser state (Adam: 8 B per trainable parameter) and the per-task checkpoint.

    python tools/bench_lora.py [--steps 20] [--warmup 5] [--reps 3] [--batch 256] [--skip-large]

Prints one JSON line at the end."""
import argparse
import json
import os
import statistics
import sys
import time
from ctypes import c_float, c_int

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from clip_event_amd import distributed as D, synthetic as S
from clip_event_amd._lib import check, lib, ptr, stream
from clip_event_amd.engine import train_step
from clip_event_amd.functional import attach_lengths, host_lengths
from clip_event_amd.losses import CriterionContrastive
from clip_event_amd.optim import FusedAdam

DEV = torch.device("cuda", 0)
RANKS = (8, 16, 64)


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


def kernels(geometry, reps):
    """us per call of merge, grad and the tiled Adam step on one model of ``geometry``."""
    out = {}
    model = S.synthetic_model(geometry, seed=0).to(DEV)
    opt = FusedAdam(model, lr=1e-6, weight_decay=0.0, max_norm=1.0)
    opt._state()
    assert model._adam_tiles_ok
    tj, tn_, tt = model._tjobs_bwd
    seg = model._adam_segment_table()
    ss = torch.ones(1, device=DEV)

    def adam():
        check(lib().ce_adam_step_tiles(ptr(model._flat), ptr(model._flat_grad), ptr(opt.m), ptr(opt.v), ptr(model._flat16), ptr(tj),
                                       c_int(tn_), c_int(tt), ptr(seg), c_int(seg.shape[0]), ptr(ss), c_float(1.0), c_float(1e-6),
                                       c_float(0.9), c_float(0.999), c_float(1e-8), c_float(0.0), c_int(3), stream()), "ce_adam_step_tiles")

    adam_us = [time_calls(adam) for _ in range(reps)]
    del opt
    for r in RANKS:
        model.enable_lora(rank=r, alpha=2.0 * r)
        model._ready()
        model._flat_grad.normal_()
        host, dev, n, tiles, strips, ws_bytes = model._lora_tab
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
        adapted = sum(model._pmap[e[0]].numel() for e in model._lora["entries"])

        def merge():
            check(lib().ce_lora_merge(host, ptr(dev), n, tiles, 0, stream()), "ce_lora_merge")

        def grad():
            check(lib().ce_lora_grad(host, ptr(dev), n, strips, ptr(ws), ws_bytes, stream()), "ce_lora_grad")

        us = {"merge": [], "grad": [], "adam_tiles": adam_us}
        for _ in range(reps):
            us["merge"].append(time_calls(merge))
            us["grad"].append(time_calls(grad))
        row = {k: spread(v) for k, v in us.items()}
        row.update(adapted_elements=adapted, workspace_bytes=ws_bytes, matrices=n,
                   merge_plus_grad_over_adam=round((statistics.median(us["merge"]) + statistics.median(us["grad"])) /
                                                   statistics.median(adam_us), 3))
        out[f"r{r}"] = row
        print(f"{geometry:12s} r={r:2d}: merge {row['merge']['median']:8.1f} us, grad {row['grad']['median']:8.1f} us, adam_tiles "
              f"{row['adam_tiles']['median']:8.1f} us  ((merge + grad) / adam {row['merge_plus_grad_over_adam']:.3f}; workspace "
              f"{ws_bytes / 2**20:.1f} MiB)", flush=True)
        del ws
        model.merge_lora()                    # a plain model again for the next rank
    return out


def make(case):
    model = S.synthetic_model("vit_b32", seed=0).to(DEV)
    if case == "top2":
        model.lock_image_tower(unlocked_layers=2)
        model.lock_text_tower(unlocked_layers=2)
    elif case == "lora":
        model.enable_lora(rank=16, alpha=32.0)
    return model, FusedAdam(model, lr=1e-6, weight_decay=0.0, max_norm=1.0)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--skip-large", action="store_true", help="leave ViT-L/14 out of the kernel timings")
    args = ap.parse_args()
    torch.cuda.set_device(DEV)
    out = {"kernels_us": {}}
    for geometry in ("vit_b32",) + (() if args.skip_large else ("vit_l14_336",)):
        out["kernels_us"][geometry] = kernels(geometry, args.reps)
        torch.cuda.empty_cache()

    B = args.batch
    crit = CriterionContrastive("ce")
    img = S.synthetic_images(B, 224, seed=999).to(DEV)
    txt_host = S.synthetic_tokens(B, 77, 49408, seed=999)
    txt, lens = txt_host.to(DEV), host_lengths(txt_host)
    yi, yt, ip = D.global_labels(B, 1, 0, True, device=DEV, rank_=0)
    cases = {c: make(c) for c in ("all", "top2", "lora")}

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
    out.update(batch=B, steps=args.steps, reps=args.reps, ms_per_step={c: spread(v) for c, v in ms.items()})
    for c, v in ms.items():
        print(f"{c:6s} {statistics.median(v):7.3f} ms/step  ({min(v):.3f} - {max(v):.3f})", flush=True)
    out["bytes"] = {}
    for c, (model, _) in cases.items():
        trainable = sum(p.numel() for p in model.parameters() if p.requires_grad)
        ckpt = sum(v.numel() * 4 for v in (model.lora_state_dict()["state"] if c == "lora" else model.state_dict()).values())
        # (FusedAdam itself keeps its two moments as flat buffers over the WHOLE layout, addressed by the parameters' offsets:
        #  "adam_state" is what the trainable parameters need -- and what the checkpoint's optimiser entry holds --, "fused_adam_state"
        #  what the fused step allocates today)
        out["bytes"][c] = {"trainable_parameters": trainable, "adam_state": 8 * trainable, "fused_adam_state": 8 * model._flat.numel(),
                           "task_checkpoint": ckpt}
        print(f"{c:6s} {trainable:11d} trainable parameters, Adam state {8 * trainable / 2**20:8.1f} MiB, per-task checkpoint "
              f"{ckpt / 2**20:7.1f} MiB", flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
