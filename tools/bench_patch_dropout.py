#!/usr/bin/env python3
"""Time and memory of the train step with patch dropout (CLIP.set_patch_dropout) beside the same step with the feature
off, on one GPU.  bench.py stays the flagship measurement (it never drops); this tool answers what the image tower's
shorter sequence buys.

    python tools/bench_patch_dropout.py                         # ViT-B/32, B = 256, p = 0, 0.25, 0.5, 0.75
    python tools/bench_patch_dropout.py --arch vit_l14_336      # ViT-L/14@336, B = 32, p = 0, 0.5

One JSON line per rate on stdout: ``arch``, ``batch``, ``patch_dropout``, ``keep`` / ``patches``, ``ms_per_step`` (HIP
events around the timed steps, after the warm-up; a new caption tensor with host-side lengths every step),
``peak_allocated_bytes`` (torch.cuda.max_memory_allocated over the timed steps), ``allocated_before_bytes`` and, for p > 0,
``ms_ratio`` / ``peak_ratio`` against the p = 0 line of the SAME process -- the feature switched off, never another rate.

All rates are measured in one child process (every rate builds a fresh model: the workspace pool keeps its buffers), and
this process, which never opens the GPU, gives every rate its own time limit (``--case-timeout`` seconds from one result
line to the next): a child that overruns it is killed and nothing further is started."""
import argparse
import gc
import json
import os
import queue
import subprocess
import sys
import threading

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEFAULTS = {"vit_b32": (256, [0.0, 0.25, 0.5, 0.75]), "vit_l14_336": (32, [0.0, 0.5])}


def parse():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--arch", default="vit_b32", choices=sorted(DEFAULTS))
    ap.add_argument("--batch", type=int, default=None, help="images per step (default: 256 for vit_b32, 32 for vit_l14_336)")
    ap.add_argument("--rates", type=float, nargs="*", default=None, help="dropout rates; 0 is always measured first")
    ap.add_argument("--fp8", type=int, nargs="?", const=3, default=0)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--case-timeout", type=float, default=240.0, help="seconds one rate may take before the child is killed")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    batch, rates = DEFAULTS[args.arch]
    args.batch = batch if args.batch is None else args.batch
    args.rates = [0.0] + [p for p in (rates if args.rates is None else args.rates) if p != 0.0]
    return args


def run_case(args, p, dev):
    import torch
    from clip_event_amd import distributed as D, synthetic as S
    from clip_event_amd.engine import train_step
    from clip_event_amd.functional import attach_lengths, host_lengths
    from clip_event_amd.losses import CriterionContrastive
    from clip_event_amd.optim import FusedAdam
    B = args.batch
    model = S.synthetic_model(args.arch, seed=0).to(dev)
    model.fp8 = int(args.fp8)
    model.set_patch_dropout(p, seed=0)
    crit = CriterionContrastive("ce")
    opt = FusedAdam(model, lr=1e-6, weight_decay=0.0, max_norm=1.0)
    img = S.synthetic_images(B, model.visual.input_resolution, seed=999).to(dev)
    txt_host = S.synthetic_tokens(B, 77, 49408, seed=999)
    txt = txt_host.to(dev)
    lens = host_lengths(txt_host)
    yi, yt, ip = D.global_labels(B, 1, 0, True, device=dev, rank_=0)

    def step():
        return train_step(model, crit, opt, img, attach_lengths(txt.clone(), lens), yi, yt, ip)

    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.steps):
        out = step()
    e1.record()
    torch.cuda.synchronize()
    row = {"arch": args.arch, "batch": B, "patch_dropout": p, "keep": model.visual.patch_keep(),
           "patches": model.visual.patch_num ** 2, "fp8": int(args.fp8), "stream16": bool(model.stream16), "steps": args.steps,
           "warmup": args.warmup, "ms_per_step": round(e0.elapsed_time(e1) / args.steps, 3),
           "peak_allocated_bytes": int(torch.cuda.max_memory_allocated(dev)), "allocated_before_bytes": int(before),
           "loss": round(float(sum(v.detach() for v in out.values())), 5)}
    del model, opt, out
    gc.collect()
    torch.cuda.empty_cache()
    return row


def child(args):
    import torch
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    base = None
    for p in args.rates:
        row = run_case(args, p, dev)
        if p == 0.0:
            base = row
        else:
            row["ms_ratio"] = round(row["ms_per_step"] / base["ms_per_step"], 4)
            row["peak_ratio"] = round(row["peak_allocated_bytes"] / base["peak_allocated_bytes"], 4)
        print(json.dumps(row), flush=True)


def main():
    args = parse()
    if args.child:
        return child(args)
    cmd = [sys.executable, os.path.abspath(__file__), "--child"] + sys.argv[1:]
    proc = subprocess.Popen(cmd, stdout=subprocess.PIPE, text=True)
    lines = queue.Queue()
    threading.Thread(target=lambda: [lines.put(ln) for ln in proc.stdout] + [lines.put(None)], daemon=True).start()
    for p in args.rates:
        try:
            ln = lines.get(timeout=args.case_timeout)
        except queue.Empty:
            proc.kill()
            proc.wait()
            sys.exit(f"patch_dropout={p}: no result within {args.case_timeout:.0f} s; child killed, nothing further started")
        if ln is None:
            sys.exit(f"patch_dropout={p}: the measuring process ended with status {proc.wait()} before its result")
        print(ln, end="", flush=True)
    sys.exit(proc.wait())


if __name__ == "__main__":
    main()
