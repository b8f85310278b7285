#!/usr/bin/env python3
"""Time and memory of the micro-batched train step (engine.train_step(micro_batch=n)) beside the unchunked step, and of the
``no_grad`` forward, on one GPU.  bench.py stays the flagship measurement; this tool answers what bench.py cannot ask:
what a batch that does not fit costs when it is cut into chunks.

    python tools/bench_micro_batch.py --arch vit_b32 --batch 256 --micro-batch 0 128 64 --no-grad-forward
    python tools/bench_micro_batch.py --arch vit_l14_336 --batch 1024 --micro-batch auto [--fp8]

One JSON line per case on stdout: ``arch``, ``batch``, ``micro_batch`` (null: unchunked), ``ms_per_step`` (HIP events around
the timed steps, after the warm-up; every step gets a NEW caption tensor with host-side lengths, as a data loader yields
it), ``peak_allocated_bytes`` (torch.cuda.max_memory_allocated over the timed steps) and ``allocated_before_bytes`` (model,
optimiser state, inputs), ``stash_bytes`` (the two towers' training workspaces at the chunk size), ``pairs_per_s`` and
``tflops`` under the FLOP model of bench.py with the second forward counted: a chunked step runs forward, forward,
backward = 4/3 of the unchunked step's tower FLOPs; the ``no_grad`` forward is 1/3 of them.

``--micro-batch 0`` is the unchunked step (it passes no ``micro_batch`` argument, so the same file also runs against a
checkout that predates the argument); ``auto`` picks the largest multiple of 32 whose stash takes at most ``--fit`` of
the memory that is free once the model, the optimiser state and the inputs are in place.  Every case builds a fresh
model: the workspace pool keeps its buffers."""
import argparse
import ctypes
import gc
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

# nominal fwd+bwd FLOP per pair at K = 1 and the text tower's share per caption: bench.py's table
ARCH = {
    "vit_b32": (44.10e9, 3 * 2 * 2.9798e9),
    "vit_b16": (3 * 2 * (17.58e9 + 2.9798e9), 3 * 2 * 2.9798e9),
    "vit_l14_336": (1185.7e9, (1345.3e9 - 1185.7e9) / 4),
}


def parse():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--arch", default="vit_b32", choices=sorted(ARCH))
    ap.add_argument("--batch", type=int, default=256, help="images per step on this GPU")
    ap.add_argument("--descriptions", type=int, default=1, help="captions per image (K)")
    ap.add_argument("--micro-batch", nargs="*", default=["0"], help="chunk sizes to time: 0 = unchunked, auto = the largest that fits")
    ap.add_argument("--no-grad-forward", action="store_true", help="also time encode_both under torch.no_grad()")
    ap.add_argument("--fp8", type=int, nargs="?", const=3, default=0)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--fit", type=float, default=0.75, help="auto: share of the free memory the stash may take")
    return ap.parse_args()


def stash_bytes(model, images: int, captions: int) -> int:
    from clip_event_amd._lib import lib
    fn = lib().ce_tower_workspace_bytes
    fn.restype = ctypes.c_size_t
    return int(fn(ctypes.byref(model._vdesc), ctypes.c_int(images))) + int(fn(ctypes.byref(model._tdesc), ctypes.c_int(captions)))


def run_case(args, what, dev):
    from clip_event_amd import distributed as D, synthetic as S
    from clip_event_amd.engine import train_step
    from clip_event_amd.functional import attach_lengths, host_lengths
    from clip_event_amd.losses import CriterionContrastive
    from clip_event_amd.optim import FusedAdam
    B, K = args.batch, max(1, args.descriptions)
    model = S.synthetic_model(args.arch, seed=0).to(dev)
    model.fp8 = int(args.fp8)
    crit = CriterionContrastive("ce")
    opt = FusedAdam(model, lr=1e-6, weight_decay=0.0, max_norm=1.0)
    img = S.synthetic_images(B, model.visual.input_resolution, seed=999).to(dev)
    txt_host = S.synthetic_tokens(B * K, 77, 49408, seed=999)
    txt = txt_host.to(dev)
    lens = host_lengths(txt_host)
    yi, yt, ip = D.global_labels(B, 1, K - 1, True, device=dev, rank_=0)
    model._ready()
    torch.cuda.synchronize()
    mb = None
    if what == "auto":
        free, _ = torch.cuda.mem_get_info(dev)
        mb = 32
        while mb + 32 < B and stash_bytes(model, mb + 32, (mb + 32) * K) <= args.fit * free:
            mb += 32
    elif what not in ("0", "no_grad"):
        mb = int(what)
    kw = {} if mb is None else {"micro_batch": mb}

    def step():
        t = attach_lengths(txt.clone(), lens)                # a new caption tensor every step
        if what == "no_grad":
            with torch.no_grad():
                return model.encode_both(img, t)
        return train_step(model, crit, opt, img, t, yi, yt, ip, **kw)

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
    ms = e0.elapsed_time(e1) / args.steps
    peak = torch.cuda.max_memory_allocated(dev)
    flop_pair, flop_text = ARCH[args.arch]
    flops = B * (flop_pair + (K - 1) * flop_text)            # the unchunked step's nominal fwd + bwd
    passes = 1.0 / 3.0 if what == "no_grad" else (4.0 / 3.0 if mb is not None and mb < B else 1.0)
    row = {"case": "no_grad_forward" if what == "no_grad" else "train_step", "arch": args.arch, "batch": B, "descriptions": K,
           "micro_batch": mb, "fp8": int(args.fp8), "stream16": bool(model.stream16), "steps": args.steps, "warmup": args.warmup,
           "ms_per_step": round(ms, 3), "pairs_per_s": round(B / (ms * 1e-3), 2),
           "peak_allocated_bytes": int(peak), "allocated_before_bytes": int(before),
           "stash_bytes": None if what == "no_grad" else stash_bytes(model, min(mb or B, B), min(mb or B, B) * K),
           "flop_model": {"unchunked_step_flops": flops, "tower_passes_vs_unchunked": round(passes, 4)},
           "tflops": round(flops * passes / (ms * 1e-3) / 1e12, 2)}
    if what != "no_grad":
        row["loss"] = round(float(sum(v.detach() for v in out.values())), 5)
    del model, opt, out
    gc.collect()
    torch.cuda.empty_cache()
    return row


def main():
    args = parse()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    cases = list(args.micro_batch) + (["no_grad"] if args.no_grad_forward else [])
    for what in cases:
        print(json.dumps(run_case(args, what, dev)), flush=True)


if __name__ == "__main__":
    main()
