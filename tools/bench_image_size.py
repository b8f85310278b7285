#!/usr/bin/env python3
"""Time of the train step with the image tower at other resolutions (CLIP.set_image_size), and of the two resampling kernels
alone, on one GPU.  bench.py stays the flagship measurement (it runs at the native size, where the feature launches nothing).

    python tools/bench_image_size.py                          # ViT-B/32, B = 256: 128 160 224 288 352 448 px (multiples of 32)
    python tools/bench_image_size.py --arch vit_l14_336       # ViT-L/14, B = 32: 126 154 224 294 336 448 px (multiples of 14)
    python tools/bench_image_size.py --kernels                # ce_pos_resample_fwd / _bwd alone against their byte floor

One JSON line per size on stdout: ``arch``, ``batch``, ``image_size``, ``tokens``, ``ms_per_step`` = the median of ``--repeats``
windows of ``--steps`` steps each (HIP events around every window, after ``--warmup`` steps at that size; a new caption tensor
with host-side lengths every step), ``ms_min`` / ``ms_max`` over the windows, ``pairs_per_s``, and against the 224 px line of
the same run ``ms_ratio`` beside ``token_ratio``.  ``--kernels``: one line per (direction, grids, width): ``us_per_launch``
= the median of ``--repeats`` windows of 200 back-to-back launches, ``bytes`` the kernel must move, ``floor_us`` = bytes /
6.4 TB/s.

Every case runs in a child process of its own, one after the other: measured in one process, a size's step time depended on its
place in the list.  This process never opens the GPU and gives every child ``--case-timeout`` seconds: a child that
overruns it is killed, and after a child that failed nothing further is started."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# multiples of the patch size nearest to 128 / 160 / 224 / 288 / 336 / 448
DEFAULTS = {"vit_b32": (256, [128, 160, 224, 288, 352, 448]), "vit_l14_336": (32, [126, 154, 224, 294, 336, 448])}
BASE = 224
HBM_BYTES_PER_S = 6.4e12
# (native grid, run grid, width): ViT-B/32 at 448 px, ViT-B/16 at 448 px, ViT-L/14@336 at 448 and at 224 px
KERNEL_CASES = [(7, 14, 768), (14, 28, 768), (24, 32, 1024), (24, 16, 1024)]
LAUNCHES = 200


def parse():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--arch", default="vit_b32", choices=sorted(DEFAULTS))
    ap.add_argument("--batch", type=int, default=None, help="images per step (default: 256 for vit_b32, 32 for vit_l14_336)")
    ap.add_argument("--sizes", type=int, nargs="*", default=None, help="image sizes; 224 is always measured first")
    ap.add_argument("--kernels", action="store_true", help="time the two resampling kernels alone instead of the step")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5, help="timed windows per case; the median is reported")
    ap.add_argument("--case-timeout", type=float, default=240.0, help="seconds one case may take before the child is killed")
    ap.add_argument("--case", type=int, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    batch, sizes = DEFAULTS[args.arch]
    args.batch = batch if args.batch is None else args.batch
    args.sizes = [BASE] + [s for s in (sizes if args.sizes is None else args.sizes) if s != BASE]
    return args


def _windows(torch, fn, n, repeats):
    """Milliseconds of ``repeats`` windows of ``n`` calls of ``fn`` each (HIP events; one synchronise per window)."""
    out = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def run_size(args, size, dev):
    import torch
    from clip_event_amd import distributed as D, synthetic as S
    from clip_event_amd.engine import train_step
    from clip_event_amd.functional import attach_lengths, host_lengths
    from clip_event_amd.losses import CriterionContrastive
    from clip_event_amd.optim import FusedAdam
    B = args.batch
    model = S.synthetic_model(args.arch, seed=0).to(dev)
    model.set_image_size(size)
    crit = CriterionContrastive("ce")
    opt = FusedAdam(model, lr=1e-6, weight_decay=0.0, max_norm=1.0)
    img = S.synthetic_images(B, size, seed=999).to(dev)
    txt_host = S.synthetic_tokens(B, 77, 49408, seed=999)
    txt = txt_host.to(dev)
    lens = host_lengths(txt_host)
    yi, yt, ip = D.global_labels(B, 1, 0, True, device=dev, rank_=0)
    out = {}

    def step():
        out["ld"] = train_step(model, crit, opt, img, attach_lengths(txt.clone(), lens), yi, yt, ip)

    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    ms = [w / args.steps for w in _windows(torch, step, args.steps, args.repeats)]
    med = statistics.median(ms)
    row = {"arch": args.arch, "batch": B, "image_size": size, "native_size": int(model.visual.native_resolution),
           "tokens": model.visual.patch_num ** 2 + 1, "stream16": bool(model.stream16), "steps": args.steps, "warmup": args.warmup,
           "repeats": args.repeats, "ms_per_step": round(med, 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3),
           "pairs_per_s": round(B / med * 1e3, 1), "loss": round(float(sum(v.detach() for v in out["ld"].values())), 5)}
    return row


def run_kernels(args, case, dev):
    import torch
    from clip_event_amd import posembed
    g_in, g_out, D = case
    pos = torch.randn(g_in * g_in + 1, D, device=dev)
    out = torch.empty(g_out * g_out + 1, D, device=dev)
    dout = torch.randn(g_out * g_out + 1, D, device=dev)
    dpos = torch.zeros(g_in * g_in + 1, D, device=dev)
    table = 2 * 4 * g_in * g_out                    # wy and wx
    rows = []
    for name, fn, nbytes in (
            ("fwd", lambda: posembed.resample(pos, g_out, out=out), 4 * D * (pos.shape[0] + out.shape[0]) + table),
            ("bwd", lambda: posembed.resample_backward(dout, g_in, accumulate=True, out=dpos),
             4 * D * (dout.shape[0] + 2 * dpos.shape[0]) + table)):
        for _ in range(20):
            fn()
        torch.cuda.synchronize()
        us = [w * 1e3 / LAUNCHES for w in _windows(torch, fn, LAUNCHES, args.repeats)]
        rows.append({"kernel": "ce_pos_resample_" + name, "g_in": g_in, "g_out": g_out, "D": D, "launches": LAUNCHES,
                     "repeats": args.repeats, "us_per_launch": round(statistics.median(us), 3), "us_min": round(min(us), 3),
                     "us_max": round(max(us), 3), "bytes": nbytes, "floor_us": round(nbytes / HBM_BYTES_PER_S * 1e6, 4)})
    return rows


def cases(args):
    return KERNEL_CASES if args.kernels else args.sizes


def child(args):
    """One case, in a process of its own."""
    import torch
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    case = cases(args)[args.case]
    print(json.dumps(run_kernels(args, case, dev) if args.kernels else run_size(args, case, dev)), flush=True)


def main():
    args = parse()
    if args.case is not None:
        return child(args)
    base = None
    for i, case in enumerate(cases(args)):
        cmd = [sys.executable, os.path.abspath(__file__), "--case", str(i)] + sys.argv[1:]
        try:
            r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=args.case_timeout)
        except subprocess.TimeoutExpired:
            sys.exit(f"case {case}: no result within {args.case_timeout:.0f} s; child killed, nothing further started")
        if r.returncode != 0 or not r.stdout.strip():
            sys.exit(f"case {case}: the measuring process ended with status {r.returncode} before its result; nothing further started")
        row = json.loads(r.stdout.strip().splitlines()[-1])
        if not args.kernels:
            base = row if case == BASE and base is None else base
            row["ms_ratio"] = round(row["ms_per_step"] / base["ms_per_step"], 4)
            row["token_ratio"] = round(row["tokens"] / base["tokens"], 4)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
