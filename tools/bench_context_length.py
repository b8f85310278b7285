#!/usr/bin/env python3
"""Time of the text tower at other context lengths (CLIP.set_context_length), packed against dense, and of the
packed long attention kernels against the dense long kernels, on one GPU.  bench.py stays the flagship measurement (it runs at
the native 77 tokens, where the feature launches nothing).

    python tools/bench_context_length.py                      # ViT-B/32 text tower, 256 captions: 77 / 128 / 248 tokens, packed and dense
    python tools/bench_context_length.py --kernels            # ce_attention_*_packed against ce_attention_* at Lmax = 248, fill 1, 1/2, 1/4

Tower lines (one JSON line per run length and layout): ``ms_fwd_bwd`` = the median of ``--repeats`` windows of ``--steps``
encode_text + backward passes each (HIP events around every window, after ``--warmup`` passes), ``ms_min`` / ``ms_max`` over the
windows, ``rows`` = activation rows of the pass, ``tower_tokens`` = what ``functional.text_tower_tokens`` gave the descriptor.
The captions follow ``synthetic_tokens``' length law at the run length (uniform in 8 .. T - 2 ids); ``dense`` is ``CE_TEXT_PACK=0``.
Kernel lines (one per fill ratio): B = 256 samples of H = 8 heads under the causal mask, every sample ``fill * Lmax`` tokens long
in the packed call, ``Lmax`` tokens in the dense one; ``us_fwd`` / ``us_bwd`` medians of ``--repeats`` windows of 50 launches.

Every case runs in a child process of its own, one after the other; this process never opens the GPU and gives every child
``--case-timeout`` seconds: a child that overruns it is killed, and after a child that failed nothing further is started."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LENGTHS = (77, 128, 248)
FILLS = (1.0, 0.5, 0.25)
LMAX, KB, KH = 248, 256, 8
LAUNCHES = 50


def parse():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--arch", default="vit_b32")
    ap.add_argument("--batch", type=int, default=256, help="captions per pass")
    ap.add_argument("--kernels", action="store_true", help="time the attention entry points alone instead of the tower")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5, help="timed windows per case; the median is reported")
    ap.add_argument("--case-timeout", type=float, default=240.0, help="seconds one case may take before the child is killed")
    ap.add_argument("--case", type=int, default=None, help=argparse.SUPPRESS)
    return ap.parse_args()


def cases(args):
    return list(FILLS) if args.kernels else [(T, packed) for T in LENGTHS for packed in (True, False)]


def _windows(torch, fn, n, repeats):
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


def run_tower(args, case, dev):
    import torch
    from clip_event_amd import synthetic as S
    from clip_event_amd.functional import _text_desc, attach_lengths, host_lengths, text_packing
    T, packed = case
    model = S.synthetic_model(args.arch, seed=0).to(dev)
    model.pack_text = packed
    model.set_context_length(T)
    n = args.batch
    host = S.synthetic_tokens(n, T, model.vocab_size, seed=999)
    lens = host_lengths(host)
    txt = attach_lengths(host.to(dev), lens)
    w = torch.randn(n, model.embed_dim, device=dev)

    def step():                       # (the gradients accumulate from pass to pass: the same launches)
        f = model.encode_text(txt)
        (f * w).sum().backward()

    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    ms = [x / args.steps for x in _windows(torch, step, args.steps, args.repeats)]
    pk = text_packing(model, txt)
    return {"arch": args.arch, "captions": n, "context_length": T, "native": int(model.native_context_length),
            "layout": "packed" if packed else "dense", "rows": int(pk.rows), "longest": int(lens.max()),
            "tower_tokens": int(_text_desc(model, pk).tokens), "stream16": bool(model.stream16), "steps": args.steps,
            "repeats": args.repeats, "ms_fwd_bwd": round(statistics.median(ms), 3), "ms_min": round(min(ms), 3),
            "ms_max": round(max(ms), 3)}


def run_kernels(args, fill, dev):
    import torch
    from clip_event_amd._lib import check, lib, ptr, stream
    B, H, L = KB, KH, LMAX
    D = H * 64
    n = max(1, int(round(fill * L)))
    rows = {}
    for name, per in (("packed", n), ("dense", L)):
        R = B * per
        qkv = torch.randn(R, 3 * D, device=dev).bfloat16()
        dout = torch.randn(R, D, device=dev).bfloat16()
        o, dqkv = torch.empty(R, D, device=dev, dtype=torch.bfloat16), torch.empty(R, 3 * D, device=dev, dtype=torch.bfloat16)
        lse, bias = torch.empty(B * H * L, device=dev), torch.zeros(3 * D, device=dev)
        cu = torch.arange(B + 1, device=dev, dtype=torch.int32) * per
        cl = lib()
        if name == "packed":
            fwd = lambda: check(cl.ce_attention_fwd_packed(ptr(qkv), 3 * D, ptr(o), D, ptr(lse), ptr(cu), B, L, H, 1, stream()), "fwd")
            bwd = lambda: check(cl.ce_attention_bwd_packed(ptr(qkv), 3 * D, ptr(o), D, ptr(dout), D, ptr(lse), ptr(dqkv), 3 * D,
                                                           ptr(bias), ptr(cu), B, L, H, 1, stream()), "bwd")
        else:
            fwd = lambda: check(cl.ce_attention_fwd(ptr(qkv), 3 * D, ptr(o), D, ptr(lse), None, B, L, H, 1, stream()), "fwd")
            bwd = lambda: check(cl.ce_attention_bwd(ptr(qkv), 3 * D, ptr(o), D, ptr(dout), D, ptr(lse), ptr(dqkv), 3 * D,
                                                    ptr(bias), None, B, L, H, 1, stream()), "bwd")
        for tag, fn in (("fwd", fwd), ("bwd", bwd)):
            for _ in range(5):
                fn()
            torch.cuda.synchronize()
            us = [x * 1e3 / LAUNCHES for x in _windows(torch, fn, LAUNCHES, args.repeats)]
            rows[f"{name}_us_{tag}"] = round(statistics.median(us), 2)
            rows[f"{name}_us_{tag}_min_max"] = [round(min(us), 2), round(max(us), 2)]
    return {"kernels": "long attention", "B": B, "H": H, "Lmax": L, "fill": fill, "tokens_per_sample": n, "launches": LAUNCHES,
            "repeats": args.repeats, **rows,
            "packed_over_dense_fwd": round(rows["packed_us_fwd"] / rows["dense_us_fwd"], 3),
            "packed_over_dense_bwd": round(rows["packed_us_bwd"] / rows["dense_us_bwd"], 3)}


def child(args):
    """One case, in a process of its own."""
    import torch
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    case = cases(args)[args.case]
    print(json.dumps(run_kernels(args, case, dev) if args.kernels else run_tower(args, case, dev)), flush=True)


def main():
    args = parse()
    if args.case is not None:
        return child(args)
    for i, case in enumerate(cases(args)):
        cmd = [sys.executable, os.path.abspath(__file__), "--case", str(i)] + sys.argv[1:]
        try:
            r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=args.case_timeout)
        except subprocess.TimeoutExpired:
            sys.exit(f"case {case}: no result within {args.case_timeout:.0f} s; child killed, nothing further started")
        if r.returncode != 0 or not r.stdout.strip():
            sys.exit(f"case {case}: the measuring process ended with status {r.returncode} before its result; nothing further started")
        print(r.stdout.strip().splitlines()[-1], flush=True)


if __name__ == "__main__":
    main()
