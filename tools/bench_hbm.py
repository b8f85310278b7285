#!/usr/bin/env python3
"""Micro-benchmarks of the HBM-bound kernels at the step's shapes with COLD operands: every call works on the next of
NSETS buffer sets (together larger than the 256 MiB Infinity Cache), as in the step, where a kernel's inputs were written
tens of kernels earlier.  Prints us per call and GB/s on the algorithmic bytes.   python tools/bench_hbm.py [ln adam sgd attn]
lion: clip + Lion, flat (22 B per parameter) and tiled (24 B), each beside the SGD-with-momentum form that moves the same bytes.
adam_ema / sgd_ema / lion_ema: the tiled update with the weight average fused in, beside the same update without it and beside "update, then
``ema.lerp_(masters, rate)``" -- what the fusion replaces -- in alternation in one process."""
import os
import sys
from ctypes import c_float, c_int, c_long

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from clip_event_amd import ops, _lib as L
from clip_event_amd._lib import check, lib, ptr, stream

DEV = "cuda:0"
NSETS = 6


def timeit(fns, iters=36, warm=6):
    for i in range(warm):
        fns[i % len(fns)]()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(iters):
        fns[i % len(fns)]()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e-3


def bench_ln():
    for name, M, D in (("image", 12800, 768), ("text", 10800, 512)):
        w = torch.ones(D, device=DEV)
        b = torch.zeros(D, device=DEV)
        gs = torch.tensor([4096.0], device=DEV)
        sets = []
        for _ in range(NSETS):
            x16 = torch.randn(M, D, device=DEV).to(torch.float16)
            dy = (torch.randn(M, D, device=DEV) * 1e-3).to(torch.bfloat16)
            dx = (torch.randn(M, D, device=DEV)).to(torch.float16)
            dxb = torch.empty(M, D, device=DEV, dtype=torch.bfloat16)
            y = torch.empty(M, D, device=DEV, dtype=torch.bfloat16)
            mean = torch.zeros(M, device=DEV)
            rstd = torch.ones(M, device=DEV)
            sets.append((x16, dy, dx, dxb, y, mean, rstd))
        dw, db, dxs = torch.zeros(D, device=DEV), torch.zeros(D, device=DEV), torch.zeros(D, device=DEV)

        def fwd(s):
            x16, dy, dx, dxb, y, mean, rstd = s
            check(lib().ce_layernorm_fwd_t(ptr(x16), c_int(L.T_F16), c_long(D), None, ptr(w), ptr(b), ptr(y), c_int(L.T_BF16), c_long(D),
                                           ptr(mean), ptr(rstd), c_int(M), c_int(D), c_float(1e-5), stream()), "ln_fwd")

        def bwd(s):
            x16, dy, dx, dxb, y, mean, rstd = s
            ops.layernorm_bwd_t(dy, x16, mean, rstd, w, dw, db, dx, gscale=gs, dx_in=dx, dxb=dxb, dxsum=dxs)

        t = timeit([lambda s=s: s[4].copy_(s[0]) for s in sets])      # floor of a launch that moves the same bytes: torch's converting copy
        print(f"copy16  {name:5s} M={M} D={D}: {t * 1e6:7.1f} us  {M * D * 4 / t / 1e9:7.0f} GB/s   (fp16 -> bf16 elementwise copy, same bytes as ln_fwd)", flush=True)
        t = timeit([lambda s=s: fwd(s) for s in sets])
        print(f"ln_fwd  {name:5s} M={M} D={D}: {t * 1e6:7.1f} us  {M * D * 4 / t / 1e9:7.0f} GB/s", flush=True)
        t = timeit([lambda s=s: bwd(s) for s in sets])
        print(f"ln_bwd  {name:5s} M={M} D={D}: {t * 1e6:7.1f} us  {M * D * 10 / t / 1e9:7.0f} GB/s", flush=True)


def bench_adam():
    n = 151_277_312
    p = torch.randn(n, device=DEV) * 0.02
    g = torch.randn(n, device=DEV) * 1e-3
    m = torch.zeros(n, device=DEV)
    v = torch.zeros(n, device=DEV)
    p16 = torch.empty(n, device=DEV, dtype=torch.bfloat16)
    ss = torch.zeros(1, device=DEV)

    def adam():
        check(lib().ce_adam_step(ptr(p), ptr(g), ptr(m), ptr(v), ptr(p16), c_long(n), ptr(ss), c_float(1.0), c_float(1e-6),
                                 c_float(0.9), c_float(0.999), c_float(1e-8), c_float(0.0), c_int(3), stream()), "adam")

    def sumsq():
        check(lib().ce_sumsq(ptr(g), c_long(n), ptr(ss), stream()), "sumsq")

    t = timeit([adam], iters=10, warm=2)
    print(f"adam    n={n}: {t * 1e6:7.1f} us  {n * 30 / t / 1e9:7.0f} GB/s", flush=True)
    t = timeit([sumsq], iters=10, warm=2)
    print(f"sumsq   n={n}: {t * 1e6:7.1f} us  {n * 4 / t / 1e9:7.0f} GB/s", flush=True)
    t = timeit([lambda: g.zero_()], iters=10, warm=2)
    print(f"zero    n={n}: {t * 1e6:7.1f} us  {n * 4 / t / 1e9:7.0f} GB/s", flush=True)


_TILED = {}


def _tiled_model():
    """The ViT-B/32 model's own flat buffers, transpose-job table and segment table (the layout the step's tiled update
    runs over) with a gradient and both optimisers' state buffers."""
    if not _TILED:
        from clip_event_amd import synthetic as S
        from clip_event_amd.optim import FusedAdam
        m = S.synthetic_model("vit_b32", seed=0).to(DEV)
        opt = FusedAdam(m, lr=1e-6)
        opt.zero_grad()
        assert m._adam_tiles_ok
        m._flat_grad.copy_(torch.randn_like(m._flat_grad) * 1e-3)
        _TILED.update(m=m, a=opt.m, b=opt.v, ss=torch.zeros(1, device=DEV), seg=m._adam_segment_table())
    return _TILED


def bench_adam_tiles():
    t = _tiled_model()
    m, seg, (tj, tn_, tt) = t["m"], t["seg"], t["m"]._tjobs_bwd
    n = sum(p.numel() for p in m.parameters())

    def adam():
        check(lib().ce_adam_step_tiles(ptr(m._flat), ptr(m._flat_grad), ptr(t["a"]), ptr(t["b"]), ptr(m._flat16), ptr(tj), c_int(tn_),
                                       c_int(tt), ptr(seg), c_int(seg.shape[0]), ptr(t["ss"]), c_float(1.0), c_float(1e-6), c_float(0.9),
                                       c_float(0.999), c_float(1e-8), c_float(0.0), c_int(3), stream()), "adam tiles")

    dt = timeit([adam], iters=10, warm=2)
    print(f"adam tiles n={n}: {dt * 1e6:7.1f} us  {n * 32 / dt / 1e9:7.0f} GB/s   (30 B + 2 B of W^T per parameter)", flush=True)
    return dt


def bench_sgd():
    """clip + SGD with momentum 0.9: the flat kernel on buffers of its own (12 B read + 10 B written per parameter) and the tiled
    form over the model's layout (+ 2 B of W^T), beside the tiled Adam update measured in the same run."""
    n = 151_277_312
    p = torch.randn(n, device=DEV) * 0.02
    g = torch.randn(n, device=DEV) * 1e-3
    buf = torch.zeros(n, device=DEV)
    p16 = torch.empty(n, device=DEV, dtype=torch.bfloat16)
    ss = torch.zeros(1, device=DEV)

    def sgd():
        check(lib().ce_sgd_step(ptr(p), ptr(g), ptr(buf), ptr(p16), c_long(n), ptr(ss), c_float(1.0), c_float(1e-6), c_float(0.9),
                                c_float(0.0), c_float(0.0), c_int(0), c_int(0), stream()), "sgd")

    dt = timeit([sgd], iters=10, warm=2)
    print(f"sgd     n={n}: {dt * 1e6:7.1f} us  {n * 22 / dt / 1e9:7.0f} GB/s", flush=True)
    del p, g, buf, p16
    t = _tiled_model()
    m, seg, (tj, tn_, tt) = t["m"], t["seg"], t["m"]._tjobs_bwd
    n = sum(q.numel() for q in m.parameters())

    def sgd_tiles():
        check(lib().ce_sgd_step_tiles(ptr(m._flat), ptr(m._flat_grad), ptr(t["a"]), ptr(m._flat16), ptr(tj), c_int(tn_), c_int(tt),
                                      ptr(seg), c_int(seg.shape[0]), ptr(t["ss"]), c_float(1.0), c_float(1e-6), c_float(0.9), c_float(0.0),
                                      c_float(0.0), c_int(0), c_int(0), stream()), "sgd tiles")

    for _ in range(2):                      # the two tiled updates in alternation: same box, same minute
        t_adam = bench_adam_tiles()
        dt = timeit([sgd_tiles], iters=10, warm=2)
        print(f"sgd tiles  n={n}: {dt * 1e6:7.1f} us  {n * 24 / dt / 1e9:7.0f} GB/s   ({dt / t_adam:.2f} of the tiled Adam update; bytes: 24 / 32 = 0.75)",
              flush=True)


def bench_lion(rounds=2):
    """clip + Lion beside clip + SGD with momentum 0.9, which moves exactly the same bytes: the flat kernels on buffers of their own
    (12 B read + 10 B written per parameter) and the tiled forms over the model's layout (+ 2 B of W^T), each pair in alternation
    (same box, same minute), ``rounds`` times."""
    n = 151_277_312
    p = torch.randn(n, device=DEV) * 0.02
    g = torch.randn(n, device=DEV) * 1e-3
    buf = torch.zeros(n, device=DEV)
    p16 = torch.empty(n, device=DEV, dtype=torch.bfloat16)
    ss = torch.zeros(1, device=DEV)

    def sgd():
        check(lib().ce_sgd_step(ptr(p), ptr(g), ptr(buf), ptr(p16), c_long(n), ptr(ss), c_float(1.0), c_float(1e-6), c_float(0.9),
                                c_float(0.0), c_float(0.0), c_int(0), c_int(0), stream()), "sgd")

    def lion():
        check(lib().ce_lion_step(ptr(p), ptr(g), ptr(buf), ptr(p16), c_long(n), ptr(ss), c_float(1.0), c_float(1e-6), c_float(0.9),
                                 c_float(0.99), c_float(0.0), stream()), "lion")

    for r in range(rounds):
        t_sgd = timeit([sgd], iters=10, warm=2)
        print(f"sgd     round {r} n={n}: {t_sgd * 1e6:7.1f} us  {n * 22 / t_sgd / 1e9:7.0f} GB/s", flush=True)
        dt = timeit([lion], iters=10, warm=2)
        print(f"lion    round {r} n={n}: {dt * 1e6:7.1f} us  {n * 22 / dt / 1e9:7.0f} GB/s   ({dt / t_sgd:.3f} of the SGD line above; same bytes)",
              flush=True)
    del p, g, buf, p16
    t = _tiled_model()
    m, seg, (tj, tn_, tt) = t["m"], t["seg"], t["m"]._tjobs_bwd
    n = sum(q.numel() for q in m.parameters())
    head = (ptr(m._flat), ptr(m._flat_grad), ptr(t["a"]), ptr(m._flat16), ptr(tj), c_int(tn_), c_int(tt), ptr(seg), c_int(seg.shape[0]),
            ptr(t["ss"]), c_float(1.0), c_float(1e-6))

    def sgd_tiles():
        check(lib().ce_sgd_step_tiles(*head, c_float(0.9), c_float(0.0), c_float(0.0), c_int(0), c_int(0), stream()), "sgd tiles")

    def lion_tiles():
        check(lib().ce_lion_step_tiles(*head, c_float(0.9), c_float(0.99), c_float(0.0), stream()), "lion tiles")

    for r in range(rounds):
        t_sgd = timeit([sgd_tiles], iters=10, warm=2)
        print(f"sgd tiles  round {r} n={n}: {t_sgd * 1e6:7.1f} us  {n * 24 / t_sgd / 1e9:7.0f} GB/s", flush=True)
        dt = timeit([lion_tiles], iters=10, warm=2)
        print(f"lion tiles round {r} n={n}: {dt * 1e6:7.1f} us  {n * 24 / dt / 1e9:7.0f} GB/s   ({dt / t_sgd:.3f} of the SGD line above; same bytes)",
              flush=True)


def bench_ema(kinds, rounds=3):
    """The step's tiled update over the ViT-B/32 layout (same parameter count as ``adam`` / ``sgd``) in three forms, measured in
    alternation (same box, same minute), ``rounds`` times: without the average (Adam 32 B, SGD 24 B per parameter); with the
    average in the same kernels (+ 8 B: read and write it); and the reference point, the update without it followed by one
    ``ema.lerp_(masters, rate)`` over the flat buffers (+ 12 B: read both, write one, and one more launch)."""
    t = _tiled_model()
    m, seg, (tj, tn_, tt) = t["m"], t["seg"], t["m"]._tjobs_bwd
    n = sum(q.numel() for q in m.parameters())
    ema = m._flat.detach().clone()
    rate = 1e-4
    tables = (ptr(m._flat16), ptr(tj), c_int(tn_), c_int(tt), ptr(seg), c_int(seg.shape[0]), ptr(t["ss"]), c_float(1.0), c_float(1e-6))
    tails = {"adam": (c_float(0.9), c_float(0.999), c_float(1e-8), c_float(0.0), c_int(3)),
             "sgd": (c_float(0.9), c_float(0.0), c_float(0.0), c_int(0), c_int(0)),
             "lion": (c_float(0.9), c_float(0.99), c_float(0.0))}
    state = {"adam": (ptr(t["a"]), ptr(t["b"])), "sgd": (ptr(t["a"]),), "lion": (ptr(t["a"]),)}
    base_bytes = {"adam": 32, "sgd": 24, "lion": 24}

    def step(kind, fused):
        name = f"ce_{kind}_step_tiles" + ("_ema" if fused else "")
        extra = (ptr(ema), c_float(rate)) if fused else ()
        check(getattr(lib(), name)(ptr(m._flat), ptr(m._flat_grad), *state[kind], *tables, *tails[kind], *extra, stream()), name)

    def then_lerp(kind):
        step(kind, False)
        ema.lerp_(m._flat, rate)

    for r in range(rounds):
        for kind in kinds:
            b = base_bytes[kind]
            plain = timeit([lambda: step(kind, False)], iters=10, warm=2)
            fused = timeit([lambda: step(kind, True)], iters=10, warm=2)
            ref = timeit([lambda: then_lerp(kind)], iters=10, warm=2)
            print(f"{kind}_ema round {r} n={n}: tiles {plain * 1e6:7.1f} us {n * b / plain / 1e12:5.2f} TB/s | tiles + fused average "
                  f"{fused * 1e6:7.1f} us {n * (b + 8) / fused / 1e12:5.2f} TB/s (+{(fused - plain) * 1e6:6.1f} us) | tiles, then lerp_ "
                  f"{ref * 1e6:7.1f} us {n * (b + 12) / ref / 1e12:5.2f} TB/s (+{(ref - plain) * 1e6:6.1f} us) | fused / reference "
                  f"{fused / ref:.3f}", flush=True)


def bench_attn():
    for name, B, Ltok, H, causal in (("image", 256, 50, 12, False), ("text", 256, 77, 8, True)):
        sets = []
        for _ in range(NSETS):
            qkv = torch.randn(B * Ltok, 3 * H * 64, device=DEV).to(torch.bfloat16)
            do = (torch.randn(B * Ltok, H * 64, device=DEV) * 1e-2).to(torch.bfloat16)
            sets.append((qkv, do))
        outs = [ops.attention_fwd(q, B, Ltok, H, causal) for q, _ in sets]
        bias = torch.zeros(3 * H * 64, device=DEV)
        t = timeit([lambda q=q: ops.attention_fwd(q, B, Ltok, H, causal) for q, _ in sets])
        M = B * Ltok
        print(f"attn_fwd {name:5s}: {t * 1e6:7.1f} us  {M * H * 64 * 2 * 4 / t / 1e9:7.0f} GB/s", flush=True)
        t = timeit([lambda q=q, d=d, o=o: ops.attention_bwd(q, o[0], d, o[1], B, Ltok, H, causal, bias_grad=bias)
                    for (q, d), o in zip(sets, outs)])
        print(f"attn_bwd {name:5s}: {t * 1e6:7.1f} us  {M * H * 64 * 2 * 8 / t / 1e9:7.0f} GB/s", flush=True)


if __name__ == "__main__":
    which = sys.argv[1:] or ["ln", "adam", "sgd", "attn"]
    if "ln" in which:
        bench_ln()
    if "adam" in which:
        bench_adam()
    if "sgd" in which:
        bench_sgd()
    if "lion" in which:
        bench_lion()
    if "adam_ema" in which or "sgd_ema" in which or "lion_ema" in which:
        bench_ema([k for k in ("adam", "sgd", "lion") if k + "_ema" in which])
    if "attn" in which:
        bench_attn()
