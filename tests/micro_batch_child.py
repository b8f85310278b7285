#!/usr/bin/env python3
"""One rank of the W = 2 check of the micro-batched step (started by tests/test_micro_batch_gpu.py the way
tests/test_ddp_gpu.py starts tests/ddp_child.py; gloo backend, every rank on cuda:0).

Each rank runs the global-batch ``engine.train_step`` on its shard twice over: unchunked, and with ``micro_batch`` = half
the per-rank batch, both through the real ``GradSync`` (CASE=allreduce: mean all-reduce; CASE=sharded: the reduce-scatter
of the sharded optimiser step).  The two must agree -- losses within 3e-3 * max(1, |loss|), worst per-parameter gradient
rel-L2 2e-3, zero where the unchunked gradient is zero (the bounds tests/ddp_child.py puts on a shard against the
concatenated batch: the chunks tile differently) -- every rank must hold the same averaged gradient, and the elements
handed to ``GradSync._reduce_range`` must add up to ONE buffer length per step.

    CASE=allreduce RANK=0 WORLD_SIZE=2 MASTER_ADDR=127.0.0.1 MASTER_PORT=29511 python tests/micro_batch_child.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.distributed as dist


def main():
    rank, W = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    case = os.environ.get("CASE", "allreduce")
    dist.init_process_group("gloo")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    from oracle import clip_oracle as O
    from clip_event_amd import synthetic as S, distributed as D
    from clip_event_amd.engine import train_step
    from clip_event_amd.losses import CriterionContrastive
    from clip_event_amd.model import build_model
    from clip_event_amd.optim import FusedAdam

    cfg = O.ClipConfig(64, 64, 4, 128, 32, 20, 512, 128, 2, 3)
    B, K = 4, 2
    sd = O.init_params(cfg, 11)
    N = W * B
    img_all = S.synthetic_images(N, cfg.image_resolution, seed=5)
    txt_all = S.synthetic_tokens(N * K, cfg.context_length, cfg.vocab_size, seed=6, min_len=2)
    crit = CriterionContrastive("ce")
    lo, hi = rank * B, (rank + 1) * B
    yi, yt, ip = D.global_labels(B, 1, K - 1, True, device=dev, rank_=rank)
    args = (img_all[lo:hi].to(dev), txt_all[lo * K:hi * K].to(dev), yi, yt, ip)

    ok = True
    out = {}
    for mb in (None, B // 2):
        m = build_model({k: v.clone() for k, v in sd.items()}).to(dev)
        m.set_hyps(True, False, False)
        sync = D.GradSync(m, sharded=(case == "sharded"))
        assert (sync.plan is not None) == (case == "sharded")
        reduced = []
        inner = sync._reduce_range

        def counting(a, b, async_op, inner=inner, reduced=reduced):
            if b > a:
                reduced.append(b - a)
            return inner(a, b, async_op)

        sync._reduce_range = counting
        opt = FusedAdam(m, lr=0.0, max_norm=1.0)           # lr 0: the averaged gradients stay in the buffer
        for it in range(2):           # twice: the second step proves the per-step bookkeeping resets
            del reduced[:]
            if m._flat_grad is not None:                    # (allocated by the first forward)
                m._flat_grad.fill_(float("nan"))
            ld = train_step(m, crit, opt, *args, grad_sync=sync, micro_batch=mb)
            torch.cuda.synchronize()
            if sum(reduced) != m._flat_grad.numel():
                ok = False
                print(f"[{case}] rank {rank} micro_batch={mb} step {it}: {sum(reduced)} elements went through _reduce_range, "
                      f"the buffer has {m._flat_grad.numel()} ({len(reduced)} calls)", flush=True)
        assert not sync.pending and not sync.dirty and not sync.announced and sync.expected == {"visual": 0, "text": 0}
        g = m._flat_grad.detach().clone()
        if not bool(torch.isfinite(g).all()):
            ok = False
            print(f"[{case}] rank {rank} micro_batch={mb}: non-finite gradient elements", flush=True)
        gmax = g.clone()
        dist.all_reduce(gmax, op=dist.ReduceOp.MAX)
        if not torch.equal(gmax, g):
            ok = False
            print(f"[{case}] rank {rank} micro_batch={mb}: ranks disagree on the averaged gradient", flush=True)
        out[mb] = (m, g, {k: float(v) for k, v in ld.items()})

    m, g, ld = out[B // 2]
    _, g_ref, ld_ref = out[None]
    for k in ld_ref:
        print(f"[{case}] rank {rank} {k}: chunked {ld[k]:.5f} vs unchunked {ld_ref[k]:.5f}", flush=True)
        if abs(ld[k] - ld_ref[k]) > 3e-3 * max(1.0, abs(ld_ref[k])):
            ok = False
    worst_rel, worst_name = 0.0, ""
    for n, p in m.named_parameters():
        o = m._offsets[n]
        a, b = g[o:o + p.numel()].double(), g_ref[o:o + p.numel()].double()
        if float(b.norm()) == 0.0:
            if float(a.norm()) != 0.0:
                ok = False
                print(f"[{case}] rank {rank} {n}: unchunked gradient is zero, chunked is not", flush=True)
            continue
        rel = float((a - b).norm() / b.norm())
        if rel > worst_rel:
            worst_rel, worst_name = rel, n
    print(f"[{case}] rank {rank} worst gradient rel-L2 chunked vs unchunked {worst_rel:.2e} at {worst_name}", flush=True)
    if worst_rel > 2e-3:
        ok = False
    flag = torch.tensor([1.0 if ok else 0.0])
    dist.all_reduce(flag, op=dist.ReduceOp.MIN)
    if rank == 0:
        print(f"[{case}] {'OK' if float(flag) == 1.0 else 'FAILED'}", flush=True)
    dist.barrier()
    dist.destroy_process_group()
    sys.exit(0 if float(flag) == 1.0 else 1)


if __name__ == "__main__":
    main()
