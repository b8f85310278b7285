#!/usr/bin/env python3
"""One rank of the W>1 check of partial fine-tuning (started by tests/test_partial_gpu.py the way tests/test_sgd_gpu.py starts
tests/sgd_ddp_child.py: gloo backend, every rank on cuda:0).  The image tower is locked; each rank runs two
``engine.train_step``s on its shard through the real ``GradSync`` with FusedSGD -- the locked tower's range is neither waited
for nor exchanged -- and rank 0 repeats the two steps in a single process on the CONCATENATED batch inside
``distributed.local_only()``.

Tolerances are those of tests/sgd_ddp_child.py: the accumulated update per trainable parameter within rel-L2 2e-3, the masters as
a whole within 1e-4, the gradient norm within 1e-2.  Locked parameters keep their bits on every rank, and the sharded optimiser
step refuses a model with frozen parameters.

    CASE=locked RANK=0 WORLD_SIZE=2 MASTER_ADDR=127.0.0.1 MASTER_PORT=29511 python tests/partial_ddp_child.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.distributed as dist

LR, MU = 0.05, 0.9


def main():
    rank, W = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    case = os.environ.get("CASE", "locked")
    dist.init_process_group("gloo")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    from oracle import clip_oracle as O
    from clip_event_amd import synthetic as S, distributed as D
    from clip_event_amd.engine import train_step
    from clip_event_amd.losses import CriterionContrastive
    from clip_event_amd.model import build_model
    from clip_event_amd.optim import FusedSGD

    cfg = O.ClipConfig(64, 64, 2, 128, 32, 20, 512, 128, 2, 3)
    B, N = 3, W * 3
    sd = O.init_params(cfg, 11)
    img_all = S.synthetic_images(N, cfg.image_resolution, seed=5)
    txt_all = S.synthetic_tokens(N, cfg.context_length, cfg.vocab_size, seed=6, min_len=2)
    crit = CriterionContrastive("ce")

    def shard(lo, hi, r):
        yi, yt, ip = D.global_labels(hi - lo, 1, 0, True, device=dev, rank_=r)
        return img_all[lo:hi].to(dev), txt_all[lo:hi].to(dev), yi, yt, ip

    def locked_model():
        m = build_model({k: v.clone() for k, v in sd.items()}).to(dev)
        m.set_hyps(True, False, False)
        m.lock_image_tower()
        return m

    def run(args, sync):
        m = locked_model()
        gs = D.GradSync(m) if sync else None
        opt = FusedSGD(m, lr=LR, momentum=MU, max_norm=1.0)
        for _ in range(2):
            train_step(m, crit, opt, *args, grad_sync=gs)
        torch.cuda.synchronize()
        return m, opt, gs

    ok = True
    try:
        D.GradSync(locked_model(), sharded=True)
        ok = False
        print(f"[{case}] rank {rank}: the sharded optimiser step accepted a model with frozen parameters", flush=True)
    except NotImplementedError as e:
        assert "frozen" in str(e)
    m, opt, sync = run(shard(rank * B, (rank + 1) * B, rank), True)
    assert sync.plan is None and not sync.pending and not sync.dirty
    for n, p in m.named_parameters():
        if n.startswith("visual."):
            same = torch.equal(p.detach().cpu().view(torch.int32), sd[n].contiguous().view(torch.int32))
            ok &= same and p.grad is None
            if not same:
                print(f"[{case}] rank {rank}: locked parameter {n} moved", flush=True)
    if rank == 0:
        with D.local_only():
            m1, opt1, _ = run(shard(0, N, 0), False)
        live = torch.zeros(m._flat.numel(), dtype=torch.bool, device=dev)
        for n, p in m1._pmap.items():
            live[m1._offsets[n]: m1._offsets[n] + p.numel()] = True
        rel = float((m._flat[live] - m1._flat[live]).norm() / m1._flat[live].norm())
        print(f"[{case}] masters after two steps, W ranks vs single process: rel-L2 {rel:.3e}", flush=True)
        ok &= rel < 1e-4
        gn, gn1 = float(opt.grad_norm()), float(opt1.grad_norm())
        print(f"[{case}] gradient norm {gn:.6f} vs {gn1:.6f}", flush=True)
        ok &= gn1 > 1.0 and abs(gn - gn1) <= 1e-2 * gn1          # (> 1: the clip is active)
        worst = (0.0, "")
        for n, p in m1.named_parameters():
            if not p.requires_grad:
                continue
            o, k = m1._offsets[n], p.numel()
            start = sd[n].to(dev).flatten().double()
            a, b = m._flat[o:o + k].double() - start, m1._flat[o:o + k].double() - start
            if float(b.norm()) == 0.0:
                if float(a.norm()) != 0.0:
                    ok = False
                    print(f"[{case}] {n}: the single process did not move it, the ranks did", flush=True)
                continue
            r = float((a - b).norm() / b.norm())
            if r > worst[0]:
                worst = (r, n)
        print(f"[{case}] worst per-parameter rel-L2 of the accumulated update {worst[0]:.3e} at {worst[1]}", flush=True)
        ok &= worst[0] <= 2e-3
    flag = torch.tensor([1.0 if ok else 0.0])
    dist.all_reduce(flag, op=dist.ReduceOp.MIN)
    if rank == 0:
        print(f"[{case}] {'OK' if float(flag) == 1.0 else 'FAILED'}", flush=True)
    dist.barrier()
    dist.destroy_process_group()
    sys.exit(0 if float(flag) == 1.0 else 1)


if __name__ == "__main__":
    main()
