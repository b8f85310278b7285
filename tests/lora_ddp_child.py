#!/usr/bin/env python3
"""One rank of the W>1 check of low-rank adapters (started by tests/test_lora_gpu.py the way tests/test_partial_gpu.py starts
tests/partial_ddp_child.py: gloo backend, every rank on cuda:0).  Each rank runs one ``engine.train_step`` on its shard through
the real ``GradSync`` with FusedSGD; rank 0 repeats the step in a single process on the CONCATENATED batch inside
``distributed.local_only()``.

The adapters' gradients are made AFTER the exchange from the all-reduced weight gradient of the frozen adapted matrices
(``finish_lora_grads`` in ``step()``): they are linear in it and the adapters are equal on every rank, so this equals all-reducing
them.  It needs the dW range of a FROZEN matrix to be exchanged, which is pinned here directly: after the step the dW slices on
every rank equal the single process's (rel-L2 2e-3; a slice that was not exchanged holds the half batch's gradient, a different
vector).

Tolerances are those of tests/partial_ddp_child.py: the update per trainable parameter within rel-L2 2e-3, the masters as a whole
within 1e-4, the gradient norm within 1e-2.  Base parameters keep their bits on every rank.

    CASE=lora RANK=0 WORLD_SIZE=2 MASTER_ADDR=127.0.0.1 MASTER_PORT=29511 python tests/lora_ddp_child.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.distributed as dist

LR, MU = 0.05, 0.9


def main():
    rank, W = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    case = os.environ.get("CASE", "lora")
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

    def lora_model():
        m = build_model({k: v.clone() for k, v in sd.items()}).to(dev)
        m.set_hyps(True, False, False)
        m.enable_lora(rank=4, alpha=8.0, seed=3)
        g = torch.Generator().manual_seed(4)                   # B != 0: both adapters of a pair see a gradient
        with torch.no_grad():
            for n, p in m.named_parameters():
                if n.endswith("lora_B"):
                    p.copy_((torch.randn(p.shape, generator=g) * 0.05).to(dev))
        return m

    def run(args, sync):
        m = lora_model()
        start = {n: p.detach().clone() for n, p in m.named_parameters()}
        gs = D.GradSync(m) if sync else None
        opt = FusedSGD(m, lr=LR, momentum=MU, max_norm=1.0)
        train_step(m, crit, opt, *args, grad_sync=gs)
        torch.cuda.synchronize()
        return m, opt, start

    ok = True
    m, opt, start = run(shard(rank * B, (rank + 1) * B, rank), True)
    adapters = set(m.lora_parameter_names())
    for n, p in m.named_parameters():
        if n not in adapters:
            same = torch.equal(p.detach().view(torch.int32), start[n].view(torch.int32))
            ok &= same and p.grad is None
            if not same:
                print(f"[{case}] rank {rank}: base parameter {n} moved", flush=True)
    if rank == 0:
        with D.local_only():
            m1, opt1, _ = run(shard(0, N, 0), False)
        worst_dw = (0.0, "")
        for w, _, _ in m1._lora["entries"]:
            a, b = m._gview(w).double(), m1._gview(w).double()
            r = float((a - b).norm() / b.norm())
            if r > worst_dw[0]:
                worst_dw = (r, w)
        print(f"[{case}] weight gradients of the frozen adapted matrices, W ranks vs single process: worst rel-L2 {worst_dw[0]:.3e} "
              f"at {worst_dw[1]}", flush=True)
        ok &= worst_dw[0] <= 2e-3
        live = torch.zeros(m._flat.numel(), dtype=torch.bool, device=dev)
        for n, p in m1._pmap.items():
            live[m1._offsets[n]: m1._offsets[n] + p.numel()] = True
        rel = float((m._flat[live] - m1._flat[live]).norm() / m1._flat[live].norm())
        print(f"[{case}] masters after the step, W ranks vs single process: rel-L2 {rel:.3e}", flush=True)
        ok &= rel < 1e-4
        gn, gn1 = float(opt.grad_norm()), float(opt1.grad_norm())
        print(f"[{case}] gradient norm {gn:.6f} vs {gn1:.6f}", flush=True)
        ok &= gn1 > 0.0 and abs(gn - gn1) <= 1e-2 * gn1
        worst = (0.0, "")
        for n in m1.lora_parameter_names():
            o, k = m1._offsets[n], m1._pmap[n].numel()
            s0 = start[n].flatten().double()
            a, b = m._flat[o:o + k].double() - s0, m1._flat[o:o + k].double() - s0
            if float(b.norm()) == 0.0:
                ok = False
                print(f"[{case}] {n}: the single process did not move it", flush=True)
                continue
            r = float((a - b).norm() / b.norm())
            if r > worst[0]:
                worst = (r, n)
        print(f"[{case}] worst per-adapter rel-L2 of the update {worst[0]:.3e} at {worst[1]}", flush=True)
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
