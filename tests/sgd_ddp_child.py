#!/usr/bin/env python3
"""One rank of the W>1 check of ``optim.FusedSGD`` (started by tests/test_sgd_gpu.py the way tests/test_ddp_gpu.py starts
tests/ddp_child.py: gloo backend, every rank on cuda:0).  Each rank runs two ``engine.train_step``s on its shard through the
real ``GradSync`` with FusedSGD -- CASE=allreduce: averaged gradients, every rank updates everything; CASE=sharded
(CE_SHARDED_ADAM=1 in the environment): reduce-scattered pieces, clip + SGD on the own shards, all-gather of the masters --
and rank 0 repeats the two steps in a single process on the CONCATENATED batch inside ``distributed.local_only()``.

Tolerances are those of tests/ddp_child.py: the accumulated update per parameter within rel-L2 2e-3 (its bound on the
gradients the update is made of: a shard and the concatenated batch tile differently), the masters as a whole within 1e-4,
the gradient norm within 1e-2, the momentum buffer within 2e-2 (its bounds on the sharded step's masters / norm / first moment).

    CASE=allreduce RANK=0 WORLD_SIZE=2 MASTER_ADDR=127.0.0.1 MASTER_PORT=29511 python tests/sgd_ddp_child.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.distributed as dist

LR, MU = 0.05, 0.9


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
    from clip_event_amd.optim import FusedSGD

    cfg = O.ClipConfig(64, 64, 4, 128, 32, 20, 512, 128, 2, 3)
    B, N = 3, W * 3
    sd = O.init_params(cfg, 11)
    img_all = S.synthetic_images(N, cfg.image_resolution, seed=5)
    txt_all = S.synthetic_tokens(N, cfg.context_length, cfg.vocab_size, seed=6, min_len=2)
    crit = CriterionContrastive("ce")

    def shard(lo, hi, r):
        yi, yt, ip = D.global_labels(hi - lo, 1, 0, True, device=dev, rank_=r)
        return img_all[lo:hi].to(dev), txt_all[lo:hi].to(dev), yi, yt, ip

    def run(args, sync):
        m = build_model({k: v.clone() for k, v in sd.items()}).to(dev)
        m.set_hyps(True, False, False)
        gs = D.GradSync(m) if sync else None                   # sharded or not: CE_SHARDED_ADAM, as a training job selects it
        opt = FusedSGD(m, lr=LR, momentum=MU, max_norm=1.0)
        for _ in range(2):
            train_step(m, crit, opt, *args, grad_sync=gs)
        torch.cuda.synchronize()
        return m, opt, gs

    m, opt, sync = run(shard(rank * B, (rank + 1) * B, rank), True)
    assert (sync.plan is not None) == (case == "sharded"), "CE_SHARDED_ADAM did not select the expected exchange"
    assert not sync.pending and not sync.dirty
    ok = True
    if case == "sharded":
        try:
            opt.state_dict()
            raise AssertionError("state_dict() of a sharded momentum buffer did not refuse")
        except RuntimeError as e:
            assert "consolidate" in str(e)
        D.consolidate(m, opt)
        assert set(opt.state_dict()["state"][0]) == {"momentum_buffer"}
    assert not m._mirror_fresh if case == "sharded" else m._mirror_fresh
    # every rank holds the same masters and (after consolidate) the same momentum buffer: bit for bit after the sharded step (one
    # all-reduced norm, every element updated by ONE rank); after the replicated update each rank has summed the squares of the
    # same averaged gradient with its own order of float atomics (ce_sumsq: relative error <= (blocks + 16) 2^-24 of the sum,
    # tests/test_embed_optim_ops.py::test_sumsq_against_fp64), so each rank's clip coefficient 1 / sqrt(sum) is within half of that
    # and two ranks' updates -- the momentum buffer, and the far smaller change of the masters -- within (blocks + 16) 2^-24
    blocks = min(2048, (m._flat.numel() + 1023) // 1024)
    for what, t in (("masters", m._flat.detach()), ("momentum buffer", opt.buf)):
        mx = t.clone()
        dist.all_reduce(mx, op=dist.ReduceOp.MAX)
        if case == "sharded":
            ok &= bool(torch.equal(mx, t))
        else:
            rel = float((mx - t).norm() / t.norm())
            print(f"[{case}] rank {rank} {what} against the element-wise maximum over the ranks: rel-L2 {rel:.3e}", flush=True)
            ok &= rel <= (blocks + 16) * 2.0 ** -24
    if rank == 0:
        with D.local_only():
            m1, opt1, _ = run(shard(0, N, 0), False)
        rel = float((m._flat - m1._flat).norm() / m1._flat.norm())
        print(f"[{case}] masters after two steps, W ranks vs single process: rel-L2 {rel:.3e}", flush=True)
        ok &= rel < 1e-4
        gn, gn1 = float(opt.grad_norm()), float(opt1.grad_norm())
        print(f"[{case}] gradient norm {gn:.6f} vs {gn1:.6f}", flush=True)
        ok &= gn1 > 1.0 and abs(gn - gn1) <= 1e-2 * gn1          # (> 1: the clip is active)
        worst = (0.0, "")
        for n, p in m1.named_parameters():
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
        live = torch.zeros(m._flat.numel(), dtype=torch.bool, device=dev)
        for n, p in m1._pmap.items():
            live[m1._offsets[n]: m1._offsets[n] + p.numel()] = True
        rel = float((opt.buf[live] - opt1.buf[live]).norm() / opt1.buf[live].norm())
        print(f"[{case}] momentum buffer: rel-L2 {rel:.3e}", flush=True)
        ok &= rel < 2e-2
    flag = torch.tensor([1.0 if ok else 0.0])
    dist.all_reduce(flag, op=dist.ReduceOp.MIN)
    if rank == 0:
        print(f"[{case}] {'OK' if float(flag) == 1.0 else 'FAILED'}", flush=True)
    dist.barrier()
    dist.destroy_process_group()
    sys.exit(0 if float(flag) == 1.0 else 1)


if __name__ == "__main__":
    main()
