#!/usr/bin/env python3
"""One rank of the W>1 check of the multi-positive loss (started by tests/test_multipos_gpu.py the way tests/test_sigmoid_gpu.py
starts tests/sigmoid_ddp_child.py: gloo backend, every rank on cuda:0).  Each rank runs ``engine.train_step`` on its shard
through the real ``GradSync``: its own rows against the all-gathered features, group ids from ``distributed.global_groups``
with (num_pos, num_neg) = (2, 2), gathered in ONE more collective than the 'ce' step issues.  Rank 0 then recomputes the step in
a single process on the CONCATENATED batch inside ``distributed.local_only()``.

The mean of the ranks' losses must equal the single-process ones, and every parameter's synchronised gradient the
single-process one, at tests/ddp_child.py's bounds: loss 3e-3 max(1, |loss|), worst per-parameter rel-L2 2e-3, zero where the
reference is zero.  The script stops at the first failure.

    CASE=p2n2 RANK=0 WORLD_SIZE=2 MASTER_ADDR=127.0.0.1 MASTER_PORT=29511 python tests/multipos_ddp_child.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.distributed as dist


class _GradOnly:
    """Optimizer stand-in: the step under test ends with the averaged gradients."""

    def __init__(self, model):
        self.model = model

    def zero_grad(self):
        self.model.zero_grad()

    def step(self):
        pass


def _finish(ok):
    flag = torch.tensor([1 if ok else 0])
    dist.all_reduce(flag, op=dist.ReduceOp.MIN)
    dist.barrier()
    dist.destroy_process_group()
    sys.exit(0 if int(flag) == 1 else 1)


def main():
    rank, W = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    case = os.environ.get("CASE", "p2n2")
    dist.init_process_group("gloo")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    from oracle import clip_oracle as O
    from clip_event_amd import synthetic as S, distributed as D, engine
    from clip_event_amd.engine import train_step, contrastive_step_losses
    from clip_event_amd.losses import CriterionContrastive, CriterionMultiPositive
    from clip_event_amd.model import build_model

    cfg = O.ClipConfig(128, 64, 2, 128, 32, 20, 512, 128, 2, 3)          # embed dim 128: the fused head
    num_pos, num_neg = {"p2n2": (2, 2)}[case]
    B, K = 2, num_pos + num_neg
    N = W * B
    sd = O.init_params(cfg, 11)
    img_all = S.synthetic_images(N, cfg.image_resolution, seed=5)
    txt_all = S.synthetic_tokens(N * K, cfg.context_length, cfg.vocab_size, seed=6, min_len=2)
    crit = CriterionMultiPositive()

    def shard(lo, hi, r):
        gi, gt, ip = D.global_groups(hi - lo, num_pos, num_neg, device=dev, rank_=r)
        return img_all[lo:hi].to(dev), txt_all[lo * K:hi * K].to(dev), gi, gt, ip

    def model():
        m = build_model({k: v.clone() for k, v in sd.items()}).to(dev)
        m.set_hyps(True, False, False)
        return m

    # count the gathers of a step: features once (as 'ce'), ids once
    gathers = []
    inner = dist.all_gather
    dist.all_gather = lambda *a, **kw: (gathers.append(tuple(a[1].shape)), inner(*a, **kw))[1]
    fused = []
    inner_head = engine.multipos_contrastive_losses
    engine.multipos_contrastive_losses = lambda *a: (fused.append((tuple(a[3].shape), tuple(a[8].shape))), inner_head(*a))[1]

    m = model()
    sync = D.GradSync(m)
    args = shard(rank * B, (rank + 1) * B, rank)
    # the 'ce' step on the same shard: its gathers are the baseline
    yi, yt, ip_ce = D.global_labels(B, 1, K - 1, True, device=dev, rank_=rank)
    train_step(m, CriterionContrastive("ce"), _GradOnly(m), args[0], args[1], yi, yt, ip_ce, grad_sync=sync)
    torch.cuda.synchronize()
    ce_gathers = len(gathers)
    per_step = []
    for it in range(2):           # twice: the second step proves the per-step bookkeeping resets
        before = len(gathers)
        ld = train_step(m, crit, _GradOnly(m), *args, grad_sync=sync)
        per_step.append(gathers[before:])
    torch.cuda.synchronize()
    ok = True
    id_gathers = [[s for s in step if len(s) == 1] for step in per_step]
    if any(len(step) != ce_gathers + 1 for step in per_step) or id_gathers != [[(B + B * K,)]] * 2 or fused != [((N * K, 128), (N * K,))] * 2:
        ok = False
        print(f"[{case}] rank {rank}: 'ce' step gathers {ce_gathers}, multipos steps {per_step}, fused head saw {fused}", flush=True)
    if not ok:
        _finish(False)
    assert not sync.pending and not sync.dirty
    g = m._flat_grad.detach().clone()
    red = D.reduce_dict({k: v.detach() for k, v in ld.items()})
    gmax = g.clone()
    dist.all_reduce(gmax, op=dist.ReduceOp.MAX)
    assert float((gmax - g).abs().max()) == 0.0, "ranks disagree on the averaged gradient"

    if rank == 0:
        with D.local_only():
            m1 = model()
            im, tx, gi, gt, ip = shard(0, N, 0)
            m1.zero_grad()
            ld1 = contrastive_step_losses(m1, crit, im, tx, gi, gt, ip)
            sum(ld1.values()).backward()
            torch.cuda.synchronize()
        if sorted(ld1) != ["loss_i", "loss_t"] or sorted(red) != ["loss_i", "loss_t"]:
            ok = False
        for k in ld1:
            want, got = float(ld1[k]), float(red[k])
            print(f"[{case}] {k}: W-rank mean {got:.6f} vs single-process {want:.6f}", flush=True)
            ok &= abs(got - want) <= 3e-3 * max(1.0, abs(want))
        worst_rel, worst_name = 0.0, ""
        for n, p in m1.named_parameters():
            o = m1._offsets[n]
            a = g[o:o + p.numel()].double()
            b = m1._flat_grad[o:o + p.numel()].double()
            if float(b.norm()) == 0.0:
                if float(a.norm()) != 0.0:
                    ok = False
                    print(f"[{case}] {n}: reference gradient is zero, W-rank is not", flush=True)
                continue
            rel = float((a - b).norm() / b.norm())
            if n == "logit_scale":
                print(f"[{case}] d{n}: W-rank {float(a):.6e} vs single-process {float(b):.6e}", flush=True)
            if rel > worst_rel:
                worst_rel, worst_name = rel, n
        print(f"[{case}] worst gradient rel-L2 {worst_rel:.2e} at {worst_name}", flush=True)
        ok &= worst_rel <= 2e-3
        print(f"[{case}] {'OK' if ok else 'FAILED'}", flush=True)
    _finish(ok)


if __name__ == "__main__":
    main()
