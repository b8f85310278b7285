#!/usr/bin/env python3
"""One rank of the W>1 check of the distillation loss (started by tests/test_distill_gpu.py the way tests/test_sigmoid_gpu.py
starts tests/sigmoid_ddp_child.py: gloo backend, every rank on cuda:0).  Each rank runs ``engine.train_step(distill=...)`` on its
shard through the real ``GradSync``: its own rows as queries against the all-gathered student AND teacher features (the student's
pair in the step's one gather with grad, the teacher's pair in one gather without), labels from ``distributed.global_labels``.
Rank 0 then recomputes the step in a single process on the CONCATENATED batch inside ``distributed.local_only()``.

The mean of the ranks' losses must equal the single-process ones, and every parameter's synchronised gradient the single-process
one, at tests/ddp_child.py's bounds: loss 3e-3 max(1, |loss|), worst per-parameter rel-L2 2e-3, zero where the reference is zero.

    CASE=k3 RANK=0 WORLD_SIZE=2 MASTER_ADDR=127.0.0.1 MASTER_PORT=29511 python tests/distill_ddp_child.py
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


def main():
    rank, W = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    case = os.environ.get("CASE", "k1")
    dist.init_process_group("gloo")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    from oracle import clip_oracle as O
    from clip_event_amd import synthetic as S, distributed as D, engine
    from clip_event_amd.engine import Distillation, train_step
    from clip_event_amd.losses import CriterionContrastive
    from clip_event_amd.model import build_model

    cfg = O.ClipConfig(128, 64, 2, 128, 32, 20, 512, 128, 2, 3)          # student: embed dim 128
    tcfg = O.ClipConfig(256, 64, 2, 128, 32, 20, 512, 128, 2, 3)         # teacher: embed dim 256
    B, K = 3, {"k1": 1, "k3": 3, "k3g": 3}[case]
    general = case.endswith("g")             # logits + CriterionDistill across the ranks instead of the fused head
    N = W * B
    sd, tsd = O.init_params(cfg, 11), O.init_params(tcfg, 12)
    img_all = S.synthetic_images(N, cfg.image_resolution, seed=5)
    txt_all = S.synthetic_tokens(N * K, cfg.context_length, cfg.vocab_size, seed=6, min_len=2)
    crit = CriterionContrastive("ce")
    keys = ["loss_dist_i", "loss_dist_t", "loss_i", "loss_t"]

    def shard(lo, hi, r):
        yi, yt, ip = D.global_labels(hi - lo, 1, K - 1, True, device=dev, rank_=r)
        return img_all[lo:hi].to(dev), txt_all[lo * K:hi * K].to(dev), yi, yt, ip

    def model(state=sd):
        m = build_model({k: v.clone() for k, v in state.items()}).to(dev)
        m.set_hyps(True, False, False)
        return m

    distill = Distillation(model(tsd), weight=0.5)

    # the exchanges: the student's pair once per step (with grad), the teacher's pair once (without)
    gathered = []
    inner = D.gather_feature_pair
    D.gather_feature_pair = lambda fi, ft: (gathered.append((tuple(fi.shape), fi.requires_grad)), inner(fi, ft))[1]
    fused = []
    inner_head = engine.distill_losses
    engine.distill_losses = lambda *a: (fused.append((tuple(a[3].shape), tuple(a[8].shape))), inner_head(*a))[1]
    os.environ["CE_FUSED_HEAD"] = "0" if general else "1"       # (the 'ce' head follows: one gather serves both losses either way)

    m = model()
    sync = D.GradSync(m)
    args = shard(rank * B, (rank + 1) * B, rank)
    for it in range(2):           # twice: the second step proves the per-step bookkeeping resets
        ld = train_step(m, crit, _GradOnly(m), *args, grad_sync=sync, distill=distill)
    torch.cuda.synchronize()
    ok = True
    if gathered != [((B, 128), True), ((B, 256), False)] * 2 or fused != ([] if general else [((N * K, 128), (N * K, 256))] * 2):
        ok = False
        print(f"[{case}] rank {rank}: gathered {gathered}, fused head saw keys {fused}", flush=True)
    assert not sync.pending and not sync.dirty
    g = m._flat_grad.detach().clone()
    red = D.reduce_dict({k: v.detach() for k, v in ld.items()})
    gmax = g.clone()
    dist.all_reduce(gmax, op=dist.ReduceOp.MAX)
    assert float((gmax - g).abs().max()) == 0.0, "ranks disagree on the averaged gradient"

    if rank == 0:
        with D.local_only():
            m1 = model()
            im, tx, yi, yt, ip = shard(0, N, 0)
            ld1 = train_step(m1, crit, _GradOnly(m1), im, tx, yi, yt, ip, distill=distill)
            torch.cuda.synchronize()
        if sorted(ld1) != keys or sorted(red) != keys:
            ok = False
        for k in keys:
            want, got = float(ld1[k]), float(red[k])
            print(f"[{case}] {k}: W-rank mean {got:.6f} vs single-process {want:.6f}", flush=True)
            ok &= abs(got - want) <= 3e-3 * max(1.0, abs(want))
        ok &= float(ld1["loss_dist_i"]) > 0
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
        for n, p in distill.teacher.named_parameters():
            ok &= p.grad is None
        print(f"[{case}] {'OK' if ok else 'FAILED'}", flush=True)
    flag = torch.tensor([1 if ok else 0])
    dist.all_reduce(flag, op=dist.ReduceOp.MIN)
    dist.barrier()
    dist.destroy_process_group()
    sys.exit(0 if int(flag) == 1 else 1)


if __name__ == "__main__":
    main()
