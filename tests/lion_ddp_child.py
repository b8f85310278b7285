#!/usr/bin/env python3
"""One rank of the W>1 check of ``optim.FusedLion`` (started by tests/test_lion_gpu.py the way tests/test_sgd_gpu.py starts
tests/sgd_ddp_child.py: gloo backend, every rank on cuda:0).  Each rank runs two ``engine.train_step``s on its shard through the
real ``GradSync`` with FusedLion -- CASE=allreduce: averaged gradients, every rank updates everything; CASE=sharded
(CE_SHARDED_ADAM=1 in the environment): clip + Lion on the own shards, all-gather of the masters, the momentum stays sharded
until ``consolidate``.

A Lion master moves by lr against a sign, so "equal" is the rule of tests/test_lion_ops.StockLion (see tests/test_lion_gpu.py):
given the SAME gradients, two evaluations agree to the last roundings except where the sign is ambiguous.  The gradient every
``step()`` consumed is recorded (over gloo every rank holds the whole mean gradient: gloo has no reduce-scatter, the pieces are
all-reduced), and rank 0 then checks

  * the ranks' masters against the stock loop over those gradients (StockLion.check);
  * against a single process on the CONCATENATED batch inside ``distributed.local_only()``, in two parts.  Its own gradients --
    what the batch decides -- agree with the ranks' per parameter within rel-L2 2e-3 and in norm within 1e-2, the bounds of
    tests/ddp_child.py / tests/sgd_ddp_child.py on exactly these quantities.  Its update -- what the optimiser path decides: one
    process, no shards, ``ce_lion_step_tiles`` over everything -- is then made from the ranks' gradients and must leave the
    ranks' masters bit for bit outside the ambiguous elements (the two sides sum the squares in different orders, nothing else
    differs), and the same momentum up to the clip coefficient's last bits;

and every rank checks that all ranks hold the same masters and momentum.  CASE=sharded also checks the refusals: parameter
groups, a frozen parameter and the weight EMA raise NotImplementedError on the sharded path.

    CASE=allreduce RANK=0 WORLD_SIZE=2 MASTER_ADDR=127.0.0.1 MASTER_PORT=29511 python tests/lion_ddp_child.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.distributed as dist

LR, WD = 2.0 ** -10, 2.0 ** -3            # lr x wd = 2^-13: the stock p (1 - lr wd) and the kernel's p - (lr wd) p round alike


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
    from clip_event_amd.optim import FusedLion, no_decay_groups
    from tests.test_lion_ops import B1, B2, StockLion

    cfg = O.ClipConfig(64, 64, 4, 128, 32, 20, 512, 128, 2, 3)
    B, N = 3, W * 3
    sd = O.init_params(cfg, 11)
    img_all = S.synthetic_images(N, cfg.image_resolution, seed=5)
    txt_all = S.synthetic_tokens(N, cfg.context_length, cfg.vocab_size, seed=6, min_len=2)
    crit = CriterionContrastive("ce")

    def shard(lo, hi, r):
        yi, yt, ip = D.global_labels(hi - lo, 1, 0, True, device=dev, rank_=r)
        return img_all[lo:hi].to(dev), txt_all[lo:hi].to(dev), yi, yt, ip

    def run(args, sync, replay=None):
        """Two steps; returns the gradients every ``step()`` found in the flat buffer.  ``replay``: gradients to put in their place
        before the update (the found ones are still returned)."""
        m = build_model({k: v.clone() for k, v in sd.items()}).to(dev)
        m.set_hyps(True, False, False)
        gs = D.GradSync(m) if sync else None                   # sharded or not: CE_SHARDED_ADAM, as a training job selects it
        opt = FusedLion(m, lr=LR, betas=(B1, B2), weight_decay=WD, max_norm=1.0)
        tape, norms = [], []
        inner = opt.step

        def step(closure=None):
            tape.append(m._flat_grad.detach().clone())
            if replay is not None:
                m._flat_grad.copy_(replay[len(tape) - 1])
            return inner(closure)

        opt.step = step
        for _ in range(2):
            train_step(m, crit, opt, *args, grad_sync=gs)
            torch.cuda.synchronize()
            norms.append(float(opt.grad_norm()))
        del opt.step
        return m, opt, gs, tape, norms

    m, opt, sync, tape, norms = run(shard(rank * B, (rank + 1) * B, rank), True)
    assert (sync.plan is not None) == (case == "sharded"), "CE_SHARDED_ADAM did not select the expected exchange"
    assert not sync.pending and not sync.dirty
    ok = True
    if case == "sharded":
        try:
            opt.state_dict()
            raise AssertionError("state_dict() of a sharded momentum did not refuse")
        except RuntimeError as e:
            assert "consolidate" in str(e)
        D.consolidate(m, opt)
        assert set(opt.state_dict()["state"][0]) == {"exp_avg"}
    assert not m._mirror_fresh if case == "sharded" else m._mirror_fresh
    # every rank holds the same masters and (after consolidate) the same momentum: bit for bit after the sharded step (one all-reduced
    # norm, every element updated by ONE rank).  After the replicated update each rank has summed the squares of the same gradient
    # in its own order of float atomics, so the clip coefficients differ in their last bits: the momentum within (blocks + 16) 2^-24
    # (tests/sgd_ddp_child.py), the masters bit for bit except where that flipped a sign -- at most 1e-4 of the elements
    blocks = min(2048, (m._flat.numel() + 1023) // 1024)
    for what, t in (("masters", m._flat.detach()), ("momentum", opt.exp_avg)):
        mx = t.clone()
        dist.all_reduce(mx, op=dist.ReduceOp.MAX)
        if case == "sharded":
            ok &= bool(torch.equal(mx, t))
        elif what == "masters":
            share = float((mx != t).float().mean())
            print(f"[{case}] rank {rank} masters that differ from the element-wise maximum over the ranks: share {share:.2e}", flush=True)
            ok &= share <= 1e-4
        else:
            rel = float((mx - t).norm() / t.norm())
            print(f"[{case}] rank {rank} momentum against the element-wise maximum over the ranks: rel-L2 {rel:.3e}", flush=True)
            ok &= rel <= (blocks + 16) * 2.0 ** -24
    if rank == 0:
        named = list(m.named_parameters())

        def by_name(flat):
            return {n: flat[m._offsets[n]: m._offsets[n] + p.numel()].view(p.shape) for n, p in named}

        # 1. the stock loop over the gradients the ranks' steps consumed
        stock = StockLion({n: sd[n].to(dev) for n, _ in named}, LR, (B1, B2), WD, 1.0)
        for g, gn in zip(tape, norms):
            norm = stock.step(by_name(g))
            ok &= norm > 1.0 and abs(gn - norm) <= 1e-4 * norm          # (> 1: the clip is active)
        try:
            stock.check(f"{case}: ranks vs stock loop", {n: p.detach() for n, p in named})
        except AssertionError as e:
            ok = False
            print(f"[{case}] {e}", flush=True)
        # 2. a single process on the concatenated batch: its own gradients, and its update from the ranks' gradients
        with D.local_only():
            m1, opt1, _, tape1, norms1 = run(shard(0, N, 0), False, replay=tape)
        for k in range(2):
            worst = (0.0, "")
            a, b = by_name(tape[k]), by_name(tape1[k])
            for n, _ in named:
                if float(b[n].norm()) == 0.0:
                    if float(a[n].norm()) != 0.0:
                        ok = False
                        print(f"[{case}] step {k} {n}: no gradient in the single process, one on the ranks", flush=True)
                    continue
                r = float((a[n].double() - b[n].double()).norm() / b[n].double().norm())
                if r > worst[0]:
                    worst = (r, n)
            gn1 = float(tape1[k].double().norm())
            print(f"[{case}] step {k}: worst per-parameter rel-L2 of the gradient, W ranks vs concatenated batch, {worst[0]:.3e} at "
                  f"{worst[1]}; gradient norm {norms[k]:.6f} vs {gn1:.6f}", flush=True)
            ok &= worst[0] <= 2e-3 and abs(norms[k] - gn1) <= 1e-2 * gn1
        flagged = torch.zeros(m._flat.numel(), dtype=torch.bool, device=dev)
        live = torch.zeros_like(flagged)
        for n, p in named:
            o = m._offsets[n]
            flagged[o:o + p.numel()] = stock.flagged[n].flatten() > 0
            live[o:o + p.numel()] = True
        differ = (m._flat != m1._flat) & live
        print(f"[{case}] masters, W ranks vs one process on the same gradients: {int(differ.sum())} elements differ, "
              f"{int((differ & ~flagged).sum())} of them outside the {int(flagged.sum())} ambiguous ones", flush=True)
        ok &= int((differ & ~flagged).sum()) == 0
        rel = float((opt.exp_avg[live] - opt1.exp_avg[live]).norm() / opt1.exp_avg[live].norm())
        print(f"[{case}] momentum, W ranks vs one process on the same gradients: rel-L2 {rel:.3e}", flush=True)
        ok &= rel <= (blocks + 16) * 2.0 ** -24 + 2.0 ** -19
    if case == "sharded":
        # what the sharded path does not take
        refused = 0
        for attempt in ("groups", "frozen", "ema"):
            try:
                if attempt == "groups":
                    FusedLion(m, lr=LR, weight_decay=WD, groups=no_decay_groups(m, WD))
                elif attempt == "frozen":
                    m.logit_scale.requires_grad_(False)
                    try:
                        FusedLion(m, lr=LR)
                    finally:
                        m.logit_scale.requires_grad_(True)
                else:
                    opt.enable_ema(0.5)
                    try:
                        opt.step()
                    finally:
                        opt.disable_ema()
            except NotImplementedError as e:
                refused += "sharded" in str(e)
        print(f"[{case}] rank {rank}: {refused} of 3 refusals", flush=True)
        ok &= refused == 3
    flag = torch.tensor([1.0 if ok else 0.0])
    dist.all_reduce(flag, op=dist.ReduceOp.MIN)
    if rank == 0:
        print(f"[{case}] {'OK' if float(flag) == 1.0 else 'FAILED'}", flush=True)
    dist.barrier()
    dist.destroy_process_group()
    sys.exit(0 if float(flag) == 1.0 else 1)


if __name__ == "__main__":
    main()
