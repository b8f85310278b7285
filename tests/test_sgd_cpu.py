"""CPU (no GPU): argument validation of ``ce_sgd_step`` / ``ce_sgd_step_tiles`` before any launch, the host-side surface of
``optim.FusedSGD`` / ``build_optimizer``, and the sharded optimiser step with SGD callbacks on the two-rank gloo stand-in of
tests/test_distributed_cpu.py."""
import os
from ctypes import c_float, c_int, c_long, c_void_p

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests.test_distributed_cpu import _FlatStandIn, _free_port


def _flat(cl, n=8, momentum=0.9, dampening=0.0, nesterov=0, buf=1):
    """``ce_sgd_step`` with fake non-NULL pointers: a call that passed validation would launch on them (and fail: no device)."""
    fake = c_void_p(0x1000)
    return cl.ce_sgd_step(fake, fake, fake if buf else c_void_p(0), fake, c_long(n), None, c_float(1.0), c_float(0.1),
                          c_float(momentum), c_float(dampening), c_float(0.0), c_int(nesterov), c_int(1), None)


def _tiles(cl, njobs=1, tiles=1, nseg=1, momentum=0.9, dampening=0.0, nesterov=0, buf=1, jobs=1, segs=1):
    fake = c_void_p(0x1000)
    return cl.ce_sgd_step_tiles(fake, fake, fake if buf else c_void_p(0), fake, fake if jobs else c_void_p(0), c_int(njobs),
                                c_int(tiles), fake if segs else c_void_p(0), c_int(nseg), None, c_float(1.0), c_float(0.1),
                                c_float(momentum), c_float(dampening), c_float(0.0), c_int(nesterov), c_int(1), None)


def test_sgd_argument_errors_are_reported_without_a_gpu():
    """Every invalid-argument case returns -EINVAL and a message of its own; validation comes before any launch, so nothing
    is launched on the fake pointers."""
    from clip_event_amd._lib import lib
    cl = lib()
    cases = [
        (lambda: _flat(cl, n=0), b"n>0"),
        (lambda: _flat(cl, n=-4), b"n>0"),
        (lambda: _flat(cl, momentum=-0.5), b"invalid momentum"),
        (lambda: _flat(cl, momentum=0.0, nesterov=1), b"nesterov"),
        (lambda: _flat(cl, dampening=0.1, nesterov=1), b"nesterov"),
        (lambda: _flat(cl, buf=0), b"momentum buffer"),
        (lambda: _tiles(cl, momentum=-0.5), b"invalid momentum"),
        (lambda: _tiles(cl, momentum=0.0, nesterov=1), b"nesterov"),
        (lambda: _tiles(cl, dampening=0.1, nesterov=1), b"nesterov"),
        (lambda: _tiles(cl, buf=0), b"momentum buffer"),
        (lambda: _tiles(cl, njobs=0, tiles=0, nseg=0), b"nothing to update"),
        (lambda: _tiles(cl, jobs=0, segs=0), b"nothing to update"),
    ]
    for i, (call, msg) in enumerate(cases):
        rc = call()
        assert rc == -22, (i, rc)
        err = cl.ce_last_error()
        assert msg in err and (b"ce_sgd_step" in err), (i, err)


class _Stub(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.a = torch.nn.Parameter(torch.zeros(4, 3))
        self.b = torch.nn.Parameter(torch.zeros(5))


def test_fused_sgd_host_surface():
    """Constructor rules and group keys are torch.optim.SGD's; frozen parameters are refused; ``build_optimizer`` returns the
    fused step for 'sgd' and keeps the stock one with ``fused=False`` or frozen parameters."""
    from clip_event_amd.optim import FusedAdam, FusedSGD, build_optimizer
    m = _Stub()
    opt = FusedSGD(m, lr=0.1, momentum=0.9, weight_decay=0.01)
    ref = torch.optim.SGD(m.parameters(), lr=0.1, momentum=0.9, weight_decay=0.01)
    assert isinstance(opt, torch.optim.Optimizer)
    assert {k: v for k, v in opt.param_groups[0].items() if k != "params"} == {k: v for k, v in ref.param_groups[0].items() if k != "params"}
    assert opt.lr == 0.1 and opt.momentum == 0.9 and opt.weight_decay == 0.01 and opt.max_norm == 1.0
    for bad in (dict(lr=-1.0), dict(momentum=-0.1), dict(weight_decay=-1.0), dict(momentum=0.0, nesterov=True),
                dict(momentum=0.9, dampening=0.1, nesterov=True)):
        with pytest.raises(ValueError):
            FusedSGD(m, **{"lr": 0.1, **bad})
    with pytest.raises(RuntimeError, match="closure"):
        opt.step(closure=lambda: 0.0)
    cfg = {"optimizer": "sgd", "lr": 0.1, "momentum": 0.9, "weight_decay": 0.01}
    built = build_optimizer(cfg, m)
    assert type(built) is FusedSGD and built.max_norm == 1.0
    assert (built.lr, built.momentum, built.weight_decay) == (0.1, 0.9, 0.01)
    assert type(build_optimizer(cfg, m, fused=False)) is torch.optim.SGD
    assert type(build_optimizer(dict(cfg, optimizer="adam"), m)) is FusedAdam
    m.b.requires_grad_(False)
    with pytest.raises(NotImplementedError):
        FusedSGD(m, lr=0.1)
    stock = build_optimizer(cfg, m)
    assert type(stock) is torch.optim.SGD and len(stock.param_groups[0]["params"]) == 1


# ---- sharded optimiser step with SGD callbacks (distributed.sharded_update, consolidate through state_buffers()) ----------

LR, MU, WD, MAX_NORM = 0.05, 0.9, 0.01, 1.0


def _sgd_reference(p, g, buf, coef, first):
    """clip + torch.optim.SGD(momentum, weight_decay) on views, in place."""
    g = g * coef + WD * p
    if first:
        buf.copy_(g)
    else:
        buf.mul_(MU).add_(g)
    p.sub_(LR * buf)


def _sharded_sgd_worker(rank, W, port, out):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=W)
    from clip_event_amd import distributed as D
    m = _FlatStandIn(tail=4)                                   # every piece splits into two equal shards
    n = m._flat_grad.numel()
    m._flat = torch.randn(n, generator=torch.Generator().manual_seed(5))
    sync = D.GradSync(m, pieces_per_tower=3, sharded=True)
    plan = sync.plan
    owned = plan.owned(rank)
    mine = torch.zeros(n, dtype=torch.bool)
    for lo, hi in owned:
        mine[lo:hi] = True
    mine[0] = True
    buf = torch.zeros(n)
    sumsq = torch.zeros(1)
    grads = []
    for step in range(1, 4):
        m._flat_grad.zero_()
        g = torch.Generator().manual_seed(100 * step + rank)
        contrib = {t: torch.randn(m._ranges[t][1] - m._ranges[t][0], generator=g) for t in ("visual", "text")}
        for t in ("visual", "text"):
            sync.note_forward(t)
        for t in ("text", "visual"):
            m.backward_pass(t, contrib[t])
        m._flat_grad[0] += float(rank + 1)
        sync.finish()
        grads.append(m._flat_grad.clone())
        m._flat_grad[~mine] = float("nan")                     # what a real reduce-scatter leaves outside the own shards: nothing usable
        touched = []

        def sumsq_fn(lo, hi):
            sumsq.add_(m._flat_grad[lo:hi].square().sum())

        def sgd_fn(lo, hi):
            coef = min(1.0, MAX_NORM / (float(sumsq.sqrt()) + 1e-6))
            _sgd_reference(m._flat[lo:hi], m._flat_grad[lo:hi], buf[lo:hi], coef, first=step == 1)
            touched.append((lo, hi))

        D.sharded_update(plan, m._flat, sumsq, sumsq_fn, sgd_fn)
        assert sorted(touched) == sorted(owned + [plan.head])
        assert bool(torch.isfinite(m._flat).all())

    class _Opt:
        """An optimiser with ONE flat state buffer and no ``m`` / ``v``: consolidate must go through state_buffers()."""
        _moments_stale = True
        calls = 0

        def state_buffers(self):
            self.calls += 1
            return (buf,)
    opt = _Opt()
    before = buf.clone()
    D.consolidate(m, opt)
    assert opt.calls == 1 and not opt._moments_stale and torch.equal(buf[mine], before[mine])
    gathered = [None] * W
    dist.all_gather_object(gathered, (m._flat, buf, grads))
    if rank == 0:
        torch.save(gathered, out)
    dist.destroy_process_group()


@pytest.mark.timeout(120)
def test_sharded_sgd_step_equals_replicated_step(tmp_path):
    """Reduce-scattered gradient pieces + clip / SGD on the own shard of every piece + all-gather of the masters leave every
    rank with the parameters a replicated step (mean gradients, one clip + SGD over everything) produces, and `consolidate`
    -- through ``state_buffers()`` -- the single momentum buffer.  Non-owned gradient shards are poisoned before the update."""
    W = 2
    out = str(tmp_path / "s.pt")
    mp.spawn(_sharded_sgd_worker, args=(W, _free_port(), out), nprocs=W, join=True)
    gathered = torch.load(out, weights_only=False)          # written by this test
    m = _FlatStandIn(tail=4)
    n = m._flat_grad.numel()
    p = torch.randn(n, generator=torch.Generator().manual_seed(5))
    buf = torch.zeros(n)
    for step in range(1, 4):
        g = gathered[0][2][step - 1]                           # rank means, identical on both ranks (gloo all-reduces whole pieces)
        assert torch.allclose(g, gathered[1][2][step - 1], atol=1e-7)
        coef = min(1.0, MAX_NORM / (float(g.square().sum().sqrt()) + 1e-6))
        assert coef < 1.0                                      # the clip is active in this stand-in
        _sgd_reference(p, g, buf, coef, first=step == 1)
    for r in range(W):
        assert torch.allclose(gathered[r][0], p, atol=1e-6), r
        assert torch.allclose(gathered[r][1], buf, atol=1e-6), r
