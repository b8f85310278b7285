"""CPU (no GPU): argument validation of the six ``ce_lion_step*`` entry points before any launch, the host-side surface of
``optim.FusedLion`` / ``build_optimizer``, the fp64 restatement ``lion_ref`` of tests/test_lion_ops.py against a plain fp32 torch
statement of the published algorithm, the entry points ``FusedLion.step()`` takes on each of its paths, and the sharded optimiser
step with Lion callbacks on the two-rank gloo stand-in of tests/test_distributed_cpu.py."""
import os
import types
from ctypes import c_float, c_int, c_long, c_void_p

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests.test_distributed_cpu import _FlatStandIn, _free_port
from tests.test_embed_optim_ops import LR as OP_LR, MAX_NORM as OP_MAX_NORM, U
from tests.test_lion_ops import B1, B2, LION_GRID, _lion_bounds, _lion_state, ambiguous, lion_ref

EINVAL = -22
FAKE = c_void_p(0x1000)           # a non-NULL pointer: a call that passed validation would launch on it (and fail: no device)
NULL = c_void_p(0)


def _group_array(rows):
    from clip_event_amd.optim import OptimGroup
    return (OptimGroup * len(rows))(*[OptimGroup(lr, wd, 0, 0) for lr, wd in rows])


def _call(cl, form, ema, n=8, m=1, b1=0.9, b2=0.99, lr=0.1, wd=0.0, tables=True, groups=((0.1, 0.0),), ngroups=None, e=1, rate=0.1):
    """One of the six entry points on fake pointers, one argument made invalid by the caller."""
    name = "ce_lion_step" + {"flat": "", "tiles": "_tiles", "groups": "_groups"}[form] + ("_ema" if ema else "")
    args = [FAKE, FAKE, FAKE if m else NULL, FAKE]
    if form == "flat":
        args.append(c_long(n))
    else:
        args += [FAKE if tables else NULL, c_int(1 if tables else 0), c_int(1 if tables else 0), FAKE if tables else NULL,
                 c_int(1 if tables else 0)]
        if form == "groups":
            args.append(NULL)
    args += [None, c_float(1.0)]
    if form == "groups":
        arr = _group_array(groups) if groups else None
        args += [arr, c_int(len(groups or ()) if ngroups is None else ngroups), c_float(b1), c_float(b2)]
    else:
        args += [c_float(lr), c_float(b1), c_float(b2), c_float(wd)]
    if ema:
        args += [FAKE if e else NULL, c_float(rate)]
    return name, getattr(cl, name)(*args, None)


def test_lion_argument_errors_are_reported_without_a_gpu():
    """Every invalid-argument case of all six entry points returns -EINVAL and a message of its own that names the entry point;
    validation comes before any launch, so nothing is launched on the fake pointers."""
    from clip_event_amd._lib import lib
    cl = lib()
    nan = float("nan")
    for ema in (False, True):
        cases = [
            ("flat", dict(n=0), b"n>0"),
            ("flat", dict(n=-4), b"n>0"),
        ]
        for form in ("flat", "tiles", "groups"):
            cases += [
                (form, dict(m=0), b"momentum buffer m is NULL"),
                (form, dict(b1=1.0), b"invalid beta1"),
                (form, dict(b1=-0.1), b"invalid beta1"),
                (form, dict(b1=nan), b"invalid beta1"),
                (form, dict(b2=1.0), b"invalid beta2"),
                (form, dict(b2=-0.5), b"invalid beta2"),
            ]
            if form != "groups":
                cases += [(form, dict(lr=-1e-3), b"invalid learning rate"), (form, dict(wd=-0.1), b"invalid weight_decay")]
            if form != "flat":
                cases.append((form, dict(tables=False), b"nothing to update"))
        cases += [
            ("groups", dict(groups=None, ngroups=1), b"need 1..8 groups"),
            ("groups", dict(ngroups=0), b"need 1..8 groups"),
            ("groups", dict(groups=((0.1, 0.0),) * 9), b"need 1..8 groups"),
            ("groups", dict(groups=((0.1, 0.0), (-0.1, 0.0))), b"invalid learning rate"),
            ("groups", dict(groups=((0.1, -1.0), (0.1, 0.0))), b"invalid weight_decay"),
        ]
        if ema:
            for form in ("flat", "tiles", "groups"):
                cases += [(form, dict(e=0), b"ema is NULL"), (form, dict(rate=0.0), b"ema_rate"), (form, dict(rate=1.5), b"ema_rate"),
                          (form, dict(rate=nan), b"ema_rate")]
        for i, (form, bad, msg) in enumerate(cases):
            name, rc = _call(cl, form, ema, **bad)
            assert rc == EINVAL, (name, bad, rc)
            err = cl.ce_last_error()
            assert msg in err and name.encode() + b":" in err, (name, bad, err)


# ---- host surface -----------------------------------------------------------------------------------------------------------------

class _Stub(torch.nn.Module):
    """Two parameters over flat buffers, with what ``_FusedFlatOptimizer`` touches of the model outside a launch."""

    def __init__(self):
        super().__init__()
        self.a = torch.nn.Parameter(torch.zeros(4, 3))
        self.b = torch.nn.Parameter(torch.zeros(5))
        self._flat, self._flat_grad = torch.zeros(24), torch.zeros(24)
        self._flat16 = torch.zeros(24, dtype=torch.bfloat16)
        self._offsets = {"a": 0, "b": 16}

    def _ready(self):
        pass


def test_fused_lion_host_surface():
    """Constructor rules are torch-style ``ValueError``s; the group keys are lr / betas / weight_decay; ``build_optimizer``
    returns the fused step for 'lion' (betas from the configuration when it has them), refuses ``fused=False`` with a message
    that says torch ships no Lion, and keeps 'sgd', 'adam' and the error for unknown names."""
    from clip_event_amd.optim import FusedAdam, FusedLion, FusedSGD, build_optimizer
    m = _Stub()
    opt = FusedLion(m)
    assert isinstance(opt, torch.optim.Optimizer)
    assert {k: v for k, v in opt.param_groups[0].items() if k != "params"} == {"lr": 1e-4, "betas": (0.9, 0.99), "weight_decay": 0.0}
    assert opt.max_norm == 1.0 and FusedLion(m, max_norm=None).max_norm is None
    opt = FusedLion(m, lr=3e-5, betas=[0.95, 0.98], weight_decay=0.3)
    assert (opt.lr, opt.betas, opt.weight_decay) == (3e-5, (0.95, 0.98), 0.3)
    assert len(opt.state_buffers()) == 1 and opt.state_buffers()[0].shape == m._flat.shape
    for bad in (dict(lr=-1.0), dict(betas=(1.0, 0.99)), dict(betas=(-0.1, 0.99)), dict(betas=(0.9, 1.0)), dict(betas=(0.9, -1.0)),
                dict(betas=(0.9,)), dict(weight_decay=-1.0)):
        with pytest.raises(ValueError):
            FusedLion(m, **bad)
    grouped = _Stub()
    grouped.trainable_plan = lambda *a, **k: None
    with pytest.raises(ValueError, match="may set"):
        FusedLion(grouped, groups=[{"params": ["a"], "betas": (0.5, 0.5)}])          # betas are shared by all groups
    with pytest.raises(ValueError):
        FusedLion(grouped, groups=[{"params": ["a"], "lr": -1.0}])
    two = FusedLion(grouped, weight_decay=0.2, groups=[{"params": ["b"], "weight_decay": 0.0}])
    assert [(g["lr"], g["betas"], g["weight_decay"], len(g["params"])) for g in two.param_groups] == \
        [(1e-4, (0.9, 0.99), 0.2, 1), (1e-4, (0.9, 0.99), 0.0, 1)]
    with pytest.raises(RuntimeError, match="closure"):
        opt.step(closure=lambda: 0.0)
    cfg = {"optimizer": "lion", "lr": 2e-5, "weight_decay": 0.1, "momentum": 0.9}
    built = build_optimizer(cfg, m)
    assert type(built) is FusedLion and built.max_norm == 1.0
    assert (built.lr, built.betas, built.weight_decay) == (2e-5, (0.9, 0.99), 0.1)
    assert build_optimizer(dict(cfg, betas=(0.95, 0.98)), m).betas == (0.95, 0.98)
    with pytest.raises(NotImplementedError, match="torch ships no Lion"):
        build_optimizer(cfg, m, fused=False)
    assert type(build_optimizer(dict(cfg, optimizer="sgd"), m)) is FusedSGD
    assert type(build_optimizer(dict(cfg, optimizer="adam"), m)) is FusedAdam
    with pytest.raises(RuntimeError, match="Invalid optimizer 'lamb'"):
        build_optimizer(dict(cfg, optimizer="lamb"), m)
    m.b.requires_grad_(False)
    with pytest.raises(NotImplementedError, match="trainable_plan"):
        FusedLion(m)


def test_fused_lion_state_dict_round_trip():
    """``state_dict()`` is empty before the first step and afterwards holds ``{"exp_avg": tensor}`` per parameter in the parameter's
    shape, with the group keys lr / betas / weight_decay; it loads into a fresh FusedLion (momentum bit for bit, hyper-parameters
    adopted, layout padding left at zero); the empty state loads as the initial state; a state in which only some parameters
    carry an ``exp_avg`` is refused."""
    from clip_event_amd.optim import FusedLion
    m = _Stub()
    opt = FusedLion(m, lr=3e-5, betas=(0.95, 0.98), weight_decay=0.3)
    empty = opt.state_dict()
    assert empty["state"] == {} and empty["param_groups"] == [{"lr": 3e-5, "betas": (0.95, 0.98), "weight_decay": 0.3, "params": [0, 1]}]
    opt.exp_avg.copy_(torch.arange(24.0) + 1)          # what a step leaves: a momentum, and the note that there is one
    opt._after_step(False)
    sd = opt.state_dict()
    assert set(sd["state"]) == {0, 1} and all(set(st) == {"exp_avg"} for st in sd["state"].values())
    assert torch.equal(sd["state"][0]["exp_avg"], (torch.arange(12.0) + 1).view(4, 3))
    assert torch.equal(sd["state"][1]["exp_avg"], torch.arange(5.0) + 17)
    sd["state"][0]["exp_avg"].zero_()                   # a copy: the optimiser's buffer is not aliased
    assert float(opt.exp_avg[0]) == 1.0
    sd = opt.state_dict()
    opt2 = FusedLion(_Stub())
    opt2.load_state_dict(sd)
    assert {k: v for k, v in opt2.param_groups[0].items() if k != "params"} == {"lr": 3e-5, "betas": (0.95, 0.98), "weight_decay": 0.3}
    want = torch.zeros(24)
    want[:12], want[16:21] = torch.arange(12.0) + 1, torch.arange(5.0) + 17
    assert torch.equal(opt2.exp_avg, want)
    again = opt2.state_dict()
    assert all(torch.equal(again["state"][i]["exp_avg"], sd["state"][i]["exp_avg"]) for i in (0, 1))
    partial = opt.state_dict()
    del partial["state"][1]
    with pytest.raises(ValueError, match="exp_avg"):
        opt2.load_state_dict(partial)
    assert torch.equal(opt2.exp_avg, want)                              # a refused state changes nothing
    opt2.load_state_dict(empty)
    assert opt2.state_dict()["state"] == {} and not bool(opt2.exp_avg.any())
    with pytest.raises(ValueError, match="does not match"):
        opt2.load_state_dict({"state": {}, "param_groups": [dict(empty["param_groups"][0], params=[0])]})


# ---- lion_ref against the published algorithm -------------------------------------------------------------------------------------

def _torch_lion(param, m, lr, wd, b1, b2):
    """The three lines of the published algorithm (lion-pytorch's update_fn; timm's has the same arithmetic) in fp32."""
    g = param.grad
    param.data.mul_(1 - lr * wd)
    param.data.add_(torch.sign(m * b1 + g * (1 - b1)), alpha=-lr)
    m.lerp_(g, 1 - b2)


def _stock_lions():
    """Whatever stock Lion happens to be importable: (name, constructor) pairs.  None is required."""
    found = []
    try:
        from timm.optim import Lion as TimmLion
        found.append(("timm", lambda ps, **kw: TimmLion(ps, foreach=False, **kw)))
    except Exception:
        pass
    try:
        from lion_pytorch import Lion as LionPytorch
        found.append(("lion_pytorch", lambda ps, **kw: LionPytorch(ps, **kw)))
    except Exception:
        pass
    return found


def test_lion_reference_matches_the_published_algorithm():
    """CPU cross-check of the fp64 restatement: ``clip_grad_norm_`` + ``p.mul_(1 - lr wd); p.add_(sign(m b1 + g (1 - b1)),
    alpha=-lr); m.lerp_(g, 1 - b2)`` on fp32 copies land within the kernel's bounds of lion_ref over the whole grid, n = 999: the
    sign agrees on every element that is not ambiguous (none is), the momentum is within 2^-20 of its terms.  (p (1 - lr wd)
    rounds 1 - lr wd once where the kernel rounds lr wd and the product: one more U |p|, inside the 2 U |p| of the bound.)  A
    stock Lion (timm, lion-pytorch) is compared the same way when one is importable."""
    worst = {"p": 0.0, "m": 0.0}
    stocks = _stock_lions()
    print(f"[lion_ref] stock implementations found: {[name for name, _ in stocks] or 'none'}")
    for clip, wd, step in LION_GRID:
        p0, g0, m0, sumsq = _lion_state(999, step, clip, 5)
        ref = lion_ref(p0, g0, m0, sumsq, wd)
        assert int(ambiguous(ref).sum()) == 0, (clip, wd, step)
        bp, bm = _lion_bounds(ref, wd)
        runs = []
        param = torch.nn.Parameter(p0.clone())
        param.grad = g0.clone()
        if sumsq is not None:
            torch.nn.utils.clip_grad_norm_([param], OP_MAX_NORM)
        m = m0.clone()
        _torch_lion(param, m, OP_LR, wd, B1, B2)
        runs.append(("three lines", param.detach(), m))
        for name, make in stocks:
            param = torch.nn.Parameter(p0.clone())
            param.grad = g0.clone()
            if sumsq is not None:
                torch.nn.utils.clip_grad_norm_([param], OP_MAX_NORM)
            opt = make([param], lr=OP_LR, betas=(B1, B2), weight_decay=wd)
            if step > 1:
                opt.state[param]["exp_avg"] = m0.clone()
            opt.step()
            runs.append((name, param.detach(), opt.state[param]["exp_avg"]))
        for name, p, m in runs:
            for what, got, want, bound in (("p", p, ref[0], bp), ("m", m, ref[1], bm)):
                err = (got.double() - want).abs()
                ratio = float((err / bound.clamp_min(1e-300)).max())
                worst[what] = max(worst[what], ratio)
                assert bool((err <= bound).all()), (name, clip, wd, step, what, ratio)
    print(f"[lion_ref vs torch] worst |err| / bound: p {worst['p']:.3f}, m {worst['m']:.3f}")


def test_ambiguity_count_is_zero_over_the_op_grids():
    """The condition the GPU tests assert case by case, checked here for the generator and seeds they use (flat: seed n + step;
    tiles: 77 + step; forms: 300 + step) at the sizes a CPU run affords: no element has |c| <= 2^-20 (b1 |m| + (1 - b1) |gc|), and
    an fp32 evaluation of c -- every product and the sum rounded on their own, as the kernel does -- never disagrees in sign
    with fp64."""
    f32 = torch.float32
    for n, seeds in ((5, (5,)), (7171, (7171,)), (25711, (300,)), (25716, (77,))):
        for clip, wd, step in LION_GRID:
            for base in seeds:
                p0, g0, m0, sumsq = _lion_state(n, step, clip, base + step)
                ref = lion_ref(p0, g0, m0, sumsq, wd)
                assert int(ambiguous(ref).sum()) == 0, (n, clip, wd, step)
                coef = torch.tensor(1.0 if sumsq is None else min(1.0, OP_MAX_NORM / (float(torch.tensor(sumsq, dtype=f32).sqrt()) + 1e-6)),
                                    dtype=f32)
                gc = g0 * coef
                c32 = m0 * torch.tensor(B1, dtype=f32) + gc * torch.tensor(1 - B1, dtype=f32)
                assert torch.equal(torch.sign(c32).double(), torch.sign(ref[3])), (n, clip, wd, step)


# ---- step(): which entry points each path takes (a recording library, no GPU) -------------------------------------------------------

class _FlatModel(_Stub):
    """_Stub plus the hooks around the update, a tile table and an optional ``grad_sync.plan``."""

    def __init__(self, plan=None, tiles=False):
        super().__init__()
        self.grad_sync = types.SimpleNamespace(plan=plan)
        self._adam_tiles_ok = tiles
        self._tjobs_bwd = (torch.zeros(1), 1, 1)
        self.polls, self.stale = 0, []

    def _adam_segment_table(self):
        return torch.zeros(2, 2, dtype=torch.int64)

    def _settle_first_touch(self):
        pass

    def wait_transposes(self):
        pass

    def mark_operands_stale(self, **kw):
        self.stale.append(kw)

    def poll_stream16_saturation(self):
        self.polls += 1


class _RecordingLib:
    """Stands in for the shared library: every entry point records its name and argument count and succeeds."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append((name, len(args)))
            return 0
        return entry


@pytest.fixture
def recording(monkeypatch):
    from clip_event_amd import optim
    fake = _RecordingLib()
    monkeypatch.setattr(optim, "lib", lambda: fake)
    monkeypatch.setattr(optim, "stream", lambda: None)
    return fake


def test_fused_lion_step_takes_the_lion_entry_points(recording):
    """``FusedLion.step()`` goes through ``ce_lion_step_tiles`` when the model's block weights tile, ``ce_lion_step`` otherwise, their
    ``_ema`` twins once ``enable_ema`` was called, no ``ce_sumsq`` with ``max_norm=None``; the argument counts are those of the
    header; the state dict is no longer empty afterwards."""
    from clip_event_amd import optim
    for tiles, flat_name, nargs in ((False, "ce_lion_step", 12), (True, "ce_lion_step_tiles", 16)):
        m = _FlatModel(tiles=tiles)
        opt = optim.FusedLion(m, weight_decay=0.1)
        opt.step()
        assert recording.calls == [("ce_sumsq", 4), (flat_name, nargs)], recording.calls
        assert m.stale == [dict(mirror_fresh=True, wt_fresh=True) if tiles else dict(mirror_fresh=True)]
        assert set(opt.state_dict()["state"]) == {0, 1}
        recording.calls.clear()
        opt.enable_ema(0.99)
        opt.step()
        assert recording.calls == [("ce_sumsq", 4), (flat_name + "_ema", nargs + 2)] and opt.ema_updates == 1
        recording.calls.clear()
        opt.disable_ema()
        opt.max_norm = None
        opt.step()
        assert recording.calls == [(flat_name, nargs)]
        recording.calls.clear()


def test_sharded_lion_step_and_its_refusals(recording, monkeypatch):
    """With a ``grad_sync.plan`` and the collectives active, ``step()`` hands ``distributed.sharded_update`` range callbacks that go
    through ``ce_sumsq`` / ``ce_lion_step``, marks the mirror stale and the momentum as sharded (``state_dict()`` then asks for
    ``consolidate``), and polls the saturation counters; EMA on the sharded path raises, and so do groups with a plan."""
    from clip_event_amd import distributed as D
    from clip_event_amd import optim
    monkeypatch.setattr(D, "active", lambda: True)
    seen = []

    def sharded_update(plan, params, sumsq, sumsq_fn, update_fn):
        seen.append((plan, params, sumsq))
        sumsq_fn(0, 4)
        update_fn(0, 4)
    monkeypatch.setattr(D, "sharded_update", sharded_update)
    m = _FlatModel(plan=object())
    opt = optim.FusedLion(m)
    opt.sat_poll_every = 1
    opt.step()
    assert m.polls == 1
    assert len(seen) == 1 and all(a is b for a, b in zip(seen[0], (m.grad_sync.plan, m._flat, opt.sumsq)))
    assert recording.calls == [("ce_sumsq", 4), ("ce_lion_step", 12)]
    assert m.stale == [dict(mirror_fresh=False)] and opt._moments_stale
    with pytest.raises(RuntimeError, match="consolidate"):
        opt.state_dict()
    opt.enable_ema(0.99)
    with pytest.raises(NotImplementedError, match="EMA"):
        opt.step()
    m.trainable_plan = lambda *a, **k: None
    with pytest.raises(NotImplementedError, match="sharded"):
        optim.FusedLion(m, groups=[{"params": ["b"], "weight_decay": 0.0}])


# ---- sharded optimiser step with Lion callbacks (distributed.sharded_update, consolidate through state_buffers()) -------------------

LR, WD, MAX_NORM = 0.05, 0.01, 1.0
SB1, SB2 = 0.9, 0.99


def _lion_reference(p, g, m, coef):
    """clip + Lion on views, in place; returns the mask of the elements whose sign is ambiguous (|c| <= 1e-6 of its terms)."""
    g = g * coef
    c = m * SB1 + g * (1 - SB1)
    p.mul_(1 - LR * WD).sub_(LR * torch.sign(c))
    near = c.abs() <= 1e-6 * (m.abs() * SB1 + g.abs() * (1 - SB1))
    m.mul_(SB2).add_(g * (1 - SB2))
    return near


def _sharded_lion_worker(rank, W, port, out):
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
    exp_avg = torch.zeros(n)
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

        def lion_fn(lo, hi):
            coef = min(1.0, MAX_NORM / (float(sumsq.sqrt()) + 1e-6))
            _lion_reference(m._flat[lo:hi], m._flat_grad[lo:hi], exp_avg[lo:hi], coef)
            touched.append((lo, hi))

        D.sharded_update(plan, m._flat, sumsq, sumsq_fn, lion_fn)
        assert sorted(touched) == sorted(owned + [plan.head])
        assert bool(torch.isfinite(m._flat).all())

    class _Opt:
        """An optimiser with ONE flat state buffer and no ``m`` / ``v``: consolidate must go through state_buffers()."""
        _moments_stale = True
        calls = 0

        def state_buffers(self):
            self.calls += 1
            return (exp_avg,)
    opt = _Opt()
    before = exp_avg.clone()
    D.consolidate(m, opt)
    assert opt.calls == 1 and not opt._moments_stale and torch.equal(exp_avg[mine], before[mine])
    gathered = [None] * W
    dist.all_gather_object(gathered, (m._flat, exp_avg, grads))
    if rank == 0:
        torch.save(gathered, out)
    dist.destroy_process_group()


@pytest.mark.timeout(120)
def test_sharded_lion_step_equals_replicated_step(tmp_path):
    """Reduce-scattered gradient pieces + clip / Lion on the own shard of every piece + all-gather of the masters leave every rank
    with the parameters a replicated step (mean gradients, one clip + Lion over everything) produces, and `consolidate` --
    through ``state_buffers()`` -- the single momentum.  Non-owned gradient shards are poisoned before the update.  The two sides
    sum the squares in different orders, so an element whose c is within 1e-6 of zero relative to its terms may take the other
    sign: the replicated side counts those (at most 4 of the stand-in's elements; none occurs) and they are left out of the
    comparison of the masters."""
    W = 2
    out = str(tmp_path / "s.pt")
    mp.spawn(_sharded_lion_worker, args=(W, _free_port(), out), nprocs=W, join=True)
    gathered = torch.load(out, weights_only=False)          # written by this test
    m = _FlatStandIn(tail=4)
    n = m._flat_grad.numel()
    p = torch.randn(n, generator=torch.Generator().manual_seed(5))
    exp_avg = torch.zeros(n)
    near = torch.zeros(n, dtype=torch.bool)
    for step in range(1, 4):
        g = gathered[0][2][step - 1]                           # rank means, identical on both ranks (gloo all-reduces whole pieces)
        assert torch.allclose(g, gathered[1][2][step - 1], atol=1e-7)
        coef = min(1.0, MAX_NORM / (float(g.square().sum().sqrt()) + 1e-6))
        assert coef < 1.0                                      # the clip is active in this stand-in
        near |= _lion_reference(p, g, exp_avg, coef)
    assert int(near.sum()) <= 4
    assert float((p - torch.randn(n, generator=torch.Generator().manual_seed(5))).abs().min()) > 0.5 * LR      # every element stepped
    for r in range(W):
        assert torch.allclose(gathered[r][0][~near], p[~near], atol=1e-6), r
        assert torch.allclose(gathered[r][1], exp_avg, atol=1e-6), r
