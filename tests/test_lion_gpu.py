"""GPU: ``optim.FusedLion`` (clip + Lion on the HIP path) as a torch optimiser and through ``engine.train_step`` /
``build_optimizer`` -- against a stock loop written here (``tests.test_lion_ops.StockLion``: ``clip_grad_norm_`` plus the three
lines of the published algorithm over the same ``.grad``s), with micro-batches, the first-touch zero-fill, a locked tower and
parameter groups, the weight EMA, a checkpoint, and on two ranks (tests/lion_ddp_child.py).  Tiny configurations of
tests/test_sgd_gpu.py.

Comparing Lion runs.  A master moves by exactly lr against the sign of c = b1 m + (1 - b1) g, so two fp32 evaluations agree to the
last roundings or differ by 2 lr; which one depends on the sign alone.  The stock loop is therefore fed the gradients the fused
step itself consumed (two ``train_step`` runs from one seed do not even give the same gradient bits: float atomics), and the
comparison is ``StockLion.check``: the elements whose sign is ambiguous in fp64 are counted on the stock side (at most 1e-4 of the
parameters), all others must agree within 2 U |p| + 2 U lr per step.  Where a weight decay is used, lr and lr x weight_decay
are powers of two, so that the stock p (1 - lr wd) and the kernel's p - (lr wd) p round the same real number once."""
import numpy as np
import pytest
import torch

from tests.test_ddp_gpu import run_ranks
from tests.test_ema_ops import _ema_bound, ema_ref
from tests.test_lion_ops import B1, B2, StockLion
from tests.test_sgd_gpu import TILES_CFG, _batch, _live, _mk

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LR, WD = 2.0 ** -10, 2.0 ** -3            # lr x wd = 2^-13: 1 - lr wd is an fp32 number
TINY = (64, 64, 2, 128, 32, 20, 512, 128, 2, 2)
LION_CFG = {"optimizer": "lion", "lr": LR, "weight_decay": WD, "betas": (B1, B2)}


def _crit():
    from clip_event_amd.losses import CriterionContrastive
    return CriterionContrastive("ce")


def _grads(m, names=None):
    """The gradients the last backward left in the flat buffer, by name."""
    return {n: m._gview(n).detach().clone() for n, p in m.named_parameters() if names is None or n in names}


def _masters(m):
    return {n: p.detach() for n, p in m.named_parameters()}


def _bits(t):
    return t.detach().contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def test_fused_lion_is_a_torch_optimizer():
    """FusedLion under the reference's driver pattern (engine.py:87-97: zero_grad, backward, step, scheduler.step): the warm-up
    cosine scheduler drives it through ``param_groups[0]['lr']``; the stock loop fed each step's ``.grad``s and the scheduler's
    rate lands on the same masters (StockLion.check) and -- the momentum carries no sign -- on the same momentum within 2^-20 of
    its terms' size per step; the state dict is empty before the first step and then holds one ``exp_avg`` per parameter, and it
    loads into a fresh FusedLion bit for bit."""
    from oracle import clip_oracle as O
    from clip_event_amd.optim import FusedLion, WarmupCosineLR
    cfg = O.ClipConfig(*TINY)
    m, sd = _mk(cfg, 21)
    img, txt, yi, yt, ip = _batch(cfg, 4)
    crit = _crit()
    opt = FusedLion(m, lr=1e-3, betas=(B1, B2), max_norm=1.0)
    assert isinstance(opt, torch.optim.Optimizer)
    assert opt.state_dict()["state"] == {} and opt.state_buffers()[0].numel() == m._flat.numel()
    stock = StockLion({n: sd[n].to(DEV) for n, _ in m.named_parameters()}, 1e-3, (B1, B2), 0.0, 1.0)
    sch = WarmupCosineLR(opt, max_iters=10, warmup_epochs=3)
    lrs = []
    for _ in range(3):
        ld = crit(*m(img, txt), yi, yt, index_pos=ip)
        opt.zero_grad()
        sum(ld.values()).backward()
        lrs.append(opt.param_groups[0]["lr"])
        norm = stock.step({n: p.grad for n, p in m.named_parameters()}, lr=lrs[-1])
        opt.step()
        sch.step()
        torch.cuda.synchronize()
        assert norm > 1.0 and abs(float(opt.grad_norm()) - norm) <= 1e-4 * norm            # the clip is active
    np.testing.assert_allclose(lrs, [O.lr_warmup_cosine(1e-3, i, 10, warmup_epochs=3) for i in range(3)], rtol=1e-12)
    stock.check("driver pattern", _masters(m))
    state = opt.state_dict()
    params = list(m.named_parameters())
    assert set(state) == {"state", "param_groups"} and len(state["state"]) == len(params)
    assert {k for k in state["param_groups"][0] if k not in ("params", "initial_lr")} == {"lr", "betas", "weight_decay"}
    for i, (n, p) in enumerate(params):
        st = state["state"][i]
        assert set(st) == {"exp_avg"} and st["exp_avg"].shape == p.shape
        # each side is within the op-level 2^-20 of the terms' size of the fp64 momentum of the same gradients, per step (an
        # earlier step's error shrinks by b2): 2 sides x 3 steps x 2^-20 x the running size of the terms
        err = (st["exp_avg"].double() - stock.m[n].double()).abs()
        assert bool((err <= 2 * 3 * 2.0 ** -20 * stock.m_mag[n].double()).all()), n
    m2, _ = _mk(cfg, 21)
    opt2 = FusedLion(m2, lr=5e-4, betas=(0.5, 0.5))
    opt2.load_state_dict(state)
    assert opt2.param_groups[0]["lr"] == opt.param_groups[0]["lr"] and opt2.betas == (B1, B2)
    live = _live(m)
    assert torch.equal(_bits(opt2.exp_avg[live]), _bits(opt.exp_avg[live]))


@pytest.mark.parametrize("form", ["tiles", "flat"])
def test_train_step_with_fused_lion_matches_the_stock_loop(form, monkeypatch):
    """Two ``train_step``s with ``build_optimizer({'optimizer': 'lion'})`` (weight decay 2^-3, clip active) against the stock loop
    over the same ``.grad``s: StockLion.check on the masters of every parameter, the mirror the masters' cast.  "tiles": the
    default path (``ce_lion_step_tiles``), which leaves the W^T copies behind too; "flat": CE_ADAM_TILES=0 (``ce_lion_step``)."""
    from oracle import clip_oracle as O
    from clip_event_amd.engine import train_step
    from clip_event_amd.optim import FusedLion, build_optimizer
    monkeypatch.setenv("CE_ADAM_TILES", "1" if form == "tiles" else "0")
    cfg = O.ClipConfig(*TILES_CFG)
    m, sd = _mk(cfg, 17)
    data = _batch(cfg, 6)
    opt = build_optimizer(LION_CFG, m)
    assert type(opt) is FusedLion and opt.max_norm == 1.0 and opt.betas == (B1, B2)
    stock = StockLion({n: sd[n].to(DEV) for n, _ in m.named_parameters()}, LR, (B1, B2), WD, 1.0)
    for it in range(2):
        train_step(m, _crit(), opt, *data)
        torch.cuda.synchronize()
        norm = stock.step(_grads(m))
        print(f"step {it}: gradient norm before the clip: stock {norm:.5f}, fused {float(opt.grad_norm()):.5f}")
        assert norm > 1.0
    assert m._adam_tiles_ok
    stock.check(f"train_step {form}", _masters(m))
    live = _live(m)
    assert torch.equal(_bits(m._flat16[live]), _bits(m._flat[live].to(torch.bfloat16)))
    assert m._mirror_fresh and m._wt_fresh == (form == "tiles")
    if form == "tiles":
        name = "visual.transformer.resblocks.1.mlp.c_fc.weight"
        w = dict(m.named_parameters())[name].detach()
        assert torch.equal(m._w16t[name], w.to(torch.bfloat16).t().contiguous())


def test_chunked_train_step_with_fused_lion_against_the_unchunked_step():
    """``micro_batch=2`` at B = 4, two steps, against the unchunked step of the same build.  What the chunking changes is the
    gradient, so that is where the two runs are compared, at the bounds of the SGD and Adam versions of this test: losses within
    3e-2, gradient norm within 5 %.  The masters of the chunked run are then held to the stock loop over the chunked run's own
    accumulated ``.grad``s (StockLion.check), as the unchunked ones are.  The share of elements on which the two runs took
    different signs -- elements whose c is smaller than the difference between the two gradients -- is printed, not bounded."""
    from oracle import clip_oracle as O
    from clip_event_amd.engine import train_step
    from clip_event_amd.optim import build_optimizer
    from tests.util import golden_json
    cfg = O.ClipConfig(**golden_json()["tiny"]["cfg"])
    data = _batch(cfg, 4)
    runs = {}
    for mb in (None, 2):
        m, sd = _mk(cfg, 11)
        opt = build_optimizer(LION_CFG, m)
        stock = StockLion({n: sd[n].to(DEV) for n, _ in m.named_parameters()}, LR, (B1, B2), WD, 1.0)
        log = []
        for _ in range(2):
            ld = train_step(m, _crit(), opt, *data, micro_batch=mb)
            torch.cuda.synchronize()
            stock.step(_grads(m))
            log.append((float(ld["loss_i"]), float(ld["loss_t"]), float(opt.grad_norm())))
        stock.check(f"micro_batch={mb}", _masters(m))
        runs[mb] = (log, m._flat.detach().clone(), _live(m))
    for (li, lt, gn), (li_r, lt_r, gn_r) in zip(runs[2][0], runs[None][0]):
        print(f"chunked loss_i {li:.5f} loss_t {lt:.5f} grad_norm {gn:.4f}; unchunked {li_r:.5f} {lt_r:.5f} {gn_r:.4f}")
        assert abs(li - li_r) < 3e-2 and abs(lt - lt_r) < 3e-2
        assert abs(gn - gn_r) < 0.05 * gn_r
    live = runs[2][2]
    differ = float(((runs[2][1][live] - runs[None][1][live]).abs() > 0.5 * LR).float().mean())
    print(f"share of elements on which the chunked and the unchunked run took different signs in two steps: {differ:.4f}")


def test_train_step_with_the_built_lion_optimizer_zeroes_by_first_touch_and_leaves_operands_fresh():
    """The checks of test_train_step_with_the_built_sgd_optimizer_... for ``build_optimizer({'optimizer': 'lion'})``:
    ``train_step`` starts with the first-touch zero-fill (the whole gradient buffer NaN-poisoned before the step, lr = 0: every
    element must come out finite, the block weights by being overwritten, and with lr = 0 no master changes a bit -- the decay
    lr x wd is 0 and is skipped) and ends with the bf16 mirror and the blocks' W^T copies written by the update: the flags are
    set, the copies equal the masters' cast, and the next forward consumes them."""
    from oracle import clip_oracle as O
    from clip_event_amd.engine import train_step
    from clip_event_amd.optim import FusedLion, build_optimizer
    cfg = O.ClipConfig(*TILES_CFG)
    m, _ = _mk(cfg, 5)
    data = _batch(cfg, 4)
    crit = _crit()
    opt = build_optimizer(dict(LION_CFG, lr=0.0), m)
    assert type(opt) is FusedLion and opt.max_norm == 1.0
    train_step(m, crit, opt, *data)                 # builds the buffers
    calls = {"first_touch": 0, "full": 0}
    inner_ft, inner_zero = m.zero_grad_first_touch, m.zero_grad

    def counting_ft():
        calls["first_touch"] += 1
        return inner_ft()

    def counting_zero(*a, **k):
        calls["full"] += 1
        return inner_zero(*a, **k)

    m.zero_grad_first_touch, m.zero_grad = counting_ft, counting_zero
    m._flat_grad.fill_(float("nan"))
    before = m._flat.detach().clone()
    ld = train_step(m, crit, opt, *data)
    torch.cuda.synchronize()
    assert calls == {"first_touch": 1, "full": 0}, calls
    assert m._first_touch == set()
    assert bool(torch.isfinite(m._flat_grad).all()), "an element of the gradient buffer was neither zeroed nor overwritten"
    assert all(np.isfinite(float(v)) for v in ld.values()) and float(opt.grad_norm()) > 0
    live = _live(m)
    assert torch.equal(_bits(m._flat[live]), _bits(before[live]))            # lr = 0
    assert bool((opt.exp_avg[live] != 0).any())                              # the momentum did follow the gradient
    # a real step: the update leaves both operand copies behind
    opt.param_groups[0]["lr"] = LR
    assert m._adam_tiles_ok
    train_step(m, crit, opt, *data)
    torch.cuda.synchronize()
    assert m._mirror_fresh and m._wt_fresh
    assert not torch.equal(m._flat[live], before[live])
    assert torch.equal(_bits(m._flat16[live]), _bits(m._flat[live].to(torch.bfloat16)))
    name = "visual.transformer.resblocks.1.mlp.c_fc.weight"
    assert m._is_block_weight(name)
    w = dict(m.named_parameters())[name].detach()
    assert torch.equal(m._w16[name], w.to(torch.bfloat16)) and torch.equal(m._w16t[name], w.to(torch.bfloat16).t().contiguous())
    mirror, wt = m._flat16.clone(), m._w16t[name].clone()
    with torch.no_grad():
        m(data[0], data[1])                        # refresh_operands: nothing to cast, no block to transpose
    torch.cuda.synchronize()
    assert not m._mirror_fresh and not m._wt_fresh
    assert torch.equal(_bits(m._flat16), _bits(mirror)) and torch.equal(m._w16t[name], wt)


def test_locked_image_tower_with_no_decay_groups():
    """Partial fine-tuning: ``lock_image_tower()`` + ``no_decay_groups`` (matrices decay 2^-3, gains / biases / logit_scale none),
    two ``train_step``s.  The locked tower's masters, momentum (zero) and bf16 mirror keep their bits and its ``.grad`` stays
    None; the trainable part equals the stock loop over the trainable parameters with each one's own decay, clipped by the norm
    of the trainable gradients alone (StockLion.check)."""
    from oracle import clip_oracle as O
    from clip_event_amd.engine import train_step
    from clip_event_amd.optim import FusedLion, no_decay_groups
    cfg = O.ClipConfig(*TILES_CFG)
    m, sd = _mk(cfg, 13)
    data = _batch(cfg, 4)
    m.lock_image_tower()
    groups = no_decay_groups(m, WD)
    assert len(groups) == 2
    opt = FusedLion(m, lr=LR, betas=(B1, B2), weight_decay=WD, max_norm=1.0, groups=groups)
    assert [g["weight_decay"] for g in opt.param_groups] == [WD, 0.0] and not opt._plain()
    with torch.no_grad():
        m(data[0], data[1])                         # builds the buffers and casts the mirror
    torch.cuda.synchronize()
    trainable = {n for n, p in m.named_parameters() if p.requires_grad}
    locked = [n for n, p in m.named_parameters() if not p.requires_grad]
    assert locked and all(n.startswith("visual.") for n in locked) and trainable
    dead = torch.zeros(m._flat.numel(), dtype=torch.bool, device=DEV)
    for n in locked:
        dead[m._offsets[n]: m._offsets[n] + m._pmap[n].numel()] = True
    p_before, p16_before = m._flat.detach().clone(), m._flat16.detach().clone()
    decay = {n: (WD if n in groups[0]["params"] else 0.0) for n in trainable}
    assert any(v == 0.0 for v in decay.values()) and any(v == WD for v in decay.values())
    stock = StockLion({n: sd[n].to(DEV) for n in trainable}, LR, (B1, B2), decay, 1.0)
    for it in range(2):
        train_step(m, _crit(), opt, *data)
        torch.cuda.synchronize()
        norm = stock.step(_grads(m, trainable))
        assert norm > 1.0 and abs(float(opt.grad_norm()) - norm) <= 1e-4 * norm
    assert all(dict(m.named_parameters())[n].grad is None for n in locked)
    assert torch.equal(_bits(m._flat[dead]), _bits(p_before[dead]))
    assert torch.equal(_bits(m._flat16[dead]), _bits(p16_before[dead]))
    assert not bool(opt.exp_avg[dead].any()) and bool(opt.exp_avg[~dead].any())
    stock.check("locked image tower + no_decay_groups", {n: p.detach() for n, p in m.named_parameters() if n in trainable})
    assert set(opt.state_dict()["state"]) == set(range(len(trainable)))


def test_ema_and_averaged_with_fused_lion():
    """``enable_ema(0.5)`` then three ``train_step``s: the average equals e_k = e_{k-1} + r (p_k - e_{k-1}) over the masters
    recorded after every step, in fp64 from e_0 = p_0, within 3 x the op-level bound of tests/test_ema_ops.py (the rule of
    test_the_average_is_the_recurrence_over_the_masters); inside ``averaged()`` the model holds the average and the optimiser the
    training weights; on exit masters, average and mirror have their bits back."""
    from oracle import clip_oracle as O
    from clip_event_amd.engine import train_step
    from clip_event_amd.optim import build_optimizer, ema_rate
    cfg = O.ClipConfig(*TILES_CFG)
    m, _ = _mk(cfg, 19)
    data = _batch(cfg, 4)
    opt = build_optimizer(LION_CFG, m)
    opt.enable_ema(0.5)
    assert torch.equal(_bits(opt.ema), _bits(m._flat)) and opt.ema_updates == 0
    e = m._flat.detach().double().clone()
    bound = torch.zeros_like(e)
    r = float(np.float32(ema_rate(0.5, False, 0)))
    for k in range(3):
        train_step(m, _crit(), opt, *data)
        torch.cuda.synchronize()
        p = m._flat.detach()
        ref = ema_ref(e, p, r)
        bound = torch.maximum(bound, _ema_bound(ref, e, p, r))
        e = ref
    err = (opt.ema.double() - e).abs()
    worst = float((err / (3 * bound).clamp_min(1e-300)).max())
    print(f"[lion ema recurrence] worst |err| / (3 x bound) {worst:.3f}")
    assert opt.ema_updates == 3 and bool((err <= 3 * bound).all()), worst
    p0, e0, p16_0 = m._flat.detach().clone(), opt.ema.detach().clone(), m._flat16.detach().clone()
    assert not torch.equal(p0, e0)
    with opt.averaged() as inside:
        assert inside is m
        assert torch.equal(_bits(m._flat), _bits(e0)) and torch.equal(_bits(opt.ema), _bits(p0))
        live = _live(m)
        assert torch.equal(_bits(m._flat16[live]), _bits(e0[live].to(torch.bfloat16)))
        with pytest.raises(RuntimeError, match="averaged"):
            opt.step()
    torch.cuda.synchronize()
    assert torch.equal(_bits(m._flat), _bits(p0)) and torch.equal(_bits(opt.ema), _bits(e0)) and torch.equal(_bits(m._flat16), _bits(p16_0))


def test_checkpoint_round_trip_with_fused_lion(tmp_path):
    """``checkpoint.save_model_on_master`` + ``load_checkpoint`` after two steps: the file's 'optimizer' entry has one ``exp_avg``
    per parameter and the group keys lr / betas / weight_decay; the resumed model and momentum equal the saved ones bit for bit,
    and a third step from the same gradient buffer (of norm 0.5: the clip coefficient is exactly 1 whatever order the norm's
    float atomics arrived in) is bit-equal to the uninterrupted one in masters, momentum and mirror."""
    from oracle import clip_oracle as O
    from clip_event_amd import checkpoint
    from clip_event_amd.engine import train_step
    from clip_event_amd.optim import FusedLion, build_optimizer
    cfg = O.ClipConfig(*TILES_CFG)
    m, _ = _mk(cfg, 9)
    data = _batch(cfg, 4)
    opt = build_optimizer(LION_CFG, m)
    for _ in range(2):
        train_step(m, _crit(), opt, *data)
    torch.cuda.synchronize()
    path = checkpoint.save_model_on_master(m, str(tmp_path), "clipevent", 2, 0.0, opt)
    assert path is not None
    m2, opt_state, epoch, _ = checkpoint.load_checkpoint(path, device=DEV)
    assert epoch == 2 and set(opt_state["state"][0]) == {"exp_avg"}
    assert {k for k in opt_state["param_groups"][0] if k != "params"} == {"lr", "betas", "weight_decay"}
    opt2 = build_optimizer(dict(LION_CFG, lr=0.5, betas=(0.5, 0.5), weight_decay=0.0), m2)
    assert type(opt2) is FusedLion
    opt2.load_state_dict(opt_state)
    live = _live(m)
    assert torch.equal(_bits(m2._flat[live]), _bits(m._flat[live])) and torch.equal(_bits(opt2.exp_avg[live]), _bits(opt.exp_avg[live]))
    assert {k: v for k, v in opt2.param_groups[0].items() if k != "params"} == {k: v for k, v in opt.param_groups[0].items() if k != "params"}
    for oo in (opt, opt2):
        oo.zero_grad()
    g = torch.randn(m._flat_grad.numel(), generator=torch.Generator().manual_seed(4))
    g = (g * (0.5 / float(g.double().norm()))).to(DEV)
    before = m._flat.detach().clone()
    for mm, oo in ((m, opt), (m2, opt2)):
        mm._flat_grad.copy_(g)
        oo.step()
    torch.cuda.synchronize()
    assert not torch.equal(m._flat[live], before[live])
    assert torch.equal(_bits(m2._flat[live]), _bits(m._flat[live])) and torch.equal(_bits(opt2.exp_avg[live]), _bits(opt.exp_avg[live]))
    assert torch.equal(_bits(m2._flat16[live]), _bits(m._flat16[live]))


@pytest.mark.timeout(900)
@pytest.mark.parametrize("case", ["allreduce", "sharded"])
def test_two_rank_fused_lion_step(case):
    """Two ranks on one GPU over gloo (tests/lion_ddp_child.py): two ``train_step``s with FusedLion through the real GradSync --
    gradient all-reduce + replicated update, and CE_SHARDED_ADAM=1 (update of the own shards, all-gather of the masters,
    ``consolidate`` of the one momentum) -- against the stock loop and the single-process steps on the concatenated batch; on the
    sharded path groups, frozen parameters and EMA raise NotImplementedError."""
    rcs, outs = run_ranks("lion_ddp_child.py", case, extra_env={"CE_SHARDED_ADAM": "1" if case == "sharded" else "0"})
    print(outs[0][-3000:])
    assert rcs == [0, 0], "\n".join(o[-3000:] for o in outs)
    assert f"[{case}] OK" in outs[0]
