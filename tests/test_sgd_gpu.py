"""GPU: ``optim.FusedSGD`` (clip + SGD with momentum on the HIP path) as a torch optimiser, against the reference's stock loop
(engine.py:87-90 with torch.optim.SGD), through ``engine.train_step`` / ``build_optimizer``, through a checkpoint, and on two
ranks (tests/sgd_ddp_child.py)."""
import numpy as np
import pytest
import torch

from tests.test_ddp_gpu import run_ranks
from tests.test_sgd_ops import _sgd_bounds, sgd_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _mk(cfg, seed):
    from oracle import clip_oracle as O
    from clip_event_amd.model import build_model
    sd = O.init_params(cfg, seed)
    m = build_model({k: v.clone() for k, v in sd.items()}).to(DEV)
    return m, sd


def _cos(a, b):
    a, b = a.double().flatten().cpu(), b.double().flatten().cpu()
    return float(a @ b / (a.norm() * b.norm() + 1e-30))


def _rel(a, b):
    a, b = a.double().flatten().cpu(), b.double().flatten().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _batch(cfg, B, K=1):
    from oracle import clip_oracle as O
    from clip_event_amd import synthetic as S
    img = S.synthetic_images(B, cfg.image_resolution, seed=1).to(DEV)
    txt = S.synthetic_tokens(B * K, cfg.context_length, cfg.vocab_size, seed=2, min_len=2).to(DEV)
    yi, yt, ip = (t.to(DEV) for t in O.build_labels(B, 1, K - 1, True))
    return img, txt, yi, yt, ip


def _live(m):
    """Mask of the flat buffer's elements that belong to a parameter (the rest is layout padding)."""
    live = torch.zeros(m._flat.numel(), dtype=torch.bool, device=DEV)
    for n, p in m._pmap.items():
        live[m._offsets[n]: m._offsets[n] + p.numel()] = True
    return live


def test_fused_sgd_is_a_torch_optimizer():
    """FusedSGD under the reference's driver pattern (engine.py:87-97: zero_grad, backward, step, scheduler.step): the
    warm-up cosine scheduler drives it; after three steps its state_dict loads into torch.optim.SGD over detached twins of the
    parameters, both take one more step from the same gradients, and every parameter element agrees within TWICE the
    op-level bound of tests/test_sgd_ops.py (one bound per side: each is an fp32 evaluation of the same fp64 update; the CPU
    check there shows torch uses half of its own).  Back again: torch's state loads into a fresh FusedSGD with every
    momentum_buffer equal bit for bit.  An empty state (before the first step) loads as "first step"; a state in which only
    some parameters carry a buffer is refused."""
    from oracle import clip_oracle as O
    from clip_event_amd.losses import CriterionContrastive
    from clip_event_amd.optim import FusedSGD, WarmupCosineLR
    cfg = O.ClipConfig(64, 64, 2, 128, 32, 20, 512, 128, 2, 2)
    m, sd = _mk(cfg, 21)
    img, txt, yi, yt, ip = _batch(cfg, 4)
    crit = CriterionContrastive("ce")
    mu, wd = 0.9, 0.01
    opt = FusedSGD(m, lr=1e-2, momentum=mu, weight_decay=wd, max_norm=None)
    assert isinstance(opt, torch.optim.Optimizer)
    empty = opt.state_dict()
    assert empty["state"] == {} and opt.state_buffers()[0].numel() == m._flat.numel()
    sch = WarmupCosineLR(opt, max_iters=10, warmup_epochs=3)
    lrs = []

    def backward():
        ld = crit(*m(img, txt), yi, yt, index_pos=ip)
        opt.zero_grad()
        sum(ld.values()).backward()

    for _ in range(3):
        backward()
        lrs.append(opt.param_groups[0]["lr"])
        opt.step()
        sch.step()
    np.testing.assert_allclose(lrs, [O.lr_warmup_cosine(1e-2, i, 10, warmup_epochs=3) for i in range(3)], rtol=1e-12)
    state = opt.state_dict()
    params = list(m.parameters())
    assert set(state) == {"state", "param_groups"} and len(state["state"]) == len(params)
    assert all(set(st) == {"momentum_buffer"} and st["momentum_buffer"].shape == p.shape for st, p in zip(state["state"].values(), params))
    # the same state in torch's own SGD, over detached copies of the parameters, fed the same gradients
    backward()
    torch.cuda.synchronize()
    before = [p.detach().clone() for p in params]
    grads = [p.grad.detach().clone() for p in params]
    twins = [torch.nn.Parameter(p.clone()) for p in before]
    for t, g in zip(twins, grads):
        t.grad = g.clone()
    bufs = [state["state"][i]["momentum_buffer"].clone() for i in range(len(params))]      # (torch adopts the loaded tensors and updates them in place)
    ref = torch.optim.SGD(twins, lr=123.0, momentum=0.0)
    ref.load_state_dict(state)                      # carries the scheduler-set lr, the momentum and the weight decay
    lr = ref.param_groups[0]["lr"]
    assert lr == opt.param_groups[0]["lr"] == sch.get_last_lr()[0] and ref.param_groups[0]["momentum"] == mu
    ref.step()
    opt.step()
    torch.cuda.synchronize()
    worst = 0.0
    for i, (p, t) in enumerate(zip(params, twins)):
        r64 = sgd_ref(before[i].cpu(), grads[i].cpu(), bufs[i].cpu(), None, wd, mu, 0.0, False, False, lr=lr)
        bound = 2 * _sgd_bounds(r64, lr=lr)[0]
        err = (p.detach().cpu().double() - t.detach().cpu().double()).abs()
        worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
        assert bool((err <= bound).all()), (i, worst)
        for side in (p, t):                          # and each side within its own bound of the fp64 update
            assert bool(((side.detach().cpu().double() - r64[0]).abs() <= bound / 2).all()), i
    print(f"FusedSGD vs torch.optim.SGD after state hand-over: worst |difference| / (2 x op-level bound) {worst:.3f}")
    # and back: torch's state into a fresh FusedSGD
    m2, _ = _mk(cfg, 21)
    opt2 = FusedSGD(m2, lr=5e-4, momentum=0.5, max_norm=None)
    opt2.load_state_dict(ref.state_dict())
    assert opt2.param_groups[0]["lr"] == lr and opt2.momentum == mu and opt2.weight_decay == wd and opt2._has_buf
    s2 = opt2.state_dict()
    for i, st in ref.state_dict()["state"].items():
        assert torch.equal(s2["state"][i]["momentum_buffer"].cpu(), st["momentum_buffer"].cpu()), i
    # a partial state is refused
    partial = ref.state_dict()
    del partial["state"][0]
    with pytest.raises(ValueError, match="momentum_buffer"):
        opt2.load_state_dict(partial)
    # the empty state loads as "first step": the next step COPIES the gradient into the buffer whatever the dampening is
    opt2.load_state_dict(empty)
    assert not opt2._has_buf and opt2.state_dict()["state"] == {}
    opt2.param_groups[0].update(dampening=0.5, weight_decay=0.0, lr=0.0)
    opt2.zero_grad()
    m2._flat_grad.copy_(torch.randn(m2._flat_grad.numel(), generator=torch.Generator().manual_seed(3)).to(DEV))
    g2 = m2._flat_grad.clone()
    opt2.step()
    torch.cuda.synchronize()
    live = _live(m2)
    assert opt2._has_buf and torch.equal(opt2.buf[live], g2[live])


def test_stock_torch_sgd_loop_matches_fused():
    """engine.py:87-90 verbatim -- ``optimizer.zero_grad(); losses.backward(); clip_grad_norm_(model.parameters(), 1);
    optimizer.step()`` with ``torch.optim.SGD(momentum 0.9, weight_decay 0.01)`` -- on the drop-in model against FusedSGD on its
    twin, three steps.  The runs' gradients differ in the last bits (float-atomic order), so the yardstick is measured in the
    test: a SECOND stock model from the same seed.  The relative L2 of the accumulated update, fused against stock, must stay
    within 4 x the stock-against-stock spread + 1e-4, for the whole update and per parameter (4: three steps of order noise;
    1e-4: the fp32 rounding of a master of size ~0.02 against an update of ~1e-5 per element).  The clip must have been active
    (gradient norm > 1 before the clip), otherwise the test says nothing about it."""
    from oracle import clip_oracle as O
    from clip_event_amd.losses import CriterionContrastive
    from clip_event_amd.optim import FusedSGD
    cfg = O.ClipConfig(64, 64, 2, 128, 32, 20, 512, 128, 2, 2)
    img, txt, yi, yt, ip = _batch(cfg, 6)
    crit = CriterionContrastive("ce")
    lr, mu, wd = 1e-2, 0.9, 0.01
    ma, sd = _mk(cfg, 17)
    ma2, _ = _mk(cfg, 17)
    mb, _ = _mk(cfg, 17)
    stock = torch.optim.SGD(ma.parameters(), lr=lr, momentum=mu, weight_decay=wd)
    stock2 = torch.optim.SGD(ma2.parameters(), lr=lr, momentum=mu, weight_decay=wd)
    fused = FusedSGD(mb, lr=lr, momentum=mu, weight_decay=wd, max_norm=1.0)
    for it in range(3):
        norms = []
        for model, o in ((ma, stock), (ma2, stock2)):
            la = crit(*model(img, txt), yi, yt, index_pos=ip)
            o.zero_grad()                                     # set_to_none=True: the lazy zero-fill path
            sum(la.values()).backward()
            norms.append(float(torch.nn.utils.clip_grad_norm_(model.parameters(), 1)))
            o.step()
        lb = crit(*mb(img, txt), yi, yt, index_pos=ip)
        fused.zero_grad()
        sum(lb.values()).backward()
        fused.step()
        torch.cuda.synchronize()
        norms.append(float(fused.grad_norm()))
        print(f"step {it}: gradient norm before the clip: stock {norms[0]:.4f}, stock' {norms[1]:.4f}, fused {norms[2]:.4f}")
        assert min(norms) > 1.0, norms

    def delta(model):
        return {n: (p.detach() - sd[n].to(DEV)).flatten() for n, p in model.named_parameters()}

    da, da2, db = delta(ma), delta(ma2), delta(mb)
    whole = lambda d: torch.cat(list(d.values()))
    fused_rel, spread = _rel(whole(db), whole(da)), _rel(whole(da2), whole(da))
    print(f"accumulated update after 3 steps, rel-L2: fused vs stock {fused_rel:.3e}, stock vs stock {spread:.3e}, "
          f"bound {4 * spread + 1e-4:.3e}")
    worst = (0.0, None, 0.0, 0.0)
    bad = []
    for n in da:
        if float(da[n].norm()) == 0.0:
            if float(db[n].norm()) != 0.0:
                bad.append((n, "stock did not move this parameter"))
            continue
        f, s = _rel(db[n], da[n]), _rel(da2[n], da[n])
        if f / (4 * s + 1e-4) > worst[0]:
            worst = (f / (4 * s + 1e-4), n, f, s)
        if f > 4 * s + 1e-4:
            bad.append((n, f, s))
    print(f"worst parameter: {worst[1]}: fused vs stock {worst[2]:.3e}, stock vs stock {worst[3]:.3e} ({worst[0]:.3f} of its bound)")
    assert fused_rel <= 4 * spread + 1e-4
    assert not bad, bad


TILES_CFG = (64, 64, 3, 192, 32, 20, 512, 128, 2, 3)        # (block weights tile: model._adam_tiles_ok)
SGD_CFG = {"optimizer": "sgd", "lr": 1e-2, "momentum": 0.9, "weight_decay": 0.01}


def test_train_step_with_the_built_sgd_optimizer_zeroes_by_first_touch_and_leaves_operands_fresh():
    """``build_optimizer({'optimizer': 'sgd'})`` returns a FusedSGD; ``train_step`` starts with the first-touch zero-fill (the
    whole gradient buffer NaN-poisoned before the step, lr = 0: every element must come out finite, the block weights by
    being overwritten) and ends with the bf16 mirror and the blocks' W^T copies written by the update: the flags are set, the
    copies equal the masters' cast, and the next forward consumes them."""
    from oracle import clip_oracle as O
    from clip_event_amd.engine import train_step
    from clip_event_amd.losses import CriterionContrastive
    from clip_event_amd.optim import FusedSGD, build_optimizer
    cfg = O.ClipConfig(*TILES_CFG)
    m, _ = _mk(cfg, 5)
    data = _batch(cfg, 4)
    crit = CriterionContrastive("ce")
    opt = build_optimizer(dict(SGD_CFG, lr=0.0), m)
    assert type(opt) is FusedSGD and opt.max_norm == 1.0 and opt.momentum == 0.9
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
    assert torch.equal(m._flat[live], before[live])            # lr = 0
    # a real step: the update leaves both operand copies behind
    opt.param_groups[0]["lr"] = 1e-2
    assert m._adam_tiles_ok
    train_step(m, crit, opt, *data)
    torch.cuda.synchronize()
    assert m._mirror_fresh and m._wt_fresh
    assert not torch.equal(m._flat[live], before[live])
    assert torch.equal(m._flat16[live].view(torch.int16), m._flat[live].to(torch.bfloat16).view(torch.int16))
    name = "visual.transformer.resblocks.1.mlp.c_fc.weight"
    assert m._is_block_weight(name)
    w = dict(m.named_parameters())[name].detach()
    assert torch.equal(m._w16[name], w.to(torch.bfloat16)) and torch.equal(m._w16t[name], w.to(torch.bfloat16).t().contiguous())
    mirror, wt = m._flat16.clone(), m._w16t[name].clone()
    with torch.no_grad():
        m(data[0], data[1])                        # refresh_operands: nothing to cast, no block to transpose
    torch.cuda.synchronize()
    assert not m._mirror_fresh and not m._wt_fresh
    assert torch.equal(m._flat16.view(torch.int16), mirror.view(torch.int16)) and torch.equal(m._w16t[name], wt)


def test_chunked_train_step_with_fused_sgd_against_the_unchunked_step():
    """``micro_batch=2`` at B = 4, two steps of the built SGD optimiser, against the unchunked step of the same build at the
    bounds test_chunked_train_step_fused_adam_against_golden puts on its step: losses within 3e-2, gradient norm within 5 %,
    worst per-parameter cosine of the accumulated update > 0.98."""
    from oracle import clip_oracle as O
    from clip_event_amd.engine import train_step
    from clip_event_amd.losses import CriterionContrastive
    from clip_event_amd.optim import build_optimizer
    from tests.util import golden_json
    cfg = O.ClipConfig(**golden_json()["tiny"]["cfg"])
    data = _batch(cfg, 4)
    crit = CriterionContrastive("ce")
    runs = {}
    for mb in (None, 2):
        m, sd = _mk(cfg, 11)
        opt = build_optimizer(SGD_CFG, m)
        log = []
        for _ in range(2):
            ld = train_step(m, crit, opt, *data, micro_batch=mb)
            torch.cuda.synchronize()
            log.append((float(ld["loss_i"]), float(ld["loss_t"]), float(opt.grad_norm())))
        runs[mb] = (log, {n: p.detach() - sd[n].to(DEV) for n, p in m.named_parameters()})
    for (li, lt, gn), (li_r, lt_r, gn_r) in zip(runs[2][0], runs[None][0]):
        print(f"chunked loss_i {li:.5f} loss_t {lt:.5f} grad_norm {gn:.4f}; unchunked {li_r:.5f} {lt_r:.5f} {gn_r:.4f}")
        assert abs(li - li_r) < 3e-2 and abs(lt - lt_r) < 3e-2
        assert abs(gn - gn_r) < 0.05 * gn_r
    worst = 1.0
    for n, d_ref in runs[None][1].items():
        if float(d_ref.norm()) > 0:
            worst = min(worst, _cos(runs[2][1][n], d_ref))
    print("worst parameter-delta cosine after 2 chunked SGD steps against the unchunked steps:", worst)
    assert worst > 0.98


def test_checkpoint_round_trip_with_fused_sgd(tmp_path):
    """``checkpoint.save_model_on_master`` + ``load_checkpoint`` with an SGD optimiser: the file's 'optimizer' entry is
    torch.optim.SGD's format (it loads into the stock optimiser), the resumed model and momentum buffer equal the saved ones bit
    for bit, and the same gradient buffer then gives the identical next step; a ``train_step`` from both agrees in the loss."""
    from oracle import clip_oracle as O
    from clip_event_amd import checkpoint
    from clip_event_amd.engine import train_step
    from clip_event_amd.losses import CriterionContrastive
    from clip_event_amd.optim import FusedSGD, build_optimizer
    cfg = O.ClipConfig(*TILES_CFG)
    m, _ = _mk(cfg, 9)
    data = _batch(cfg, 4)
    crit = CriterionContrastive("ce")
    opt = build_optimizer(SGD_CFG, m)
    for _ in range(2):
        train_step(m, crit, opt, *data)
    torch.cuda.synchronize()
    path = checkpoint.save_model_on_master(m, str(tmp_path), "clipevent", 2, 0.0, opt)
    assert path is not None
    m2, opt_state, epoch, _ = checkpoint.load_checkpoint(path, device=DEV)
    assert epoch == 2 and set(opt_state["state"][0]) == {"momentum_buffer"}
    stock = torch.optim.SGD([torch.nn.Parameter(p.detach().clone()) for p in m2.parameters()], lr=1.0)
    stock.load_state_dict(opt_state)                           # torch's own format
    assert stock.param_groups[0]["momentum"] == 0.9 and stock.param_groups[0]["lr"] == 1e-2
    opt2 = build_optimizer(dict(SGD_CFG, lr=0.5, momentum=0.1), m2)
    assert type(opt2) is FusedSGD
    opt2.load_state_dict(opt_state)
    live = _live(m)
    assert torch.equal(m2._flat[live], m._flat[live]) and torch.equal(opt2.buf[live], opt.buf[live])
    assert {k: v for k, v in opt2.param_groups[0].items() if k != "params"} == {k: v for k, v in opt.param_groups[0].items() if k != "params"}
    # the identical next step from the same gradients (of norm 0.5: the clip coefficient is exactly 1 whatever order the norm's
    # float atomics arrived in, as in tests/test_model_gpu.py::test_fused_adam_in_tiles_equals_the_flat_kernel)
    for mm, oo in ((m, opt), (m2, opt2)):
        oo.zero_grad()
    g = torch.randn(m._flat_grad.numel(), generator=torch.Generator().manual_seed(4))
    g = (g * (0.5 / float(g.double().norm()))).to(DEV)
    for mm, oo in ((m, opt), (m2, opt2)):
        mm._flat_grad.copy_(g)
        oo.step()
    torch.cuda.synchronize()
    assert torch.equal(m2._flat[live], m._flat[live]) and torch.equal(opt2.buf[live], opt.buf[live])
    assert torch.equal(m2._flat16[live].view(torch.int16), m._flat16[live].view(torch.int16))
    la = train_step(m, crit, opt, *data)
    lb = train_step(m2, crit, opt2, *data)
    la, lb = float(sum(v.detach() for v in la.values())), float(sum(v.detach() for v in lb.values()))
    print(f"resumed run continues: loss {la:.6f} vs {lb:.6f}")
    assert abs(la - lb) < 1e-3 * max(1.0, abs(la))


@pytest.mark.timeout(900)
@pytest.mark.parametrize("case", ["allreduce", "sharded"])
def test_two_rank_fused_sgd_step_equals_concatenated_batch(case):
    """Two ranks on one GPU over gloo (tests/sgd_ddp_child.py): two ``train_step``s with FusedSGD through the real GradSync --
    gradient all-reduce + replicated update, and CE_SHARDED_ADAM=1 (reduce-scatter, update of the own shards, all-gather of the
    masters, ``consolidate`` of the one momentum buffer) -- against the single-process steps on the concatenated batch."""
    rcs, outs = run_ranks("sgd_ddp_child.py", case, extra_env={"CE_SHARDED_ADAM": "1" if case == "sharded" else "0"})
    print(outs[0][-3000:])
    assert rcs == [0, 0], "\n".join(o[-3000:] for o in outs)
    assert f"[{case}] OK" in outs[0]
