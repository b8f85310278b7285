"""GPU: partial fine-tuning through the model -- frozen parameters, a locked tower, a backward that stops at the lowest trainable
block, the micro-batched step with a locked tower, parameter groups against ``torch.optim.AdamW``, a plan that changes between
steps, and two ranks (tests/partial_ddp_child.py).  Tiny oracle geometry: 2 image blocks, 3 text blocks, width 128."""
import numpy as np
import pytest
import torch

from tests.test_ddp_gpu import run_ranks
from tests.test_embed_optim_ops import B1, B2, EPS, LR, U, _adam_bounds, adam_ref
from tests.test_sgd_ops import _sgd_bounds, sgd_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CFG_ARGS = (64, 64, 2, 128, 32, 20, 512, 128, 2, 3)


@pytest.fixture(params=[False, True], ids=["stream32", "stream16"])
def stream16(request, monkeypatch):
    """Both residual-stream formats (fixture of tests/test_model_gpu.py)."""
    monkeypatch.setenv("CE_STREAM16", "1" if request.param else "0")
    return request.param


def _cfg():
    from oracle import clip_oracle as O
    return O.ClipConfig(*CFG_ARGS)


def _mk(seed=31):
    from oracle import clip_oracle as O
    from clip_event_amd.model import build_model
    sd = O.init_params(_cfg(), seed)
    return build_model({k: v.clone() for k, v in sd.items()}).to(DEV), sd


def _batch(B, K=1):
    from oracle import clip_oracle as O
    from clip_event_amd import synthetic as S
    cfg = _cfg()
    img = S.synthetic_images(B, cfg.image_resolution, seed=1).to(DEV)
    txt = S.synthetic_tokens(B * K, cfg.context_length, cfg.vocab_size, seed=2, min_len=2).to(DEV)
    yi, yt, ip = (t.to(DEV) for t in O.build_labels(B, 1, K - 1, True))
    return img, txt, yi, yt, ip


def _rel(a, b):
    a, b = a.double().flatten().cpu(), b.double().flatten().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _bits_equal(a, b):
    return torch.equal(a.detach().cpu().contiguous().view(torch.int32), b.detach().cpu().contiguous().view(torch.int32))


def _crit():
    from clip_event_amd.losses import CriterionContrastive
    return CriterionContrastive("ce")


def _gradients(m, batch):
    """The gradients one ``train_step`` leaves in the flat buffer (FusedAdam with lr 0: nothing moves), by name, trainable only."""
    from clip_event_amd.engine import train_step
    from clip_event_amd.optim import FusedAdam
    train_step(m, _crit(), FusedAdam(m, lr=0.0, max_norm=1.0), *batch)
    torch.cuda.synchronize()
    return {n: m._gview(n).detach().clone() for n, p in m.named_parameters() if p.requires_grad}


def _spread_rule(tag, got, twin_a, twin_b, names):
    """The suite's rule for gradients whose LayerNorm / bias sums are float atomics (not order-stable): against an all-trainable
    twin rel-L2 <= 4 x spread + 1e-6, per parameter and over all of them together, where the spread is the rel-L2 between two
    all-trainable runs from the same seed."""
    worst = 0.0
    for n in names:
        spread, r = _rel(twin_b[n], twin_a[n]), _rel(got[n], twin_a[n])
        worst = max(worst, r / (4 * spread + 1e-6))
        assert r <= 4 * spread + 1e-6, (tag, n, r, spread)

    def cat(d):
        return torch.cat([d[n].flatten() for n in names])
    spread, r = _rel(cat(twin_b), cat(twin_a)), _rel(cat(got), cat(twin_a))
    print(f"[{tag}] {len(names)} parameters: whole rel-L2 {r:.3e} (spread {spread:.3e}); worst per-parameter rel / bound {worst:.3f}")
    assert r <= 4 * spread + 1e-6, (tag, r, spread)


# ---- frozen subset ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which,tiles", [("adam", "1"), ("adam", "0"), ("sgd", "1")])
def test_frozen_subset_is_untouched_and_the_rest_follows_the_update_rule(which, tiles, monkeypatch):
    """conv1, one gain, the token embedding and the whole of text block 0 frozen; three ``train_step``s with the clip active.
    Frozen parameters keep their bits and ``.grad`` None; after step 1 every trainable parameter is within the op-level bound of the
    fp64 restatement fed that step's own gradients and the sum of squares of the TRAINABLE gradients only; ``grad_norm()`` is their
    fp64 norm to 1e-5.  With CE_ADAM_TILES=0 the block weights go through the segment table."""
    from clip_event_amd.engine import train_step
    from clip_event_amd.optim import FusedAdam, FusedSGD
    monkeypatch.setenv("CE_ADAM_TILES", tiles)
    m, sd = _mk()
    frozen = ["visual.conv1.weight", "visual.transformer.resblocks.1.ln_1.weight", "token_embedding.weight"] + \
        [n for n, _ in m.named_parameters() if n.startswith("transformer.resblocks.0.")]
    for n, p in m.named_parameters():
        p.requires_grad_(n not in frozen)
    wd, mu = 0.01, 0.9
    if which == "adam":
        opt = FusedAdam(m, lr=LR, betas=(B1, B2), eps=EPS, weight_decay=wd, max_norm=1.0)
    else:
        opt = FusedSGD(m, lr=LR, momentum=mu, max_norm=1.0)
    batch = _batch(4)
    for step in (1, 2, 3):
        train_step(m, _crit(), opt, *batch)
        torch.cuda.synchronize()
        for n, p in m.named_parameters():
            if n in frozen:
                assert p.grad is None and _bits_equal(p, sd[n]), (step, n)
        if step > 1:
            continue
        grads = {n: p.grad.detach().cpu() for n, p in m.named_parameters() if n not in frozen}
        sumsq = sum(float((g.double() ** 2).sum()) for g in grads.values())
        assert sumsq > 1.0                                                            # the clip is active
        gn = float(opt.grad_norm())
        print(f"[frozen subset {which} tiles={tiles}] grad_norm {gn:.7f}, fp64 over the trainable gradients {sumsq ** 0.5:.7f}")
        assert abs(gn - sumsq ** 0.5) <= 1e-5 * sumsq ** 0.5
        worst = 0.0
        for n, p in m.named_parameters():
            if n in frozen:
                continue
            zero = torch.zeros_like(sd[n])
            if which == "adam":
                ref = adam_ref(sd[n], grads[n], zero, zero, float(np.float32(sumsq)), wd, 1)
                bound = _adam_bounds(ref)[0]
            else:
                ref = sgd_ref(sd[n], grads[n], zero, float(np.float32(sumsq)), 0.0, mu, 0.0, False, True, lr=LR)
                bound = _sgd_bounds(ref, lr=LR)[0]
            err = (p.detach().cpu().double() - ref[0]).abs()
            worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
            assert bool((err <= bound).all()), (n, worst)
        print(f"[frozen subset {which} tiles={tiles}] step 1 masters: worst |err| / bound {worst:.3f}")
    moved = [n for n, p in m.named_parameters() if n not in frozen and not _bits_equal(p, sd[n])]
    assert len(moved) >= len(sd) - len(frozen) - 2 and bool(torch.isfinite(m._flat).all())


# ---- locked image tower ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("head", ["small", "fused", "general"])
def test_locked_image_tower_runs_forward_only(head, monkeypatch):
    """``lock_image_tower()``: ``encode_both`` with grad mode on returns image features equal, bit for bit, to ``encode_image``
    under ``no_grad`` and without a graph; the text tower's gradients follow an all-trainable twin's (spread rule); a
    ``train_step`` completes and leaves every image parameter's bits.  Through the three-launch head, the fused head
    (CE_FUSED_HEAD=1) and logits + criterion (CE_FUSED_HEAD=0)."""
    from clip_event_amd import functional as F
    from clip_event_amd.engine import train_step
    from clip_event_amd.optim import FusedAdam
    if head != "small":
        monkeypatch.setenv("CE_FUSED_HEAD", "1" if head == "fused" else "0")
    batch = _batch(5)
    m, sd = _mk()
    m.lock_image_tower()
    fi, ft = m.encode_both(batch[0], batch[1])
    assert not fi.requires_grad and fi.grad_fn is None and ft.requires_grad
    with torch.no_grad():
        fi0 = m.encode_image(batch[0])
    assert _bits_equal(fi, fi0)
    del fi, ft
    calls = []
    inner = F._tower_forward_infer
    F._tower_forward_infer = lambda model, desc, tag, *a: (calls.append(tag), inner(model, desc, tag, *a))[1]
    try:
        got = _gradients(m, batch)
    finally:
        F._tower_forward_infer = inner
    assert calls == ["vision"]                                   # stash-free, and the text tower kept its stash
    assert all(p.grad is None for n, p in m.named_parameters() if n.startswith("visual."))
    twins = []
    for _ in range(2):
        t, _sd = _mk()
        twins.append(_gradients(t, batch))
    names = [n for n in got if n != "logit_scale"]
    assert names and not any(n.startswith("visual.") for n in names)
    _spread_rule(f"locked image tower, {head} head", got, twins[0], twins[1], names)
    ld = train_step(m, _crit(), FusedAdam(m, lr=1e-3, max_norm=1.0), *batch)
    torch.cuda.synchronize()
    assert all(np.isfinite(float(v)) for v in ld.values())
    for n, p in m.named_parameters():
        assert _bits_equal(p, sd[n]) == n.startswith("visual."), n


# ---- truncated backward ----------------------------------------------------------------------------------------------------------

def test_backward_stops_at_the_lowest_trainable_block(stream16):
    """``lock_text_tower(unlocked_layers=1)`` on three text blocks: a sentinel written into the gradient slices of blocks 0-1 and of
    the text embeddings after ``zero_grad()`` survives the backward bit for bit -- no kernel ran below the cut -- and the
    gradients of block 2, ``ln_final`` and ``text_projection`` follow an all-trainable twin's (spread rule)."""
    batch = _batch(4)
    img, txt, yi, yt, ip = batch

    def backward(m):
        m.zero_grad()
        ld = _crit()(*m(img, txt), yi, yt, index_pos=ip)
        return ld

    m, _ = _mk()
    m(img, txt)                                                    # builds the flat buffers
    m.lock_text_tower(unlocked_layers=1)
    assert m.trainable_plan().stop_layer == {"visual": 0, "text": 2}
    below = [n for n, _ in m.named_parameters() if n.startswith(("transformer.resblocks.0.", "transformer.resblocks.1.",
                                                                 "token_embedding.")) or n == "positional_embedding"]
    assert len(below) == 2 * 12 + 2
    ld = backward(m)
    for n in below:
        m._gview(n).fill_(-77.25)
    sum(ld.values()).backward()
    torch.cuda.synchronize()
    for n in below:
        assert bool((m._gview(n) == -77.25).all()), n
    got = {n: m._gview(n).detach().clone() for n, p in m.named_parameters() if p.requires_grad}
    twins = []
    for _ in range(2):
        t, _sd = _mk()
        sum(backward(t).values()).backward()
        torch.cuda.synchronize()
        twins.append({n: t._gview(n).detach().clone() for n, _ in t.named_parameters()})
    names = [n for n in got if n.startswith(("transformer.resblocks.2.", "ln_final.")) or n == "text_projection"]
    assert len(names) == 12 + 3
    _spread_rule(f"truncated text backward, stream16={stream16}", got, twins[0], twins[1], names)
    assert all(torch.isfinite(got[n]).all() for n in got)


# ---- micro-batch + lock ----------------------------------------------------------------------------------------------------------

def test_micro_batched_step_encodes_a_locked_tower_once():
    """``train_step(micro_batch=2)`` at B = 6 with the image tower locked against the unchunked locked step, under
    tests/test_micro_batch_gpu.py's rule for chunked against unchunked (losses within 3e-3 max(1, |loss|), per trainable parameter
    gradient rel-L2 <= 2e-3, exactly zero where the unchunked gradient is), and the update one clip + SGD step makes of those
    gradients -- linear in them -- within the same 2e-3 over all trainable parameters together; the forward-only image tower runs
    once per chunk, not twice, and the image parameters keep their bits."""
    from clip_event_amd import functional as F
    from clip_event_amd.engine import train_step
    from clip_event_amd.optim import FusedSGD
    batch = _batch(6)
    out = {}
    for mb in (2, None):
        m, sd = _mk()
        m.lock_image_tower()
        opt = FusedSGD(m, lr=0.05, momentum=0.9, max_norm=1.0)
        calls = []
        inner = F._tower_forward_infer
        F._tower_forward_infer = lambda model, desc, tag, *a: (calls.append(tag), inner(model, desc, tag, *a))[1]
        try:
            ld = train_step(m, _crit(), opt, *batch, micro_batch=mb)
            torch.cuda.synchronize()
        finally:
            F._tower_forward_infer = inner
        out[mb] = (m, {k: float(v) for k, v in ld.items()}, calls)
        assert all(_bits_equal(p, sd[n]) for n, p in m.named_parameters() if n.startswith("visual."))
    (m, ld, calls), (m_ref, ld_ref, calls_ref) = out[2], out[None]
    assert sorted(calls) == ["text"] * 3 + ["vision"] * 3, calls          # pass 1: both towers per chunk; pass 3: the text tower with its stash
    assert calls_ref == ["vision"]
    assert sorted(ld) == sorted(ld_ref)
    for k in ld_ref:
        print(f"[micro-batch + lock] {k}: chunked {ld[k]:.6f}, unchunked {ld_ref[k]:.6f}")
        assert abs(ld[k] - ld_ref[k]) <= 3e-3 * max(1.0, abs(ld_ref[k])), k
    worst, upd, upd_ref = (0.0, None), [], []
    for (n, p), (_, q) in zip(m.named_parameters(), m_ref.named_parameters()):
        if not p.requires_grad:
            continue
        upd.append((p.detach().cpu() - sd[n]).flatten())
        upd_ref.append((q.detach().cpu() - sd[n]).flatten())
        a, b = m._gview(n), m_ref._gview(n)
        if float(b.norm()) == 0.0:
            assert float(a.abs().max()) == 0.0, n
            continue
        r = _rel(a, b)
        if r > worst[0]:
            worst = (r, n)
    whole = _rel(torch.cat(upd), torch.cat(upd_ref))
    print(f"[micro-batch + lock] worst per-parameter gradient rel-L2 {worst[0]:.3e} at {worst[1]}; update of all trainable "
          f"parameters rel-L2 {whole:.3e}")
    assert worst[0] <= 2e-3, worst
    assert whole <= 2e-3


# ---- groups end to end -----------------------------------------------------------------------------------------------------------

def test_decoupled_groups_hand_over_to_torch_adamw_and_back():
    """``FusedAdam(decoupled=True, groups=no_decay_groups(m, 0.2))`` over a model with a locked image tower, three steps under
    ``WarmupCosineLR`` (which drives every group); the state_dict loads into ``torch.optim.AdamW`` over detached twins in the
    same groups (indices consecutive over the groups' trainable parameters), both take one more step from the same gradients
    and every element agrees within twice the op-level bound (test_fused_sgd_is_a_torch_optimizer's argument: one bound per
    side; the decoupled form has one more U |p|); torch's state loads back with bit-equal moments."""
    from clip_event_amd.optim import FusedAdam, WarmupCosineLR, no_decay_groups
    m, _ = _mk()
    m.lock_image_tower()
    img, txt, yi, yt, ip = _batch(4)
    groups = no_decay_groups(m, 0.2)
    opt = FusedAdam(m, lr=LR, betas=(B1, B2), eps=EPS, max_norm=None, decoupled=True, groups=groups)
    sch = WarmupCosineLR(opt, max_iters=10, warmup_epochs=3)
    assert len(opt.param_groups) == 2

    def backward():
        ld = _crit()(*m(img, txt), yi, yt, index_pos=ip)
        opt.zero_grad()
        sum(ld.values()).backward()

    for _ in range(3):
        backward()
        opt.step()
        sch.step()
    lrs = [g["lr"] for g in opt.param_groups]
    assert lrs[0] == lrs[1] == sch.get_last_lr()[0] and 0 < lrs[0] <= LR
    state = opt.state_dict()
    by_name = dict(m.named_parameters())
    order = [n for g in groups for n in g["params"]]
    assert [g["params"] for g in state["param_groups"]] == [list(range(len(groups[0]["params"]))),
                                                            list(range(len(groups[0]["params"]), len(order)))]
    assert len(state["state"]) == len(order) and all(g["decoupled_weight_decay"] for g in state["param_groups"])
    backward()
    torch.cuda.synchronize()
    before = {n: by_name[n].detach().clone() for n in order}
    grads = {n: by_name[n].grad.detach().clone() for n in order}
    twins = {n: torch.nn.Parameter(before[n].clone()) for n in order}
    for n in order:
        twins[n].grad = grads[n].clone()
    moments = {n: (state["state"][i]["exp_avg"].clone(), state["state"][i]["exp_avg_sq"].clone()) for i, n in enumerate(order)}
    ref = torch.optim.AdamW([{"params": [twins[n] for n in g["params"]]} for g in groups], lr=123.0, weight_decay=7.0)
    ref.load_state_dict(state)
    assert [(g["lr"], g["weight_decay"], g["decoupled_weight_decay"]) for g in ref.param_groups] == [(lrs[0], 0.2, True), (lrs[1], 0.0, True)]
    ref.step()
    opt.step()
    torch.cuda.synchronize()
    worst = 0.0
    for gi, g in enumerate(groups):
        lr, wd = lrs[gi], g["weight_decay"]
        for n in g["params"]:
            p0 = before[n].cpu()
            r64 = adam_ref(p0, grads[n].cpu(), moments[n][0].cpu(), moments[n][1].cpu(), None, 0.0, 4)
            p_ref = p0.double() * (1 - lr * wd) + (r64[0] - p0.double()) * (lr / LR)
            r64 = (p_ref, *r64[1:6], r64[6] * lr / LR)
            bound = 2 * (_adam_bounds(r64)[0] + U * p_ref.abs())
            err = (by_name[n].detach().cpu().double() - twins[n].detach().cpu().double()).abs()
            worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
            assert bool((err <= bound).all()), (n, worst)
            assert bool(((by_name[n].detach().cpu().double() - p_ref).abs() <= bound / 2).all()), n      # this side within its own bound
    print(f"FusedAdam (decoupled, two groups) vs torch.optim.AdamW after state hand-over: worst |difference| / (2 x bound) {worst:.3f}")
    # and back
    m2, _ = _mk()
    m2.lock_image_tower()
    opt2 = FusedAdam(m2, lr=5e-4, max_norm=None, decoupled=True, groups=no_decay_groups(m2, 0.0))
    opt2.load_state_dict(ref.state_dict())
    assert opt2.step_count == 4 and [(g["lr"], g["weight_decay"]) for g in opt2.param_groups] == [(lrs[0], 0.2), (lrs[1], 0.0)]
    s2 = opt2.state_dict()
    for i, st in ref.state_dict()["state"].items():
        assert torch.equal(s2["state"][i]["exp_avg"].cpu(), st["exp_avg"].cpu()), i
        assert torch.equal(s2["state"][i]["exp_avg_sq"].cpu(), st["exp_avg_sq"].cpu()), i


# ---- plan change -----------------------------------------------------------------------------------------------------------------

def test_a_parameter_unfrozen_between_steps_joins_with_zero_moments():
    """``text_projection`` trains in step 1, is frozen for step 2 and unfrozen for step 3: frozen, it keeps its bits; unfrozen, it
    moves again and its moments are those of a parameter that starts from zero at the shared step count 3 (adam_ref with m = v =
    0 within the op-level bound), not a continuation of step 1's; the other parameters move in every step."""
    from clip_event_amd.engine import train_step
    from clip_event_amd.optim import FusedAdam
    m, sd = _mk()
    batch = _batch(4)
    name, other = "text_projection", "visual.proj"
    opt = FusedAdam(m, lr=LR, betas=(B1, B2), eps=EPS, max_norm=None)
    snaps = []
    for step in (1, 2, 3):
        m.text_projection.requires_grad_(step != 2)
        train_step(m, _crit(), opt, *batch)
        torch.cuda.synchronize()
        snaps.append({n: dict(m.named_parameters())[n].detach().clone() for n in (name, other)})
        assert len(opt.param_groups[0]["params"]) == len(sd) - (step == 2)
    assert not _bits_equal(snaps[0][name], sd[name]) and _bits_equal(snaps[1][name], snaps[0][name])
    assert not _bits_equal(snaps[2][name], snaps[1][name])
    assert not _bits_equal(snaps[1][other], snaps[0][other]) and not _bits_equal(snaps[2][other], snaps[1][other])
    g = m.text_projection.grad.detach().cpu()
    zero = torch.zeros_like(g)
    ref = adam_ref(snaps[1][name].cpu(), g, zero, zero, None, 0.0, 3)
    bp, bm, bv = _adam_bounds(ref)
    st = opt.state_dict()["state"]
    idx = [n for n, _ in m.named_parameters()].index(name)
    for what, got, want, bound in (("master", snaps[2][name], ref[0], bp), ("exp_avg", st[idx]["exp_avg"], ref[1], bm),
                                   ("exp_avg_sq", st[idx]["exp_avg_sq"], ref[2], bv)):
        err = (got.cpu().double() - want).abs()
        assert bool((err <= bound).all()), (what, float((err / bound.clamp_min(1e-300)).max()))


# ---- two ranks -------------------------------------------------------------------------------------------------------------------

@pytest.mark.timeout(900)
def test_two_rank_step_with_a_locked_image_tower():
    codes, outs = run_ranks("partial_ddp_child.py", "locked")
    for out in outs:
        print(out[-3000:])
    assert codes == [0, 0]
