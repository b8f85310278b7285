"""GPU: low-rank adapters through the model -- equivalence with a plain model that carries the merged weights, the fused optimisers
on the adapters, the invalidation rule of the merge, the zero-gradient paths of the weight gradient that the adapters' gradients are
made from, the micro-batched step, ``merge_lora()`` and the checkpoint, fp8 operands, and two ranks (tests/lora_ddp_child.py).
Tiny oracle geometry of tests/test_partial_gpu.py: 2 image blocks, 3 text blocks, width 128.

"Exactly summable" adapters: the adapted base matrices rounded to multiples of 2^-12, A and B in {0, +-2^-5}, s = 2.  Then
W0 + s B A is an fp32 number that the merge kernel computes exactly, so the operand copies of the adapter model EQUAL those of a
plain model whose masters are W0 + s B A, and everything the towers compute from them is comparable bit for bit."""
import os

import numpy as np
import pytest
import torch

from tests.test_ddp_gpu import run_ranks
from tests.test_embed_optim_ops import B1, B2, EPS, LR, U, _adam_bounds, adam_ref
from tests.test_lion_ops import B1 as LB1, B2 as LB2, _lion_bounds, lion_ref
from tests.test_sgd_ops import _sgd_bounds, sgd_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CFG_ARGS = (64, 64, 2, 128, 32, 20, 512, 128, 2, 3)
RANK, ALPHA = 4, 8.0          # s = 2


def _cfg():
    from oracle import clip_oracle as O
    return O.ClipConfig(*CFG_ARGS)


def _base_sd(seed=31):
    """The oracle's parameters with every block matrix rounded to multiples of 2^-12."""
    from oracle import clip_oracle as O
    sd = O.init_params(_cfg(), seed)
    for n in sd:
        if "resblocks" in n and n.endswith(("in_proj_weight", "out_proj.weight", "c_fc.weight", "c_proj.weight")):
            sd[n] = torch.round(sd[n] * 4096) / 4096
    return sd


def _plain(sd):
    from clip_event_amd.model import build_model
    return build_model({k: v.clone() for k, v in sd.items()}).to(DEV)


def _fill(m, seed=7, exact=True, b_zero=False):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n in m.lora_parameter_names():
            p = dict(m.named_parameters())[n]
            v = (torch.randint(-1, 2, p.shape, generator=g).float() / 32) if exact else torch.randn(p.shape, generator=g) * 0.05
            if b_zero and n.endswith("lora_B"):
                v = torch.zeros(p.shape)
            p.copy_(v.to(p.device))


def _lora(sd, fill=True, **kw):
    m = _plain(sd)
    kw = {"rank": RANK, "alpha": ALPHA, **kw}
    m.enable_lora(**kw)
    if fill:
        _fill(m)
    return m


def _merged_sd(sd, m):
    """The plain state dict with ``W0 + s B A`` (fp64, exact in fp32 for exactly summable adapters) in place of every adapted W0."""
    pm = {n: p.detach().cpu() for n, p in m.named_parameters()}
    out = {k: v.clone() for k, v in sd.items()}
    s = m.lora_scale()
    for w, a, b in m._lora["entries"]:
        out[w] = (pm[w].double() + s * (pm[b].double() @ pm[a].double())).float()
    return out


def _batch(B=4, K=1):
    from oracle import clip_oracle as O
    from clip_event_amd import synthetic as S
    cfg = _cfg()
    img = S.synthetic_images(B, cfg.image_resolution, seed=1).to(DEV)
    txt = S.synthetic_tokens(B * K, cfg.context_length, cfg.vocab_size, seed=2, min_len=2).to(DEV)
    yi, yt, ip = (t.to(DEV) for t in O.build_labels(B, 1, K - 1, True))
    return img, txt, yi, yt, ip


def _crit():
    from clip_event_amd.losses import CriterionContrastive
    return CriterionContrastive("ce")


def _rel(a, b):
    a, b = a.double().flatten().cpu(), b.double().flatten().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _bits_equal(a, b):
    return torch.equal(a.detach().cpu().contiguous().view(torch.int32), b.detach().cpu().contiguous().view(torch.int32))


def _features(m, batch):
    with torch.no_grad():
        return m.encode_image(batch[0]).clone(), m.encode_text(batch[1]).clone()


def _loss_backward(m, batch, zero="zero_grad"):
    """One forward and backward outside the engine: the loss and the gradient slices by name (adapters after finish_lora_grads)."""
    img, txt, yi, yt, ip = batch
    m._ready()
    if zero == "zero_grad":
        m.zero_grad()
    elif zero == "none":
        m.zero_grad(set_to_none=True)
    li, lt = m(img, txt)
    ld = _crit()(li, lt, yi, yt, index_pos=ip)
    loss = sum(ld.values())
    loss.backward()
    m.finish_lora_grads()
    torch.cuda.synchronize()
    return float(loss.detach()), {n: m._gview(n).detach().clone() for n, _ in m.named_parameters()}


def _adapter_grads_within_bounds(m, grads, tag):
    """A.grad / B.grad against the fp64 formula applied to the dW read back, with tests/test_lora_ops.py's bounds."""
    pm = {n: p.detach().double() for n, p in m.named_parameters()}
    s, worst = m.lora_scale(), [0.0, 0.0]
    for w, a, b in m._lora["entries"]:
        dw = grads[w].double()
        out, inn = dw.shape
        for k, (got, ref, bound) in enumerate(((grads[a], s * (pm[b].t() @ dw), (out + 2) * U * s * (pm[b].abs().t() @ dw.abs())),
                                               (grads[b], s * (dw @ pm[a].t()), (inn + 2) * U * s * (dw.abs() @ pm[a].abs().t())))):
            err = (got.double() - ref).abs()
            assert bool((err <= bound).all()), (tag, w, "AB"[k])
            worst[k] = max(worst[k], float((err / bound.clamp_min(1e-300)).max()))
    print(f"[{tag}] adapter gradients, worst |err| / bound: dA {worst[0]:.3f}, dB {worst[1]:.3f}")


# ---- (a) equivalence with a merged model ------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def reference():
    """The adapter model's loss, gradients and features on the batch, computed once (read-only)."""
    sd = _base_sd()
    m = _lora(sd, freeze_base=False)
    batch = _batch()
    loss, grads = _loss_backward(m, batch)
    return {"sd": sd, "loss": loss, "grads": grads, "features": _features(m, batch), "merged": _merged_sd(sd, m),
            "names": m.lora_parameter_names(), "pm": {n: p.detach().clone() for n, p in m.named_parameters()}, "s": m.lora_scale(),
            "entries": list(m._lora["entries"])}


def test_equals_a_plain_model_with_the_merged_weights(reference):
    """Exactly summable adapters (everything else trainable too): features and loss equal those of a plain model whose masters are
    W0 + s B A; every gradient slice that is no adapter's -- the weight gradients of the frozen adapted matrices included -- is
    bit-equal where two runs of the plain model are bit-equal and within 4 x their spread + 1e-6 (rel-L2) otherwise; the adapters'
    gradients are within the op-level bounds of the fp64 formula applied to the dW read back."""
    batch = _batch()
    twins = []
    for _ in range(2):
        p = _plain(reference["merged"])
        loss, grads = _loss_backward(p, batch)
        twins.append((loss, grads, _features(p, batch), p._flat16.detach().clone()))
    m = _lora(reference["sd"], freeze_base=False)
    m._ready()
    torch.cuda.synchronize()                  # (the W^T copies may come from the auxiliary stream)
    for w, _, _ in reference["entries"]:      # the premise: the same operand bits
        assert torch.equal(m._w16[w].view(torch.int16), p._w16[w].view(torch.int16)), w
        assert torch.equal(m._w16t[w].view(torch.int16), m._w16[w].t().contiguous().view(torch.int16)), w
    assert all(torch.equal(a, b) for a, b in zip(reference["features"], twins[0][2]))
    if twins[0][0] == twins[1][0]:
        assert reference["loss"] == twins[0][0]
    else:
        assert abs(reference["loss"] - twins[0][0]) <= 4 * abs(twins[0][0] - twins[1][0]) + 1e-6
    exact = loose = 0
    for n in twins[0][1]:
        a, b, got = twins[0][1][n], twins[1][1][n], reference["grads"][n]
        # gains and biases are summed with float atomics: two runs of such a slice agree bit for bit only by chance
        # (measured: in_proj_bias / c_proj.bias / ln_1.weight slices differ by 3e-8 .. 6e-8 rel-L2 in some pairs of runs and not in
        # others), so their agreement says nothing about a third run; they always take the spread rule
        if _bits_equal(a, b) and got.dim() != 1:
            assert _bits_equal(got, a), n
            exact += 1
        else:
            spread, r = _rel(b, a), _rel(got, a)
            assert r <= 4 * spread + 1e-6, (n, r, spread)
            loose += 1
    print(f"[merged twin] {exact} slices bit-equal, {loose} within 4 x spread")
    m2 = _lora(reference["sd"], freeze_base=False)
    _, grads = _loss_backward(m2, batch)
    _adapter_grads_within_bounds(m2, grads, "equivalence")
    for n in reference["names"]:
        assert m2._pmap[n].grad is not None and m2._pmap[n].grad.data_ptr() == m2._gview(n).data_ptr()
        assert float(grads[n].abs().max()) > 0.0, n
    for w, _, _ in reference["entries"]:
        assert m2._pmap[w].grad is None


def test_finish_is_idempotent_and_a_noop_without_adapters(reference):
    m = _lora(reference["sd"])
    batch = _batch()
    _, g1 = _loss_backward(m, batch)
    m.finish_lora_grads()
    torch.cuda.synchronize()
    assert all(_bits_equal(m._gview(n), g1[n]) for n in reference["names"])
    p = _plain(reference["sd"])
    p.finish_lora_grads()                       # before any layout, and after
    _loss_backward(p, batch)


def test_an_unfrozen_adapted_matrix_is_refused(reference):
    from clip_event_amd.optim import FusedAdam
    m = _lora(reference["sd"])
    batch = _batch()
    _loss_backward(m, batch)
    opt = FusedAdam(m, lr=LR)
    w = reference["entries"][0][0]
    m._pmap[w].requires_grad_(True)
    with pytest.raises(RuntimeError, match="stays frozen"):
        m.encode_text(batch[1])
    with pytest.raises(RuntimeError, match="stays frozen"):
        opt.step()


# ---- (b) the fused optimisers ---------------------------------------------------------------------------------------------------------

def _optimizer(which, m, wd):
    from clip_event_amd.optim import FusedAdam, FusedLion, FusedSGD
    if which == "adam":
        return FusedAdam(m, lr=LR, betas=(B1, B2), eps=EPS, weight_decay=wd, max_norm=1.0)
    if which == "sgd":
        return FusedSGD(m, lr=LR, momentum=0.9, weight_decay=0.0, max_norm=1.0)
    return FusedLion(m, lr=LR, betas=(LB1, LB2), weight_decay=wd, max_norm=1.0)


@pytest.mark.parametrize("which,steps", [("adam", 3), ("sgd", 1), ("lion", 1)])
def test_clipped_fused_steps_train_the_adapters_only(which, steps):
    """``engine.train_step`` with the clip active (s = 32 makes the adapters' gradient norm exceed 1): every base master keeps its
    bits and ``.grad`` None; ``grad_norm()`` is the fp64 norm of the ADAPTERS' gradients to 1e-5 (tests/test_partial_gpu.py's
    tolerance); after step 1 every adapter is within the op-level bound of the fp64 restatement of the update; the loss of step 2
    differs from step 1's -- a stale merge would repeat it bit for bit."""
    from clip_event_amd.engine import train_step
    sd = _base_sd()
    m = _lora(sd, fill=False, alpha=128.0)
    _fill(m, exact=False)
    names = m.lora_parameter_names()
    start = {n: p.detach().cpu().clone() for n, p in m.named_parameters()}
    wd = 0.01
    opt = _optimizer(which, m, wd)
    batch = _batch()
    losses = []
    for step in range(1, steps + 1):
        ld = train_step(m, _crit(), opt, *batch)
        torch.cuda.synchronize()
        losses.append(float(sum(ld.values())))
        for n, p in m.named_parameters():
            if n not in names:
                assert p.grad is None and _bits_equal(p, start[n]), (step, n)
        if step > 1:
            continue
        grads = {n: m._pmap[n].grad.detach().cpu() for n in names}
        sumsq = sum(float((g.double() ** 2).sum()) for g in grads.values())
        gn = float(opt.grad_norm())
        print(f"[lora {which}] grad_norm {gn:.7f}, fp64 over the adapters' gradients {sumsq ** 0.5:.7f}")
        assert sumsq > 1.0                                                           # the clip is active
        assert abs(gn - sumsq ** 0.5) <= 1e-5 * sumsq ** 0.5
        worst = 0.0
        for n in names:
            zero = torch.zeros_like(start[n])
            if which == "adam":
                ref = adam_ref(start[n], grads[n], zero, zero, float(np.float32(sumsq)), wd, 1)
                bound = _adam_bounds(ref)[0]
            elif which == "sgd":
                ref = sgd_ref(start[n], grads[n], zero, float(np.float32(sumsq)), 0.0, 0.9, 0.0, False, True, lr=LR)
                bound = _sgd_bounds(ref, lr=LR)[0]
            else:
                ref = lion_ref(start[n], grads[n], zero, float(np.float32(sumsq)), wd, lr=LR)
                bound = _lion_bounds(ref, wd, lr=LR)[0]
            err = (m._pmap[n].detach().cpu().double() - ref[0]).abs()
            worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
            assert bool((err <= bound).all()), (n, worst)
        print(f"[lora {which}] step 1 adapters: worst |err| / bound {worst:.3f}")
    if which == "adam":
        assert losses[1] != losses[0] and losses[2] != losses[1], losses
    assert all(not _bits_equal(m._pmap[n], start[n]) for n in names)


# ---- (c) the invalidation rule ----------------------------------------------------------------------------------------------------

def test_every_change_of_an_adapter_reaches_the_next_forward(reference):
    from clip_event_amd.engine import train_step
    from clip_event_amd.optim import FusedAdam
    batch = _batch()
    m = _lora(reference["sd"])
    f0 = _features(m, batch)
    assert all(torch.equal(a, b) for a, b in zip(f0, reference["features"]))
    # an in-place update (a stock optimiser's): _version moves
    name = "visual.transformer.resblocks.1.mlp.c_fc.lora_B"
    tname = "transformer.resblocks.2.attn.in_proj_lora_A"
    with torch.no_grad():
        m._pmap[name].add_(1.0 / 32)
        m._pmap[tname].add_(1.0 / 32)
    f1 = _features(m, batch)
    assert not torch.equal(f1[0], f0[0]) and not torch.equal(f1[1], f0[1])
    # load_lora_state_dict
    m.load_lora_state_dict({"config": m.lora_config(), "state": {n: reference["pm"][n] for n in reference["names"]}})
    f2 = _features(m, batch)
    assert all(torch.equal(a, b) for a, b in zip(f2, f0))
    # averaged(): the average of the adapters is merged on entry, the training adapters again on exit
    opt = FusedAdam(m, lr=LR, max_norm=1.0)
    opt.enable_ema(0.5)
    for _ in range(2):
        train_step(m, _crit(), opt, *batch)
    raw = _features(m, batch)
    shadow = opt.ema_state_dict()["shadow"]
    fresh = _lora(reference["sd"], fill=False)
    fresh.load_lora_state_dict({"config": fresh.lora_config(), "state": {n: shadow[n] for n in reference["names"]}})
    want = _features(fresh, batch)
    with opt.averaged():
        got = _features(m, batch)
        assert all(torch.equal(a, b) for a, b in zip(got, want))
        assert not torch.equal(got[0], raw[0]) and not torch.equal(got[1], raw[1])
    back = _features(m, batch)
    assert all(torch.equal(a, b) for a, b in zip(back, raw))


# ---- (d) the zero-gradient paths --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("path", ["zero_grad", "set_to_none", "first_touch", "first_touch_settled"])
def test_the_weight_gradient_of_an_adapted_matrix_starts_from_zero(path, reference):
    """The dW slice of a frozen adapted matrix is consumed now.  Poisoned with a sentinel before the step, it must not reach the
    adapters' gradients on any path: ``zero_grad()``, ``zero_grad(set_to_none=True)`` followed by the backward's attach,
    ``zero_grad_first_touch()`` (the backward overwrites), and ``zero_grad_first_touch()`` with a tower that sees no backward
    (``_settle_first_touch`` zeroes its slices: the adapters' gradients there are exactly 0)."""
    batch = _batch()
    m = _lora(reference["sd"])
    _loss_backward(m, batch)                                   # builds the buffers, attaches the gradients
    torch.cuda.synchronize()
    for w, _, _ in reference["entries"]:
        m._gview(w).fill_(1.0e6)
    img, txt, yi, yt, ip = batch
    if path == "zero_grad":
        _, grads = _loss_backward(m, batch, zero="zero_grad")
    elif path == "set_to_none":
        _, grads = _loss_backward(m, batch, zero="none")
    else:
        m.zero_grad_first_touch()
        if path == "first_touch":
            li, lt = m(img, txt)
            sum(_crit()(li, lt, yi, yt, index_pos=ip).values()).backward()
        else:                                                  # the text tower alone: the image tower's slices are settled
            m.encode_text(txt).square().sum().backward()
        m._settle_first_touch()
        m.finish_lora_grads()
        torch.cuda.synchronize()
        grads = {n: m._gview(n).detach().clone() for n, _ in m.named_parameters()}
    if path == "first_touch_settled":
        for n in reference["names"]:
            g = grads[n]
            assert bool(torch.isfinite(g).all()) and float(g.abs().max()) < 1.0e3, n
            if n.startswith("visual."):
                assert float(g.abs().max()) == 0.0, n
        return
    _adapter_grads_within_bounds(m, grads, path)
    want = reference["grads"]
    worst = 0.0
    for n in reference["names"]:
        # the reference is (a)'s run of the same weights.  The two differ by the order of the float atomics in the towers' backward
        # (tests/test_micro_batch_gpu.py sees < 1e-5 rel-L2 between such runs); a leaked sentinel of 1e6 is wrong by orders of magnitude
        r = _rel(grads[n], want[n])
        worst = max(worst, r)
        assert r <= 1e-4, (path, n, r)
    print(f"[{path}] adapters' gradients against the reference run: worst rel-L2 {worst:.2e}")


# ---- (e) micro-batched step -------------------------------------------------------------------------------------------------------

def test_micro_batched_step_agrees_with_the_unchunked_one(reference):
    """``micro_batch=2`` of 4: losses within 3e-3 max(1, |loss|), every adapter's gradient within rel-L2 2e-3 of the unchunked step's
    (tests/test_micro_batch_gpu.py's tolerances)."""
    from clip_event_amd.engine import train_step
    from clip_event_amd.optim import FusedAdam
    batch = _batch()
    out = {}
    for mb in (None, 2):
        m = _lora(reference["sd"])
        opt = FusedAdam(m, lr=0.0, max_norm=1.0)
        ld = train_step(m, _crit(), opt, *batch, micro_batch=mb)
        torch.cuda.synchronize()
        out[mb] = ({k: float(v) for k, v in ld.items()}, {n: m._gview(n).detach().clone() for n in reference["names"]})
    for k, v in out[None][0].items():
        assert abs(out[2][0][k] - v) <= 3e-3 * max(1.0, abs(v)), (k, out[2][0][k], v)
    worst = max(_rel(out[2][1][n], out[None][1][n]) for n in reference["names"])
    print(f"[lora micro_batch=2] worst per-adapter gradient rel-L2 {worst:.3e}")
    assert worst <= 2e-3


# ---- (f) merge_lora and the checkpoint --------------------------------------------------------------------------------------------

def test_merge_lora_gives_a_plain_model(reference, tmp_path):
    """Random (not exactly summable) adapters: after ``merge_lora()`` the keys are the reference's, every flag is what it was, the
    adapted masters are W0 + s B A within the merge kernel's fp32 bound, and the features are those of the adapter model to rel-L2
    2^-8 -- the masters were rounded to fp32 before the bf16 cast, so an operand can land on the neighbouring bf16 number (one
    unit, 2^-8 relative), and only where the fp32 rounding crossed a bf16 tie."""
    from clip_event_amd.checkpoint import checkpoint_dict, load_checkpoint
    batch = _batch()
    sd = reference["sd"]
    m = _lora(sd, fill=False)
    _fill(m, exact=False)
    before = _features(m, batch)
    pm = {n: p.detach().cpu().clone() for n, p in m.named_parameters()}
    entries, s = list(m._lora["entries"]), m.lora_scale()
    # the checkpoint round trip of the adapter model first
    path = os.path.join(tmp_path, "lora_1.pth")
    torch.save(checkpoint_dict(m, None, "lora", 1, 0.0), path)
    m2, _, _, _ = load_checkpoint(path, device=DEV)
    assert m2.lora_config() == m.lora_config()
    assert all(_bits_equal(p, pm[n]) for n, p in m2.named_parameters())
    assert all(torch.equal(a, b) for a, b in zip(_features(m2, batch), before))
    m.merge_lora()
    assert set(m.state_dict()) == set(sd) and m.lora_config() is None and all(p.requires_grad for p in m.parameters())
    after = _features(m, batch)
    now = {n: p.detach().cpu() for n, p in m.named_parameters()}
    for w, a, b in entries:
        ref = pm[w].double() + s * (pm[b].double() @ pm[a].double())
        mag = pm[w].double().abs() + s * (pm[b].double().abs() @ pm[a].double().abs())
        assert bool(((now[w].double() - ref).abs() <= (RANK + 2) * U * mag).all()), w
    assert all(_bits_equal(now[n], pm[n]) for n in sd if n not in {e[0] for e in entries})
    rels = [_rel(x, y) for x, y in zip(after, before)]
    print(f"[merge_lora] features against the adapter model: rel-L2 {rels[0]:.2e} (image), {rels[1]:.2e} (text)")
    assert max(rels) <= 2.0 ** -8
    _loss_backward(m, batch)                                   # a plain model again: it trains


# ---- (g) fp8 operands -------------------------------------------------------------------------------------------------------------

def test_fp8_operands_follow_the_adapters(reference, monkeypatch):
    monkeypatch.setenv("CE_FP8", "1")
    batch = _batch()
    m = _lora(reference["sd"], fill=False)
    _fill(m, b_zero=True)
    assert m.fp8 == 1
    f0 = _features(m, batch)
    _fill(m, b_zero=False)
    f1 = _features(m, batch)
    assert not torch.equal(f0[0], f1[0]) and not torch.equal(f0[1], f1[1])
    assert bool(torch.isfinite(f1[0]).all()) and bool(torch.isfinite(f1[1]).all())


# ---- GradSync: the dW range of a frozen adapted matrix is exchanged, and (h) two ranks ---------------------------------------------

@pytest.mark.timeout(900)
def test_two_rank_step_equals_the_single_rank_step():
    codes, outs = run_ranks("lora_ddp_child.py", "lora")
    for out in outs:
        print(out[-3000:])
    assert codes == [0, 0]
    assert "[lora] OK" in outs[0]
