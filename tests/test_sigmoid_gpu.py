"""GPU: the sigmoid pairwise loss through the model -- the fused sigmoid head against logits + ``CriterionSigmoid``, the learnable
``logit_bias`` through FusedAdam, the micro-batched step, the weight EMA, a locked tower, a checkpoint, the error without the
bias, the untouched 'ce' step, and two ranks (tests/sigmoid_ddp_child.py).  Tiny oracle geometry as tests/test_partial_gpu.py's
(2 image blocks, 3 text blocks, width 128) with embed dim 128, the smallest the fused head takes."""
import numpy as np
import pytest
import torch

from tests.sigmoid_ref import reference
from tests.test_ddp_gpu import run_ranks

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CFG_ARGS = (128, 64, 2, 128, 32, 20, 512, 128, 2, 3)
ULP10 = float(np.spacing(np.float32(10.0)))          # the bias lives near -10: one fp32 step there


def _cfg():
    from oracle import clip_oracle as O
    return O.ClipConfig(*CFG_ARGS)


def _mk(bias=-10.0, seed=31):
    """(model, its initial state dict); ``bias`` None: the model without ``logit_bias``."""
    from oracle import clip_oracle as O
    from clip_event_amd.model import build_model
    sd = O.init_params(_cfg(), seed)
    m = build_model({k: v.clone() for k, v in sd.items()}).to(DEV)
    if bias is not None:
        m.enable_logit_bias(bias)
    return m, sd


def _batch(B, K=1):
    from oracle import clip_oracle as O
    from clip_event_amd import synthetic as S
    cfg = _cfg()
    img = S.synthetic_images(B, cfg.image_resolution, seed=1).to(DEV)
    txt = S.synthetic_tokens(B * K, cfg.context_length, cfg.vocab_size, seed=2, min_len=2).to(DEV)
    yi, yt, ip = (t.to(DEV) for t in O.build_labels(B, 1, K - 1, True))
    return img, txt, yi, yt, ip


def _crit():
    from clip_event_amd.losses import CriterionSigmoid
    return CriterionSigmoid()


def _rel(a, b):
    a, b = a.double().flatten().cpu(), b.double().flatten().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _bits_equal(a, b):
    return torch.equal(a.detach().cpu().contiguous().view(torch.int32), b.detach().cpu().contiguous().view(torch.int32))


def _step_gradients(m, batch, micro_batch=None):
    """(losses as floats, flat gradient) of one ``train_step`` with FusedAdam at lr 0: nothing moves."""
    from clip_event_amd.engine import train_step
    from clip_event_amd.optim import FusedAdam
    ld = train_step(m, _crit(), FusedAdam(m, lr=0.0, max_norm=1.0), *batch, micro_batch=micro_batch)
    torch.cuda.synchronize()
    return {k: float(v.detach()) for k, v in ld.items()}, m._flat_grad.detach().clone()


@pytest.mark.parametrize("K", [1, 3])
def test_fused_sigmoid_head_equals_logits_plus_criterion_path(K, monkeypatch):
    """``train_step`` through ``SigmoidHeadFn`` and through logits + ``CriterionSigmoid`` (CE_FUSED_HEAD=0): the same loss (1e-5)
    and the same flat gradients (rel-L2 5e-3: the towers' backward rounds the feature gradient to bf16 first) -- the bounds of
    test_small_head_equals_logits_plus_criterion_path -- and the bias and scale gradients, which no tower touches, to 2e-5."""
    from clip_event_amd import engine
    batch = _batch(5, K)
    out = {}
    calls = []
    inner = engine.sigmoid_contrastive_losses
    monkeypatch.setattr(engine, "sigmoid_contrastive_losses", lambda *a: (calls.append(1), inner(*a))[1])
    for fused in ("1", "0"):
        if fused == "0":
            monkeypatch.setenv("CE_FUSED_HEAD", "0")
        m, _ = _mk()
        ld, g = _step_gradients(m, batch)
        assert len(calls) == 1                                     # the fused head ran in the first pass and only there
        out[fused] = (ld, g, m)
    (ld_f, g_f, m_f), (ld_g, g_g, m_g) = out["1"], out["0"]
    assert sorted(ld_f) == sorted(ld_g) == ["loss_sig"]
    print(f"[sigmoid K={K}] fused {ld_f['loss_sig']:.7f}, logits + criterion {ld_g['loss_sig']:.7f}")
    assert abs(ld_f["loss_sig"] - ld_g["loss_sig"]) < 1e-5 * max(1.0, abs(ld_g["loss_sig"]))
    rel = _rel(g_f, g_g)
    print(f"[sigmoid K={K}] flat gradient rel-L2 fused vs general: {rel:.3e}")
    assert rel < 5e-3
    for n in ("logit_bias", "logit_scale"):
        a, b = float(m_f._gview(n)), float(m_g._gview(n))
        print(f"[sigmoid K={K}] d{n}: fused {a:.7e}, general {b:.7e}")
        assert b != 0.0 and abs(a - b) < 2e-5 * abs(b), n


def test_first_adam_step_moves_the_bias_by_what_the_fp64_gradient_implies():
    """One ``train_step`` with FusedAdam (no clip): the first Adam step is lr g / (|g| + eps), g the gradient of the fp64 reference
    on the model's own features.  The bound is the rounding of the stored bias (one fp32 step at 10) plus 1e-5 of the step: with
    lr = 1e-2 that checks the step to 1e-4 of its size."""
    from clip_event_amd.engine import train_step
    from clip_event_amd.optim import FusedAdam
    lr, eps = 1e-2, 1e-8
    m, sd = _mk()
    img, txt, yi, yt, ip = batch = _batch(6, 3)
    with torch.no_grad():
        fi, ft = m.encode_both(img, txt)
    want = reference(fi, ft, m.logit_scale.detach(), m.logit_bias.detach(), yi, None)
    g = float(want[4])
    opt = FusedAdam(m, lr=lr, eps=eps, max_norm=None)
    ld = train_step(m, _crit(), opt, *batch)
    torch.cuda.synchronize()
    assert abs(float(ld["loss_sig"].detach()) - float(want[0])) < 1e-5 * abs(float(want[0]))
    moved = float(m.logit_bias.detach().double()) - (-10.0)
    expect = -lr * g / (abs(g) + eps)
    print(f"[sigmoid adam] fp64 dlogit_bias {g:.6e}: bias moved {moved:.7e}, expected {expect:.7e}")
    assert abs(g) > 1e-3                                            # sign(g) is not in doubt
    assert abs(moved - expect) <= ULP10 + 1e-5 * abs(expect)
    # and the scale, the head range's other slot
    gs = float(want[3])
    moved_s = float(m.logit_scale.detach().double()) - float(sd["logit_scale"].double())
    assert abs(moved_s + lr * gs / (abs(gs) + eps)) <= float(np.spacing(np.float32(2.66))) + 1e-5 * lr


def test_micro_batched_step_gives_the_unchunked_loss_and_gradients():
    """``micro_batch=2`` on B = 4 against the unchunked step under tests/test_micro_batch_gpu.py's rule: losses within
    3e-3 max(1, |loss|), per parameter rel-L2 <= 2e-3, exactly zero where the unchunked gradient is."""
    batch = _batch(4, 3)
    m, _ = _mk()
    ld, g = _step_gradients(m, batch, micro_batch=2)
    m_ref, _ = _mk()
    ld_ref, g_ref = _step_gradients(m_ref, batch)
    assert sorted(ld) == sorted(ld_ref) == ["loss_sig"]
    print(f"[sigmoid micro-batch] chunked {ld['loss_sig']:.6f}, unchunked {ld_ref['loss_sig']:.6f}")
    assert abs(ld["loss_sig"] - ld_ref["loss_sig"]) <= 3e-3 * max(1.0, abs(ld_ref["loss_sig"]))
    worst = (0.0, "")
    for n, p in m_ref.named_parameters():
        o = m_ref._offsets[n]
        a, b = g[o:o + p.numel()], g_ref[o:o + p.numel()]
        if float(b.norm()) == 0.0:
            assert float(a.abs().max()) == 0.0, n
            continue
        r = _rel(a, b)
        if r > worst[0]:
            worst = (r, n)
    print(f"[sigmoid micro-batch] worst per-parameter gradient rel-L2 {worst[0]:.3e} at {worst[1]}")
    assert worst[0] <= 2e-3, worst
    assert float(g_ref[m_ref._offsets["logit_bias"]]) != 0.0


def test_the_weight_average_carries_the_bias():
    """``enable_ema(0.5)``: after one step the average of ``logit_bias`` is 0.5 (-10) + 0.5 (the new bias), to the rounding of a
    value near 10, and ``averaged()`` swaps it into the model."""
    from clip_event_amd.engine import train_step
    from clip_event_amd.optim import FusedAdam
    m, _ = _mk()
    opt = FusedAdam(m, lr=1e-2, max_norm=None)
    opt.enable_ema(0.5)
    train_step(m, _crit(), opt, *_batch(4))
    torch.cuda.synchronize()
    shadow = opt.ema_state_dict()["shadow"]
    assert "logit_bias" in shadow and shadow["logit_bias"].shape == ()
    new = float(m.logit_bias.detach().double())
    avg = float(shadow["logit_bias"].double())
    print(f"[sigmoid ema] bias {new:.7f}, average {avg:.7f}")
    assert new != -10.0 and abs(avg - 0.5 * (-10.0 + new)) <= 2 * ULP10
    with opt.averaged():
        assert _bits_equal(m.logit_bias, shadow["logit_bias"])
    assert float(m.logit_bias.detach().double()) == new


def test_locked_text_tower_still_trains_the_bias():
    from clip_event_amd.engine import train_step
    from clip_event_amd.optim import FusedAdam
    m, sd = _mk()
    m.lock_text_tower()
    ld = train_step(m, _crit(), FusedAdam(m, lr=1e-3, max_norm=1.0), *_batch(5, 3))
    torch.cuda.synchronize()
    assert np.isfinite(float(ld["loss_sig"].detach()))
    from clip_event_amd.model import tower_of
    for n, p in m.named_parameters():
        if tower_of(n) == "text":
            assert p.grad is None and _bits_equal(p, sd[n]), n
    assert float(m.logit_bias) != -10.0 and not _bits_equal(m.logit_scale, sd["logit_scale"])
    assert not _bits_equal(m.visual.proj, sd["visual.proj"])


def test_checkpoint_round_trip_keeps_the_bias(tmp_path):
    from clip_event_amd import checkpoint
    from clip_event_amd.engine import train_step
    from clip_event_amd.optim import FusedAdam
    m, _ = _mk(bias=-9.0)
    opt = FusedAdam(m, lr=1e-2, max_norm=1.0)
    train_step(m, _crit(), opt, *_batch(4))
    torch.cuda.synchronize()
    path = checkpoint.save_model_on_master(m, str(tmp_path), "clipevent", 1, 0.0, opt)
    m2, opt_state, epoch, _ = checkpoint.load_checkpoint(path, device=DEV)
    assert epoch == 1 and float(m.logit_bias) != -9.0
    assert _bits_equal(m2.logit_bias, m.logit_bias) and _bits_equal(m2.logit_scale, m.logit_scale)
    opt2 = FusedAdam(m2, lr=1e-2, max_norm=1.0)
    opt2.load_state_dict(opt_state)
    batch = _batch(4)
    a = train_step(m, _crit(), opt, *batch)
    b = train_step(m2, _crit(), opt2, *batch)
    torch.cuda.synchronize()
    assert abs(float(a["loss_sig"]) - float(b["loss_sig"])) <= 1e-3 * max(1.0, abs(float(a["loss_sig"])))
    assert abs(float(m.logit_bias) - float(m2.logit_bias)) <= 2 * ULP10 + 1e-3 * 1e-2


@pytest.mark.parametrize("fused", ["1", "0"])
def test_sigmoid_loss_without_the_bias_says_what_to_call(fused, monkeypatch):
    from clip_event_amd.engine import contrastive_step_losses
    monkeypatch.setenv("CE_FUSED_HEAD", fused)
    m, _ = _mk(bias=None)
    with pytest.raises(RuntimeError, match="enable_logit_bias"):
        contrastive_step_losses(m, _crit(), *_batch(4))


def test_enable_logit_bias_after_the_first_forward_rebuilds_the_layout():
    """The flat buffers exist already: they are dropped and rebuilt with one more 64-element slot in ``head``; the other
    parameters keep their bits and the features do not change."""
    m, sd = _mk(bias=None)
    img, txt, *_ = _batch(4)
    with torch.no_grad():
        fi, ft = m.encode_both(img, txt)
    head = m._ranges["head"]
    numel = m._flat.numel()
    m.enable_logit_bias()
    assert m._flat is None
    with torch.no_grad():
        fi2, ft2 = m.encode_both(img, txt)
    assert torch.equal(fi, fi2) and torch.equal(ft, ft2)
    assert {"logit_scale", "logit_bias"} == {n for n in m._offsets if m._ranges["head"][0] <= m._offsets[n] < m._ranges["head"][1]}
    assert abs(m._offsets["logit_bias"] - m._offsets["logit_scale"]) == 64
    assert m._ranges["head"][1] - m._ranges["head"][0] == head[1] - head[0] and m._flat.numel() == numel      # inside the 512-element piece
    assert all(_bits_equal(p, sd[n]) for n, p in m.named_parameters() if n != "logit_bias")
    assert m.logit_bias.data_ptr() == m._flat.data_ptr() + 4 * m._offsets["logit_bias"]


def test_sharded_plan_keeps_the_bias_in_the_replicated_head_range():
    """The sharded optimiser step's plan cuts the towers' ranges and updates the ``head`` range on every rank: the bias lies in
    it, in no piece, and the plan's pieces are those of a model without the bias (the towers moved by nothing)."""
    from clip_event_amd import distributed as D
    img, txt, *_ = _batch(2)
    plans = []
    for bias in (None, -10.0):
        m, _ = _mk(bias=bias)
        with torch.no_grad():
            m.encode_both(img, txt)
        plans.append((m, D.ShardPlan(m, 3, 2)))
    (m0, p0), (m1, p1) = plans
    o = m1._offsets["logit_bias"]
    assert p1.head[0] <= o < p1.head[1] and not any(lo <= o < hi for lo, hi in p1.pieces)
    assert p1.pieces == p0.pieces and p1.head == p0.head


def test_ce_step_without_the_bias_is_what_it_was():
    """'No change when off', inside this commit: two models without ``logit_bias``, built and stepped the same way with
    ``CriterionContrastive('ce')``.  Everything in the step that is order-stable is compared bit for bit: the layout (one head
    slot, ``logit_scale``), the loss dict of the 'ce' pair, and the flat parameter buffer after the optimiser step.  The
    backward's LayerNorm and bias sums are float atomics (tests/test_partial_gpu.py ``_spread_rule``), so two backward passes of
    the same model differ in last bits on any commit and Adam's first step turns a last bit into 2 lr; the second model's
    ``step()`` therefore sees the first model's gradient with the clip inert (the rule of tests/test_ema_gpu.py, DESIGN 4f
    "Tests"), and the two models' own gradients
    are held to rel-L2 1e-5 -- reordered fp32 sums of at most a few thousand terms, each within 2^-24 of the sum of magnitudes."""
    from clip_event_amd.engine import train_step
    from clip_event_amd.losses import CriterionContrastive
    from clip_event_amd.optim import FusedAdam
    batch = _batch(4, 3)
    runs, tape = [], []
    for _ in range(2):
        m, _sd = _mk(bias=None)
        opt = FusedAdam(m, lr=1e-3, max_norm=1e9)            # the gradient norm is a float-atomic sum too: the clip stays inert
        inner = opt.step

        def step(closure=None, m=m, inner=inner):
            tape.append(m._flat_grad.detach().clone())
            m._flat_grad.copy_(tape[0])
            return inner(closure)

        opt.step = step
        ld = train_step(m, CriterionContrastive("ce"), opt, *batch)
        torch.cuda.synchronize()
        runs.append((m, {k: float(v.detach()) for k, v in ld.items()}))
    (a, ld_a), (b, ld_b) = runs
    assert sorted(ld_a) == ["loss_i", "loss_t"] and ld_a == ld_b
    assert [n for n in a._offsets if a._ranges["head"][0] <= a._offsets[n] < a._ranges["head"][1]] == ["logit_scale"]
    assert a._offsets == b._offsets and a._flat.numel() == b._flat.numel()
    differ = [n for n, p in a.named_parameters()
              if not _bits_equal(tape[0][a._offsets[n]:a._offsets[n] + p.numel()], tape[1][a._offsets[n]:a._offsets[n] + p.numel()])]
    rel = _rel(tape[1], tape[0])
    print(f"[ce, no bias] two backward passes: flat gradient rel-L2 {rel:.3e}; {len(differ)} parameters differ in some bit: {differ[:8]}")
    assert rel <= 1e-5
    assert _bits_equal(a._flat, b._flat)
    assert not _bits_equal(a.visual.proj, _sd["visual.proj"])                    # and the step did move the parameters


# ---- two ranks -------------------------------------------------------------------------------------------------------------------

@pytest.mark.timeout(900)
@pytest.mark.parametrize("case", ["k1", "k3"])
def test_two_rank_sigmoid_step_equals_the_concatenated_batch(case):
    codes, outs = run_ranks("sigmoid_ddp_child.py", case)
    for out in outs:
        print(out[-3000:])
    assert codes == [0, 0]
    assert f"[{case}] OK" in outs[0]
