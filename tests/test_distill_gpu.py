"""GPU: distillation through the model -- ``train_step(distill=Distillation(teacher))`` on the fused distillation head against
logits + ``CriterionDistill``, the frozen teacher, weight 0, precomputed teacher features, the micro-batched step, patch dropout
on the student, the sigmoid criterion, a teacher of another resolution, and two ranks (tests/distill_ddp_child.py).  Tiny oracle
geometry as tests/test_sigmoid_gpu.py's with student embed dim 128 and a teacher of embed dim 256."""
import pytest
import torch

from tests import distill_ref as R
from tests.test_ddp_gpu import run_ranks

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
STUDENT = (128, 64, 2, 128, 32, 20, 512, 128, 2, 3)
TEACHER = (256, 64, 2, 128, 32, 20, 512, 128, 2, 3)


def _mk(args=STUDENT, seed=31):
    from oracle import clip_oracle as O
    from clip_event_amd.model import build_model
    sd = O.init_params(O.ClipConfig(*args), seed)
    return build_model({k: v.clone() for k, v in sd.items()}).to(DEV), sd


def _batch(B, K=1, res=64):
    from oracle import clip_oracle as O
    from clip_event_amd import synthetic as S
    img = S.synthetic_images(B, res, seed=1).to(DEV)
    txt = S.synthetic_tokens(B * K, 20, 512, seed=2, min_len=2).to(DEV)
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


def _step(m, batch, distill, crit=None, **kw):
    """(losses as floats, flat gradient) of one ``train_step`` with FusedAdam at lr 0: nothing moves."""
    from clip_event_amd.engine import train_step
    from clip_event_amd.optim import FusedAdam
    ld = train_step(m, crit or _crit(), FusedAdam(m, lr=0.0, max_norm=1.0), *batch, distill=distill, **kw)
    torch.cuda.synchronize()
    return {k: float(v.detach()) for k, v in ld.items()}, m._flat_grad.detach().clone()


def _distill(weight=1.0, seed=77):
    from clip_event_amd.engine import Distillation
    teacher, sd = _mk(TEACHER, seed)
    return Distillation(teacher, weight=weight), sd


@pytest.mark.parametrize("K", [1, 3])
def test_fused_distillation_equals_logits_plus_criterion_path(K, monkeypatch):
    """``train_step`` through ``DistillHeadFn`` and through logits + ``CriterionDistill`` (CE_FUSED_HEAD=0): the same losses (1e-5)
    and flat gradients (rel-L2 5e-3: the towers' backward rounds the feature gradient to bf16 first), the scale gradient, which no
    tower touches, to 2e-5 -- test_sigmoid_gpu.py's bounds -- and the losses equal the fp64 reference on the models' own features."""
    from clip_event_amd import engine
    batch = _batch(5, K)
    distill, _ = _distill()
    calls, out = [], {}
    inner = engine.distill_losses
    monkeypatch.setattr(engine, "distill_losses", lambda *a: (calls.append(1), inner(*a))[1])
    for fused in ("1", "0"):
        monkeypatch.setenv("CE_FUSED_HEAD", fused)
        m, _ = _mk()
        ld, g = _step(m, batch, distill)
        assert len(calls) == 1                                     # the fused head ran in the first pass and only there
        out[fused] = (ld, g, m)
    (ld_f, g_f, m_f), (ld_g, g_g, m_g) = out["1"], out["0"]
    assert sorted(ld_f) == sorted(ld_g) == ["loss_dist_i", "loss_dist_t", "loss_i", "loss_t"]
    with torch.no_grad():
        fi, ft = m_f.encode_both(batch[0], batch[1])
        tfi, tft = distill.encode(batch[0], batch[1])
    ls, tls = m_f.logit_scale.detach().cpu(), distill.logit_scale("cpu")
    want = {"loss_dist_i": float(R.distill_loss(fi.cpu(), ft.cpu(), ls, tfi.cpu(), tft.cpu(), tls)),
            "loss_dist_t": float(R.distill_loss(ft.cpu(), fi.cpu(), ls, tft.cpu(), tfi.cpu(), tls, batch[4].cpu()))}
    for k in ("loss_dist_i", "loss_dist_t"):
        print(f"[distill K={K}] {k}: fused {ld_f[k]:.7f}, logits + criterion {ld_g[k]:.7f}, fp64 on the features {want[k]:.7f}")
        assert abs(ld_f[k] - ld_g[k]) < 1e-5 * max(1.0, abs(ld_g[k]))
        assert abs(ld_f[k] - want[k]) < 1e-5 * max(1.0, abs(want[k]))
    rel = _rel(g_f, g_g)
    a, b = float(m_f._gview("logit_scale")), float(m_g._gview("logit_scale"))
    print(f"[distill K={K}] flat gradient rel-L2 fused vs general {rel:.3e}; dlogit_scale fused {a:.7e}, general {b:.7e}")
    assert rel < 5e-3
    assert b != 0.0 and abs(a - b) < 2e-5 * abs(b)


def test_train_step_adds_the_keys_and_leaves_the_teacher_alone():
    from clip_event_amd.engine import train_step
    from clip_event_amd.optim import FusedAdam
    distill, tsd = _distill(weight=0.7)
    m, sd = _mk()
    ld = train_step(m, _crit(), FusedAdam(m, lr=1e-3, max_norm=1.0), *_batch(4, 3), distill=distill)
    torch.cuda.synchronize()
    assert sorted(ld) == ["loss_dist_i", "loss_dist_t", "loss_i", "loss_t"]
    assert all(torch.isfinite(v.detach()).item() and float(v.detach()) > 0 for v in ld.values())
    for n, p in distill.teacher.named_parameters():
        assert p.grad is None and not p.requires_grad and _bits_equal(p, tsd[n]), n
    assert not distill.teacher.training
    assert not _bits_equal(m.visual.proj, sd["visual.proj"])                     # the student did move


def test_weight_zero_is_the_plain_step():
    """``weight=0``: ``loss_i`` / ``loss_t`` and the gradients of the step without distillation (loss 1e-5, flat gradient rel-L2
    5e-3, test_sigmoid_gpu.py's bounds between two paths; here the same path runs twice and float atomics alone differ)."""
    batch = _batch(5, 3)
    distill, _ = _distill(weight=0.0)
    m, _ = _mk()
    ld, g = _step(m, batch, distill)
    m0, _ = _mk()
    ld0, g0 = _step(m0, batch, None)
    assert ld["loss_dist_i"] == 0.0 and ld["loss_dist_t"] == 0.0
    for k in ("loss_i", "loss_t"):
        assert abs(ld[k] - ld0[k]) < 1e-5 * max(1.0, abs(ld0[k])), k
    rel = _rel(g, g0)
    print(f"[distill weight 0] flat gradient rel-L2 against the plain step {rel:.3e}")
    assert rel < 5e-3
    a, b = float(m._gview("logit_scale")), float(m0._gview("logit_scale"))
    assert abs(a - b) < 2e-5 * abs(b)


def test_teacher_features_equal_the_teacher_pass():
    from clip_event_amd.engine import Distillation
    batch = _batch(4, 3)
    distill, _ = _distill()
    m, _ = _mk()
    ld, g = _step(m, batch, distill)
    feats = distill.encode(batch[0], batch[1])
    given = Distillation(None, logit_scale=float(distill.teacher.logit_scale.detach()))
    m2, _ = _mk()
    ld2, g2 = _step(m2, batch, given, teacher_features=feats)
    for k in ("loss_dist_i", "loss_dist_t"):
        assert abs(ld[k] - ld2[k]) <= 1e-6 * max(1.0, abs(ld[k])), k
    assert _rel(g2, g) < 1e-5


def test_micro_batched_step_gives_the_unchunked_loss_and_gradients():
    """``micro_batch=2`` on B = 4 against the unchunked step under tests/test_micro_batch_gpu.py's rule: losses within
    3e-3 max(1, |loss|), per parameter rel-L2 <= 2e-3, exactly zero where the unchunked gradient is."""
    batch = _batch(4, 3)
    distill, _ = _distill()
    m, _ = _mk()
    ld, g = _step(m, batch, distill, micro_batch=2)
    m_ref, _ = _mk()
    ld_ref, g_ref = _step(m_ref, batch, distill)
    assert sorted(ld) == sorted(ld_ref)
    for k in ld_ref:
        print(f"[distill micro-batch] {k}: chunked {ld[k]:.6f}, unchunked {ld_ref[k]:.6f}")
        assert abs(ld[k] - ld_ref[k]) <= 3e-3 * max(1.0, abs(ld_ref[k])), k
    worst = (0.0, "")
    for n, p in m_ref.named_parameters():
        o = m_ref._offsets[n]
        a, b = g[o:o + p.numel()], g_ref[o:o + p.numel()]
        if float(b.norm()) == 0.0:
            assert float(a.abs().max()) == 0.0, n
            continue
        worst = max(worst, (_rel(a, b), n))
    print(f"[distill micro-batch] worst per-parameter gradient rel-L2 {worst[0]:.3e} at {worst[1]}")
    assert worst[0] <= 2e-3, worst


def test_student_patch_dropout_leaves_the_teacher_features_whole(monkeypatch):
    """The student drops half its patches; the teacher features that reach the head are its ``eval`` features of the whole images,
    to 1e-6 relative L2 (the same kernels on the same inputs)."""
    from clip_event_amd import engine
    batch = _batch(4, 1)
    distill, _ = _distill()
    want = distill.encode(batch[0], batch[1])
    seen = []
    inner = engine._distill_from_features
    monkeypatch.setattr(engine, "_distill_from_features", lambda model, d, fi, ft, tfi, tft, *a: (seen.append((tfi, tft)), inner(model, d, fi, ft, tfi, tft, *a))[1])
    m, _ = _mk()
    m.set_patch_dropout(0.5, seed=3)
    ld, _ = _step(m, batch, distill)
    assert len(seen) == 1 and _rel(seen[0][0], want[0]) <= 1e-6 and _rel(seen[0][1], want[1]) <= 1e-6
    assert seen[0][0].shape == want[0].shape and not seen[0][0].requires_grad
    assert all(v == v for v in ld.values()) and "loss_dist_i" in ld


def test_distillation_beside_the_sigmoid_criterion():
    from clip_event_amd.losses import CriterionSigmoid
    batch = _batch(5, 3)
    distill, _ = _distill()
    m, _ = _mk()
    m.enable_logit_bias(-10.0)
    ld, g = _step(m, batch, distill, crit=CriterionSigmoid())
    assert sorted(ld) == ["loss_dist_i", "loss_dist_t", "loss_sig"]
    m2, _ = _mk()
    ld2, _ = _step(m2, batch, distill)
    for k in ("loss_dist_i", "loss_dist_t"):                       # computed from the features alone: the criterion does not enter
        assert abs(ld[k] - ld2[k]) <= 1e-6 * max(1.0, abs(ld[k])), k
    assert float(g.abs().max()) > 0 and bool(torch.isfinite(g).all())


def test_teacher_of_another_resolution_needs_teacher_image():
    from clip_event_amd.engine import Distillation, train_step
    from clip_event_amd.optim import FusedAdam
    teacher, _ = _mk((256, 96, 2, 128, 32, 20, 512, 128, 2, 3), 5)
    distill = Distillation(teacher)
    m, _ = _mk()
    batch = _batch(4, 1)
    with pytest.raises(ValueError, match="teacher_image"):
        train_step(m, _crit(), FusedAdam(m, lr=0.0), *batch, distill=distill)
    big = _batch(4, 1, res=96)[0]
    ld = train_step(m, _crit(), FusedAdam(m, lr=0.0), *batch, distill=distill, teacher_image=big)
    torch.cuda.synchronize()
    assert float(ld["loss_dist_i"].detach()) > 0


# ---- two ranks -------------------------------------------------------------------------------------------------------------------

@pytest.mark.timeout(900)
@pytest.mark.parametrize("case", ["k1", "k3", "k3g"])
def test_two_rank_distillation_step_equals_the_concatenated_batch(case):
    """k1 / k3: the fused head forced (CE_FUSED_HEAD=1); k3g: logits + ``CriterionDistill`` across the ranks (CE_FUSED_HEAD=0)."""
    codes, outs = run_ranks("distill_ddp_child.py", case)
    for out in outs:
        print(out[-3000:])
    assert codes == [0, 0]
    assert f"[{case}] OK" in outs[0]
