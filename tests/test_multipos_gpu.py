"""GPU: several positive captions per image through the model -- the fused multi-positive head against logits +
``CriterionMultiPositive``, the micro-batched step, two images that share a group, the one-positive layout against the 'ce'
step, ``CriterionSigmoid(multi_positive=True)`` fused against logits, the refusal of the per-instance layout, and two ranks
(tests/multipos_ddp_child.py).  Tiny oracle geometry as tests/test_sigmoid_gpu.py's with embed dim 128, B = 4 and the
(num_pos, num_neg) = (2, 2) layout of ``distributed.global_groups``."""
import pytest
import torch

from tests.multipos_ref import multipos_loss, positives
from tests.test_ddp_gpu import run_ranks

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CFG_ARGS = (128, 64, 2, 128, 32, 20, 512, 128, 2, 3)


def _cfg():
    from oracle import clip_oracle as O
    return O.ClipConfig(*CFG_ARGS)


def _mk(bias=None, seed=31):
    from oracle import clip_oracle as O
    from clip_event_amd.model import build_model
    sd = O.init_params(_cfg(), seed)
    m = build_model({k: v.clone() for k, v in sd.items()}).to(DEV)
    if bias is not None:
        m.enable_logit_bias(bias)
    return m


def _batch(B=4, num_pos=2, num_neg=2):
    """(image, text, groups_per_image, groups_per_text, index_pos)"""
    from clip_event_amd import distributed as D, synthetic as S
    cfg = _cfg()
    K = num_pos + num_neg
    img = S.synthetic_images(B, cfg.image_resolution, seed=1).to(DEV)
    txt = S.synthetic_tokens(B * K, cfg.context_length, cfg.vocab_size, seed=2, min_len=2).to(DEV)
    gi, gt, ip = D.global_groups(B, num_pos, num_neg, device=DEV, rank_=0)
    return img, txt, gi, gt, ip


def _rel(a, b):
    a, b = a.double().flatten().cpu(), b.double().flatten().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _step_gradients(m, crit, batch, micro_batch=None):
    """(losses as floats, flat gradient) of one ``train_step`` with FusedAdam at lr 0: nothing moves."""
    from clip_event_amd.engine import train_step
    from clip_event_amd.optim import FusedAdam
    ld = train_step(m, crit, FusedAdam(m, lr=0.0, max_norm=1.0), *batch, micro_batch=micro_batch)
    torch.cuda.synchronize()
    return {k: float(v.detach()) for k, v in ld.items()}, m._flat_grad.detach().clone()


def _count(monkeypatch, name):
    from clip_event_amd import engine
    calls = []
    inner = getattr(engine, name)
    monkeypatch.setattr(engine, name, lambda *a: (calls.append(1), inner(*a))[1])
    return calls


def _fused_against_logits(monkeypatch, crit, batch, head, keys, scalars, bias=None):
    """``train_step`` on the fused head and with CE_FUSED_HEAD=0 (logits + criterion): the bounds of
    tests/test_sigmoid_gpu.py::test_fused_sigmoid_head_equals_logits_plus_criterion_path -- losses 1e-5 max(1, |loss|), flat gradient
    rel-L2 5e-3 (the towers' backward rounds the feature gradient to bf16 first), the head's scalar gradients, which no tower
    touches, 2e-5."""
    calls = _count(monkeypatch, head)
    out = {}
    for fused in ("1", "0"):
        if fused == "0":
            monkeypatch.setenv("CE_FUSED_HEAD", "0")
        m = _mk(bias)
        ld, g = _step_gradients(m, crit, batch)
        assert len(calls) == 1                                     # the fused head ran in the first pass and only there
        out[fused] = (ld, g, m)
    (ld_f, g_f, m_f), (ld_g, g_g, m_g) = out["1"], out["0"]
    assert sorted(ld_f) == sorted(ld_g) == keys
    for k in keys:
        print(f"[{crit.kind}] {k}: fused {ld_f[k]:.7f}, logits + criterion {ld_g[k]:.7f}")
        assert abs(ld_f[k] - ld_g[k]) < 1e-5 * max(1.0, abs(ld_g[k])), k
    rel = _rel(g_f, g_g)
    print(f"[{crit.kind}] flat gradient rel-L2 fused vs general: {rel:.3e}")
    assert rel < 5e-3
    for n in scalars:
        a, b = float(m_f._gview(n)), float(m_g._gview(n))
        print(f"[{crit.kind}] d{n}: fused {a:.7e}, general {b:.7e}")
        assert b != 0.0 and abs(a - b) < 2e-5 * abs(b), n


def test_fused_multipos_head_equals_logits_plus_criterion_path(monkeypatch):
    from clip_event_amd.losses import CriterionMultiPositive
    _fused_against_logits(monkeypatch, CriterionMultiPositive(), _batch(), "multipos_contrastive_losses", ["loss_i", "loss_t"],
                          ("logit_scale",))


def test_sigmoid_multi_positive_fused_equals_logits_plus_criterion_path(monkeypatch):
    from clip_event_amd.losses import CriterionSigmoid
    _fused_against_logits(monkeypatch, CriterionSigmoid(multi_positive=True), _batch(), "sigmoid_contrastive_losses", ["loss_sig"],
                          ("logit_bias", "logit_scale"), bias=-10.0)


def test_micro_batched_step_gives_the_unchunked_loss_and_gradients():
    """``micro_batch=2`` on B = 4 against the unchunked step under tests/test_micro_batch_gpu.py's rule: losses within
    3e-3 max(1, |loss|), per parameter rel-L2 <= 2e-3, exactly zero where the unchunked gradient is."""
    from clip_event_amd.losses import CriterionMultiPositive
    batch = _batch()
    m = _mk()
    ld, g = _step_gradients(m, CriterionMultiPositive(), batch, micro_batch=2)
    m_ref = _mk()
    ld_ref, g_ref = _step_gradients(m_ref, CriterionMultiPositive(), batch)
    assert sorted(ld) == sorted(ld_ref) == ["loss_i", "loss_t"]
    for k in ld:
        print(f"[multipos micro-batch] {k}: chunked {ld[k]:.6f}, unchunked {ld_ref[k]:.6f}")
        assert abs(ld[k] - ld_ref[k]) <= 3e-3 * max(1.0, abs(ld_ref[k]))
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
    print(f"[multipos micro-batch] worst per-parameter gradient rel-L2 {worst[0]:.3e} at {worst[1]}")
    assert worst[0] <= 2e-3, worst


def test_two_images_sharing_a_group_have_each_others_texts_as_positives():
    """Images 0 and 1 carry one id: the two positive texts of each are positives of both (four per image row, two image
    positives per text row).  The head's losses on the model's own features equal the fp64 reference's at 1e-5, and differ from
    the losses of the unshared layout."""
    from clip_event_amd import engine
    from clip_event_amd.losses import CriterionMultiPositive
    img, txt, gi, gt, ip = _batch()
    gi2, gt2 = gi.clone(), gt.clone()
    gi2[1] = gi[0]
    gt2[4:6] = gi[0]
    assert positives(gi2, gt2).sum(1).tolist() == [4, 4, 2, 2] and positives(gt2[ip], gi2).sum(1).tolist() == [2, 2, 2, 2, 1, 1, 1, 1]
    m = _mk()
    with torch.no_grad():
        fi, ft = m.encode_both(img, txt)
        shared = engine._criterion_from_features(m, CriterionMultiPositive(), fi, ft, gi2, gt2, ip, True, None)
        plain = engine._criterion_from_features(m, CriterionMultiPositive(), fi, ft, gi, gt, ip, True, None)
    torch.cuda.synchronize()
    ls, fi, ft = m.logit_scale.detach().cpu(), fi.float().cpu(), ft.float().cpu()
    want_i = float(multipos_loss(fi, ft, ls, gi2.cpu(), gt2.cpu()))
    want_t = float(multipos_loss(ft, fi, ls, gt2.cpu(), gi2.cpu(), ip.cpu()))
    print(f"[multipos shared group] loss_i {float(shared['loss_i']):.7f} (fp64 {want_i:.7f}, unshared {float(plain['loss_i']):.7f}), "
          f"loss_t {float(shared['loss_t']):.7f} (fp64 {want_t:.7f}, unshared {float(plain['loss_t']):.7f})")
    assert abs(float(shared["loss_i"]) - want_i) < 1e-5 * abs(want_i)
    assert abs(float(shared["loss_t"]) - want_t) < 1e-5 * abs(want_t)
    assert abs(float(shared["loss_i"]) - float(plain["loss_i"])) > 1e-4 * abs(want_i)


def test_one_positive_layout_gives_the_ce_step(monkeypatch):
    """(num_pos, num_neg) = (1, 3): the multi-positive step's losses and gradients are the 'ce' step's on the fused path
    (CE_FUSED_HEAD=1: below 2^17 logits 'ce' would take the three-launch head), at the fused-against-logits bounds."""
    from oracle import clip_oracle as O
    from clip_event_amd.losses import CriterionContrastive, CriterionMultiPositive
    monkeypatch.setenv("CE_FUSED_HEAD", "1")
    calls = _count(monkeypatch, "fused_contrastive_losses")
    img, txt, gi, gt, ip = _batch(4, 1, 3)
    yi, yt, ip_ce = (t.to(DEV) for t in O.build_labels(4, 1, 3, True))
    assert torch.equal(ip, ip_ce)
    m_ce, m_mp = _mk(), _mk()
    ld_ce, g_ce = _step_gradients(m_ce, CriterionContrastive("ce"), (img, txt, yi, yt, ip_ce))
    ld_mp, g_mp = _step_gradients(m_mp, CriterionMultiPositive(), (img, txt, gi, gt, ip))
    assert len(calls) == 1 and sorted(ld_ce) == sorted(ld_mp) == ["loss_i", "loss_t"]
    for k in ld_ce:
        print(f"[multipos vs ce] {k}: multipos {ld_mp[k]:.7f}, ce {ld_ce[k]:.7f}")
        assert abs(ld_mp[k] - ld_ce[k]) < 1e-5 * max(1.0, abs(ld_ce[k])), k
    rel = _rel(g_mp, g_ce)
    a, b = float(m_mp._gview("logit_scale")), float(m_ce._gview("logit_scale"))
    print(f"[multipos vs ce] flat gradient rel-L2 {rel:.3e}, dlogit_scale {a:.7e} vs {b:.7e}")
    assert rel < 5e-3
    assert b != 0.0 and abs(a - b) < 2e-5 * abs(b)


@pytest.mark.parametrize("fused", ["1", "0"])
def test_per_instance_layout_is_refused(fused, monkeypatch):
    from clip_event_amd.engine import contrastive_step_losses
    from clip_event_amd.losses import CriterionMultiPositive
    monkeypatch.setenv("CE_FUSED_HEAD", fused)
    m = _mk()
    m.set_hyps(False, False, False)
    with pytest.raises(RuntimeError, match="constrastive_overbatch=True"):
        contrastive_step_losses(m, CriterionMultiPositive(), *_batch())
    with pytest.raises(RuntimeError, match="constrastive_overbatch=True"):
        CriterionMultiPositive()(torch.zeros(4, 16, device=DEV), torch.zeros(16, 4, device=DEV), torch.arange(4), torch.arange(16),
                                 constrastive_overbatch=False)


# ---- two ranks -------------------------------------------------------------------------------------------------------------------

@pytest.mark.timeout(900)
def test_two_rank_multipos_step_equals_the_concatenated_batch():
    codes, outs = run_ranks("multipos_ddp_child.py", "p2n2")
    for out in outs:
        print(out[-3000:])
    assert codes == [0, 0]
    assert "[p2n2] OK" in outs[0]
