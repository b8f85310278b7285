"""GPU: patch dropout through the model -- ``encode_image`` / ``encode_both`` on the class token and a subset of the
patches, its backward, the draw bookkeeping, the micro-batched step and the fused optimiser.

The reference is the oracle's image tower restated with a keep list (tests/patch_dropout_ref.encode_image_keep); the kept
patches come from the numpy restatement of the sampler.  The bounds are the suite's own for the same code at the same
size: tests/test_model_gpu.py::test_tiny_features_bf16_oracle (features) and ::test_tiny_against_oracle (loss, gradients),
tests/test_micro_batch_gpu.py::_compare_to_unchunked (chunked step)."""
import contextlib

import numpy as np
import pytest
import torch

from tests import patch_dropout_ref as R
from tests.test_micro_batch_gpu import _compare_to_unchunked
from tests.test_model_gpu import _cos, _grad_report, _mk, _rel

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SMALL = (128, 96, 2, 128, 16, 20, 512, 128, 2, 2)          # grid 6: N = 36, T = 37; p = 0.5 keeps 18
LONG = (128, 224, 2, 128, 14, 20, 512, 128, 2, 2)          # N = 256: p = 0.5 gives 129 tokens (long attention), patch 14
SEED, DRAW, PSEED = 5, 3, 11


@pytest.fixture(params=[False, True], ids=["stream32", "stream16"])
def stream16(request, monkeypatch):
    """Both residual-stream formats (fixture of tests/test_forward_only_gpu.py)."""
    monkeypatch.setenv("CE_STREAM16", "1" if request.param else "0")
    return request.param


def _data(cfg, B, K=3):
    from oracle import clip_oracle as O
    from clip_event_amd import synthetic as S
    img = S.synthetic_images(B, cfg.image_resolution, seed=21)
    txt = S.synthetic_tokens(B * K, cfg.context_length, cfg.vocab_size, seed=22, min_len=4)
    return img, txt, O.build_labels(B, 1, K - 1, True)


_REF = {}


def _reference(cfg_args, B, stream16):
    """Computed once per configuration and shared: fp32 restatement (features, losses, gradients) and, per stream format,
    the restatement with the build's rounding points."""
    from oracle import clip_oracle as O
    cfg = O.ClipConfig(*cfg_args)
    key = (cfg_args, B)
    if key not in _REF:
        sd = O.init_params(cfg, SEED)
        img, txt, (yi, yt, ip) = _data(cfg, B)
        N = cfg.grid ** 2
        idx, inv = R.keep_tables(PSEED, DRAW, 0, B, N, max(1, int(N * 0.5)))
        q = {k: v.detach().clone().requires_grad_(True) for k, v in sd.items()}
        fi = R.encode_image_keep(q, cfg, img, idx)
        li, lt = O.logits_from_features(fi, O.encode_text(q, cfg, txt), q["logit_scale"], True)
        ld = O.criterion_contrastive(li, lt, yi, yt, ip)
        sum(ld.values()).backward()
        _REF[key] = dict(idx=idx, inv=inv, f32=fi.detach(), ld={k: float(v.detach()) for k, v in ld.items()},
                         grads={k: v.grad for k, v in q.items()}, sd=sd, cfg=cfg)
    ref = _REF[key]
    if ("same", stream16) not in ref:
        img = _data(ref["cfg"], B)[0]
        with (O.stream_f16() if stream16 else contextlib.nullcontext()), torch.no_grad():
            ref[("same", stream16)] = R.encode_image_keep(ref["sd"], ref["cfg"], img, ref["idx"], bf16=True)
    return ref


def _check_against_restatement(cfg_args, B, stream16):
    from clip_event_amd.losses import CriterionContrastive
    ref = _reference(cfg_args, B, stream16)
    cfg, idx = ref["cfg"], ref["idx"]
    N, keep = cfg.grid ** 2, idx.shape[1]
    m, _ = _mk(cfg, SEED)
    img, txt, (yi, yt, ip) = _data(cfg, B)
    img, txt = img.to(DEV), txt.to(DEV)
    # features from the explicit list, model in eval mode, no grad
    m.eval()
    with torch.no_grad():
        f_list = m.encode_image(img, keep_idx=idx)
    torch.cuda.synchronize()
    same = ref[("same", stream16)]
    print(f"[{cfg_args[1]}/{cfg_args[4]} keep {keep}/{N}] features: rel-l2 vs restatement with the same rounding points "
          f"{_rel(f_list, same):.2e}, vs fp32 {_rel(f_list, ref['f32']):.2e}, cos {_cos(f_list, ref['f32']):.6f}")
    assert _rel(f_list, same) < (6e-3 if stream16 else 5e-3) and _cos(f_list, ref["f32"]) > 0.9995
    # the sampler picks the same patches: bit-identical features
    m.train()
    m.set_patch_dropout(0.5, seed=PSEED)
    assert m.visual.patch_keep() == keep
    with m.pinned_patch_draw(DRAW), torch.no_grad():
        f_sampled = m.encode_image(img)
    assert torch.equal(f_sampled, f_list)
    # contrastive loss and backward, dropping through the sampler
    with m.pinned_patch_draw(DRAW):
        li, lt = m(img, txt)
    ld = CriterionContrastive("ce")(li, lt, yi.to(DEV), yt.to(DEV), index_pos=ip.to(DEV), constrastive_overbatch=True)
    (ld["loss_i"] + ld["loss_t"]).backward()
    torch.cuda.synchronize()
    assert m.patch_draw == 0                      # pinned passes do not move the counter
    for k in ("loss_i", "loss_t"):
        print(f"{k} {float(ld[k].detach()):.5f} (restatement {ref['ld'][k]:.5f})")
        assert abs(float(ld[k].detach()) - ref["ld"][k]) < 2e-2
    worst, rels = _grad_report(m, ref["grads"], f"patch dropout {cfg_args[1]}/{cfg_args[4]}")
    assert worst[0] > 0.98 and np.median(rels) < 0.03
    # positional rows that no sample kept: exactly zero, here and in the restatement
    dropped = np.setdiff1d(np.arange(N), idx.reshape(-1))
    print(f"patches no sample kept: {len(dropped)} of {N}")
    if len(dropped):
        rows = torch.from_numpy(1 + dropped).long()
        assert float(m.visual.positional_embedding.grad.cpu()[rows].abs().max()) == 0.0
        assert float(ref["grads"]["visual.positional_embedding"][rows].abs().max()) == 0.0


def test_small_model_against_the_restatement(stream16):
    _check_against_restatement(SMALL, 4, stream16)


def test_long_attention_and_generic_patch_path(stream16):
    """129 tokens: the shortest length on the long-sequence attention path; patch 14: generic im2col, padded conv1 columns."""
    _check_against_restatement(LONG, 2, stream16)


def test_full_list_equals_dense(stream16):
    """An explicit list of ALL patches runs the new branch at the dense shapes."""
    from oracle import clip_oracle as O
    from clip_event_amd.functional import logits_from_features
    from clip_event_amd.losses import CriterionContrastive
    cfg = O.ClipConfig(*SMALL)
    B = 4
    img, txt, (yi, yt, ip) = _data(cfg, B)
    img, txt = img.to(DEV), txt.to(DEV)
    full = np.tile(np.arange(cfg.grid ** 2), (B, 1))
    crit = CriterionContrastive("ce")
    grads, feats = [], []
    for keep_idx in (None, full):
        m, _ = _mk(cfg, SEED)
        fi, ft = m.encode_both(img, txt, keep_idx=keep_idx)
        li, lt = logits_from_features(fi, ft, m.logit_scale, True)
        ld = crit(li, lt, yi.to(DEV), yt.to(DEV), index_pos=ip.to(DEV), constrastive_overbatch=True)
        (ld["loss_i"] + ld["loss_t"]).backward()
        torch.cuda.synchronize()
        feats.append(fi.detach().clone())
        grads.append({n: p.grad.detach().clone() for n, p in m.named_parameters()})
    assert torch.equal(feats[0], feats[1])
    worst = (0.0, None)
    for n, g in grads[0].items():
        if float(g.norm()) == 0.0:
            assert float(grads[1][n].abs().max()) == 0.0, n
            continue
        r = _rel(grads[1][n], g)
        if r > worst[0]:
            worst = (r, n)
    print(f"full list against dense: worst per-parameter gradient rel-L2 {worst[0]:.3e} at {worst[1]}")
    assert worst[0] <= 1e-6, worst


def test_grad_mode_and_mode_switches(stream16):
    from oracle import clip_oracle as O
    from clip_event_amd.inference import zero_shot
    cfg = O.ClipConfig(*SMALL)
    B = 4
    img, txt, _ = _data(cfg, B, K=1)
    img, txt = img.to(DEV), txt.to(DEV)
    m, _ = _mk(cfg, SEED)
    m.eval()
    with torch.no_grad():
        dense = m.encode_image(img)
        zs_eval = zero_shot(m, img, txt)
    m.set_patch_dropout(0.5, seed=PSEED)
    with torch.no_grad():
        assert torch.equal(m.encode_image(img), dense)              # eval mode: dense
    m.train()
    with m.pinned_patch_draw(DRAW):
        with_grad = m.encode_image(img)
        assert with_grad.requires_grad
        with torch.no_grad():
            without = m.encode_image(img)
    assert torch.equal(with_grad.detach(), without)
    assert not torch.equal(without, dense)
    # a grid pass never drops, even in training mode; the inference helpers neither
    assert tuple(m.encode_image(img, use_grid=True).shape) == (B, 37, cfg.embed_dim)
    zs_train = zero_shot(m, img, txt)
    assert all(torch.equal(a, b) for a, b in zip(zs_train, zs_eval))
    assert m.patch_draw == 0
    # two unpinned training calls: two draws, two keep sets
    with torch.no_grad():
        a, b = m.encode_image(img), m.encode_image(img)
    assert m.patch_draw == 2 and not torch.equal(a, b)
    with m.pinned_patch_draw(0), torch.no_grad():
        assert torch.equal(m.encode_image(img), a)
    # a locked image tower (forward-only even with grad mode on) drops too
    m.lock_image_tower()
    with m.pinned_patch_draw(DRAW):
        locked = m.encode_image(img)
    assert not locked.requires_grad and torch.equal(locked, without)


def test_partly_locked_tower_and_fp8_operands(stream16):
    """The dropped branch under ``stop > 0`` (the backward ends above the input side) and with fp8 operands: the sampler and
    the explicit list still agree bit for bit, the frozen input side gets no gradient, the open block gets one."""
    from oracle import clip_oracle as O
    cfg = O.ClipConfig(*SMALL)
    B = 4
    img = _data(cfg, B)[0].to(DEV)
    idx = R.keep_tables(PSEED, DRAW, 0, B, 36, 18)[0]
    m, _ = _mk(cfg, SEED)
    m.fp8 = 3
    m.lock_image_tower(unlocked_layers=1)
    m.set_patch_dropout(0.5, seed=PSEED)
    with m.pinned_patch_draw(DRAW):
        f = m.encode_image(img)
    assert torch.equal(f.detach(), m.encode_image(img, keep_idx=idx).detach())
    f.square().sum().backward()
    torch.cuda.synchronize()
    P = dict(m.named_parameters())
    assert float(P["visual.transformer.resblocks.1.attn.in_proj_weight"].grad.abs().max()) > 0.0
    assert bool(torch.isfinite(P["visual.proj"].grad).all())
    for n in ("visual.conv1.weight", "visual.positional_embedding", "visual.class_embedding",
              "visual.transformer.resblocks.0.attn.in_proj_weight"):
        assert P[n].grad is None or float(P[n].grad.abs().max()) == 0.0, n


def _step_gradients(m, crit, args, micro_batch, draw):
    """tests/test_micro_batch_gpu._step_gradients with the draw counter set before the measured step."""
    from clip_event_amd.engine import train_step
    from clip_event_amd.optim import FusedAdam
    opt = FusedAdam(m, lr=0.0, max_norm=1.0)
    train_step(m, crit, opt, *args, micro_batch=micro_batch)       # builds the buffers
    m._flat_grad.fill_(float("nan"))
    m.patch_draw = draw
    ld = train_step(m, crit, opt, *args, micro_batch=micro_batch)
    torch.cuda.synchronize()
    assert m.patch_draw == draw + 1                                 # one draw per step, chunked or not
    g = m._flat_grad.detach().clone()
    assert bool(torch.isfinite(g).all())
    return {k: float(v) for k, v in ld.items()}, g


def test_micro_batched_step_drops_what_the_unchunked_step_drops(stream16):
    """B = 5 in chunks of 2: a ragged last chunk; the same draw in both runs."""
    from oracle import clip_oracle as O
    from clip_event_amd.losses import CriterionContrastive
    cfg = O.ClipConfig(*SMALL)
    img, txt, (yi, yt, ip) = _data(cfg, 5)
    args = (img.to(DEV), txt.to(DEV), yi.to(DEV), yt.to(DEV), ip.to(DEV))
    crit = CriterionContrastive("ce")
    out = []
    for mb in (2, None):
        m, _ = _mk(cfg, SEED)
        m.set_patch_dropout(0.5, seed=PSEED)
        out.append((m,) + _step_gradients(m, crit, args, mb, draw=DRAW))
    (m, ld, g), (_, ld_ref, g_ref) = out
    _compare_to_unchunked("patch dropout, micro_batch=2", m, g, g_ref, ld, ld_ref)


def test_two_fused_adam_steps(stream16):
    from oracle import clip_oracle as O
    from clip_event_amd.engine import train_step
    from clip_event_amd.losses import CriterionContrastive
    from clip_event_amd.optim import FusedAdam
    cfg = O.ClipConfig(*SMALL)
    img, txt, (yi, yt, ip) = _data(cfg, 4)
    m, _ = _mk(cfg, SEED)
    m.set_patch_dropout(0.5, seed=PSEED)
    before = {n: p.detach().clone() for n, p in m.named_parameters()}
    opt = FusedAdam(m, lr=1e-4, max_norm=1.0)
    crit = CriterionContrastive("ce")
    for _ in range(2):
        ld = train_step(m, crit, opt, img.to(DEV), txt.to(DEV), yi.to(DEV), yt.to(DEV), ip.to(DEV))
    torch.cuda.synchronize()
    assert all(np.isfinite(float(v)) for v in ld.values()) and m.patch_draw == 2
    for n in ("visual.conv1.weight", "visual.class_embedding", "visual.proj", "visual.transformer.resblocks.0.attn.in_proj_weight"):
        assert not torch.equal(dict(m.named_parameters())[n].detach(), before[n]), n
    assert m.stream16_saturation() == (0, 0)
