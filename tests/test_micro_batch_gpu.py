"""GPU: ``engine.train_step(..., micro_batch=n)`` -- features of every chunk without a stash, the head once over the whole
batch, then a second forward + backward per chunk with the feature gradients injected -- against the fp32 oracle with the
bounds the unchunked step has to meet, and against the unchunked step of the same build.

A chunk and the whole batch tile differently, so chunked and unchunked results differ where bf16 roundings flip with the
summation order: the situation of a rank's shard against the concatenated batch, with the bounds tests/ddp_child.py puts
on it (losses 3e-3 * max(1, |loss|), worst per-parameter gradient rel-L2 2e-3).  A dropped, doubled or misrouted chunk is
an error of order 1 / chunks.

The chunked-against-unchunked figure (worst per-parameter rel-L2, printed per stream format) had not been measured on a
GPU when these tests were written: DESIGN.md 4a lists it among the measurements still to take."""
import ctypes
import gc

import numpy as np
import pytest
import torch

from tests.test_ddp_gpu import run_ranks

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(params=[False, True], ids=["stream32", "stream16"])
def stream16(request, monkeypatch):
    """Both residual-stream formats (fixture of tests/test_model_gpu.py): same tolerances for both."""
    monkeypatch.setenv("CE_STREAM16", "1" if request.param else "0")
    return request.param


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


def _step_gradients(m, crit, img, txt, yi, yt, ip, micro_batch):
    """One ``train_step`` with FusedAdam(lr=0) -- the gradients stay in the buffer -- over a NaN-poisoned gradient buffer."""
    from clip_event_amd.engine import train_step
    from clip_event_amd.optim import FusedAdam
    opt = FusedAdam(m, lr=0.0, max_norm=1.0)
    train_step(m, crit, opt, img, txt, yi, yt, ip, micro_batch=micro_batch)      # builds the buffers
    m._flat_grad.fill_(float("nan"))
    ld = train_step(m, crit, opt, img, txt, yi, yt, ip, micro_batch=micro_batch)
    torch.cuda.synchronize()
    assert m._first_touch == set()
    g = m._flat_grad.detach().clone()
    assert bool(torch.isfinite(g).all()), "an element of the gradient buffer was neither zeroed nor overwritten"
    return {k: float(v) for k, v in ld.items()}, g


def _compare_to_unchunked(tag, m, g, g_ref, ld, ld_ref):
    """Losses within 3e-3 * max(1, |loss|); per parameter with a non-zero unchunked gradient rel-L2 <= 2e-3, exactly zero
    where the unchunked gradient is zero."""
    assert sorted(ld) == sorted(ld_ref)
    for k in ld_ref:
        print(f"[{tag}] {k}: chunked {ld[k]:.6f}, unchunked {ld_ref[k]:.6f}")
    worst = (0.0, None)
    zero_bad = []
    for n, p in m.named_parameters():
        o = m._offsets[n]
        a, b = g[o:o + p.numel()], g_ref[o:o + p.numel()]
        if float(b.norm()) == 0.0:
            if float(a.abs().max()) != 0.0:
                zero_bad.append(n)
            continue
        r = _rel(a, b)
        if r > worst[0]:
            worst = (r, n)
    print(f"[{tag}] chunked against unchunked: worst per-parameter gradient rel-L2 {worst[0]:.3e} at {worst[1]}; "
          f"flat buffer rel-L2 {_rel(g, g_ref):.3e}")
    for k in ld_ref:
        assert abs(ld[k] - ld_ref[k]) <= 3e-3 * max(1.0, abs(ld_ref[k])), (k, ld[k], ld_ref[k])
    assert not zero_bad, zero_bad
    assert worst[0] <= 2e-3, worst


_TINY_ORACLE = {}


@pytest.mark.parametrize("micro_batch", [2, 3, 1])
def test_tiny_chunked_step_against_oracle_and_unchunked(micro_batch, stream16):
    """The tiny golden configuration (4 images, 3 captions each) in chunks of 2, 3 (ragged last chunk) and 1."""
    from oracle import clip_oracle as O
    from clip_event_amd import synthetic as S
    from clip_event_amd.losses import CriterionContrastive
    from tests.util import golden_json
    G = golden_json()["tiny"]
    cfg = O.ClipConfig(**G["cfg"])
    B, K = G["B"], G["K"]
    img = S.synthetic_images(B, cfg.image_resolution, seed=G["img_seed"])
    txt = S.synthetic_tokens(B * K, cfg.context_length, cfg.vocab_size, seed=G["txt_seed"], min_len=G["txt_min_len"])
    yi, yt, ip = O.build_labels(B, 1, K - 1, True)
    m, sd = _mk(cfg, G["param_seed"])
    m_ref, _ = _mk(cfg, G["param_seed"])
    crit = CriterionContrastive("ce")
    dev_args = (img.to(DEV), txt.to(DEV), yi.to(DEV), yt.to(DEV), ip.to(DEV))
    ld, g = _step_gradients(m, crit, *dev_args, micro_batch)
    ld_ref, g_ref = _step_gradients(m_ref, crit, *dev_args, None)
    if "g" not in _TINY_ORACLE:
        _TINY_ORACLE["g"] = O.loss_and_grads(sd, cfg, img, txt, yi, yt, ip, True)[:2]
    ld32, g32 = _TINY_ORACLE["g"]
    tag = f"tiny micro_batch={micro_batch} stream16={stream16}"
    # against the fp32 oracle: what test_tiny_against_oracle asks of the unchunked step
    worst, rels = (1.0, None), []
    for n, p in m.named_parameters():
        ref = g32[n]
        if ref is None or float(ref.norm()) == 0.0:
            continue
        o = m._offsets[n]
        got = g[o:o + p.numel()].view_as(p)
        c = _cos(got, ref)
        rels.append(_rel(got, ref))
        if c < worst[0]:
            worst = (c, n)
    print(f"[{tag}] against the fp32 oracle: worst gradient cosine {worst[0]:.5f} at {worst[1]}; median rel-L2 {np.median(rels):.4f}; "
          f"loss_i {ld['loss_i']:.5f} (oracle {float(ld32['loss_i']):.5f}) loss_t {ld['loss_t']:.5f} (oracle {float(ld32['loss_t']):.5f})")
    assert worst[0] > 0.98 and np.median(rels) < 0.03
    assert abs(ld["loss_i"] - float(ld32["loss_i"])) < 2e-2 and abs(ld["loss_t"] - float(ld32["loss_t"])) < 2e-2
    _compare_to_unchunked(tag, m, g, g_ref, ld, ld_ref)


_NOISE_FLOOR_ORACLE = {}


def test_vitb32_b8_chunked_gradient_error_is_at_the_bf16_noise_floor(stream16):
    """BASELINE config 1's shapes (ViT-B/32, 8 images, the golden tokens) in chunks of 2: per parameter the relative L2
    error against the fp32 oracle stays within 2 x the oracle's own bf16 restatement + 0.02, cosine > 0.98 -- the bound of
    test_vitb32_b8_gradient_error_is_at_the_bf16_noise_floor -- and the chunked step meets the chunked-against-unchunked
    bounds here too."""
    from oracle import clip_oracle as O
    from clip_event_amd import synthetic as S
    from clip_event_amd.losses import CriterionContrastive
    from tests.util import golden_json, golden_npz
    G = golden_json()["vitb32"]
    Z = golden_npz("vitb32_b8.npz")
    m, sd = _mk(O.VIT_B32, G["param_seed"])
    m_ref, _ = _mk(O.VIT_B32, G["param_seed"])
    img = S.synthetic_images(8, 224, seed=G["img_seed"])
    txt = torch.from_numpy(Z["tokens"])
    y = torch.arange(8, device=DEV)
    crit = CriterionContrastive("ce")
    ld, g = _step_gradients(m, crit, img.to(DEV), txt.to(DEV), y, y, y, 2)
    ld_ref, g_ref = _step_gradients(m_ref, crit, img.to(DEV), txt.to(DEV), y, y, y, None)
    yc = torch.arange(8)
    if "g" not in _NOISE_FLOOR_ORACLE:         # the oracle's two runs are the same for both stream formats
        _NOISE_FLOOR_ORACLE["g"] = (O.loss_and_grads(sd, O.VIT_B32, img, txt, yc, yc, yc)[1],
                                    O.loss_and_grads(sd, O.VIT_B32, img, txt, yc, yc, yc, bf16=True)[1])
    g32, g16 = _NOISE_FLOOR_ORACLE["g"]
    rows = []
    for n, p_ in m.named_parameters():
        ref = g32[n]
        if ref is None or float(ref.norm()) == 0.0:
            continue
        o = m._offsets[n]
        got = g[o:o + p_.numel()].view_as(p_)
        rows.append((n, _rel(got, ref), _rel(g16[n], ref), _cos(got, ref)))
    rows.sort(key=lambda r: -r[1])
    for n, e_hip, e_16, c in rows[:6]:
        print(f"{n:48s} rel-L2 vs fp32: chunked HIP {e_hip:.4f}, bf16 oracle {e_16:.4f}; cosine {c:.5f}")
    print(f"[noise floor, micro_batch=2, stream16={stream16}] largest margin use {max(r[1] / (2.0 * r[2] + 0.02) for r in rows):.3f} of the bound")
    for n, e_hip, e_16, c in rows:
        assert e_hip < 2.0 * e_16 + 0.02, (n, e_hip, e_16)
        assert c > 0.98, (n, c)
    _compare_to_unchunked(f"ViT-B/32 B=8 micro_batch=2 stream16={stream16}", m, g, g_ref, ld, ld_ref)


def test_chunked_train_step_fused_adam_against_golden(stream16):
    """Two ``train_step``s with ``micro_batch`` and a real learning rate against golden.json["tiny_step"], exactly as
    test_train_step_fused_adam checks the unchunked update."""
    from oracle import clip_oracle as O
    from clip_event_amd import synthetic as S
    from clip_event_amd.engine import train_step
    from clip_event_amd.losses import CriterionContrastive
    from clip_event_amd.optim import FusedAdam
    from tests.util import golden_json
    G = golden_json()
    cfg = O.ClipConfig(**G["tiny"]["cfg"])
    m, sd = _mk(cfg, 11)
    img = S.synthetic_images(4, cfg.image_resolution, seed=31)
    txt = S.synthetic_tokens(4, cfg.context_length, cfg.vocab_size, seed=32, min_len=2)
    yi, yt, ip = O.build_labels(4, 1, 0, True)
    opt = FusedAdam(m, lr=G["tiny_step"]["lr"], weight_decay=G["tiny_step"]["weight_decay"], max_norm=1.0)
    crit = CriterionContrastive("ce")
    p_ref, state = sd, {}
    for step in G["tiny_step"]["steps"]:
        ld = train_step(m, crit, opt, img.to(DEV), txt.to(DEV), yi.to(DEV), yt.to(DEV), ip.to(DEV), micro_batch=2)
        torch.cuda.synchronize()
        p_ref, ld_ref, gn_ref = O.train_step(p_ref, cfg, state, img, txt, yi, yt, ip, lr=G["tiny_step"]["lr"],
                                             weight_decay=G["tiny_step"]["weight_decay"])
        print(f"step loss_i {float(ld['loss_i']):.5f} (ref {step['loss_i']:.5f}) grad_norm {float(opt.grad_norm()):.4f} (ref {step['grad_norm']:.4f})")
        assert abs(float(ld["loss_i"]) - step["loss_i"]) < 3e-2
        assert abs(float(opt.grad_norm()) - step["grad_norm"]) < 0.05 * step["grad_norm"]
    worst = 1.0
    for n, p in m.named_parameters():
        d_hip = p.detach().cpu() - sd[n]
        d_ref = p_ref[n] - sd[n]
        if float(d_ref.norm()) > 0:
            worst = min(worst, _cos(d_hip, d_ref))
    print("worst parameter-delta cosine after 2 chunked Adam steps:", worst)
    assert worst > 0.98


def test_micro_batch_that_does_not_chunk_takes_the_unchunked_path(stream16):
    """``None`` and a value >= the number of images: today's step (the forward-only tower must not run); with ``train_arg``
    or ``criterion_ot`` a chunking value is refused."""
    from oracle import clip_oracle as O
    from clip_event_amd import functional as F, synthetic as S
    from clip_event_amd.engine import train_step
    from clip_event_amd.losses import CriterionAlignment, CriterionContrastive
    from clip_event_amd.optim import FusedAdam
    cfg = O.ClipConfig(64, 64, 2, 128, 32, 20, 512, 128, 2, 2)
    m, _ = _mk(cfg, 4)
    B, K = 4, 2
    img = S.synthetic_images(B, cfg.image_resolution, seed=1).to(DEV)
    txt = S.synthetic_tokens(B * K, cfg.context_length, cfg.vocab_size, seed=2, min_len=2).to(DEV)
    yi, yt, ip = (t.to(DEV) for t in O.build_labels(B, 1, K - 1, True))
    crit = CriterionContrastive("ce")
    opt = FusedAdam(m, lr=0.0, max_norm=1.0)
    inner = F._tower_forward_infer

    def refuse(*a, **k):
        raise AssertionError("the forward-only tower ran in a step that does not chunk")

    F._tower_forward_infer = refuse
    try:
        grads = []
        for mb in (None, B, B + 3):
            train_step(m, crit, opt, img, txt, yi, yt, ip, micro_batch=mb)
            torch.cuda.synchronize()
            grads.append(m._flat_grad.detach().clone())
        assert _rel(grads[1], grads[0]) < 1e-5 and _rel(grads[2], grads[0]) < 1e-5       # (fp32 atomics: order of the adds)
        with pytest.raises(AssertionError, match="forward-only tower ran"):
            train_step(m, crit, opt, img, txt, yi, yt, ip, micro_batch=2)
    finally:
        F._tower_forward_infer = inner
    m._lease_batch = None
    with pytest.raises(NotImplementedError, match="micro_batch"):
        train_step(m, crit, opt, img, txt, yi, yt, ip, micro_batch=2, train_arg="desc", bboxs=[], bbox_desc_vec=[], bbox_label_vec=[])
    with pytest.raises(NotImplementedError, match="micro_batch"):
        train_step(m, crit, opt, img, txt, yi, yt, ip, micro_batch=2, criterion_ot=CriterionAlignment())
    with pytest.raises(ValueError, match="micro_batch"):
        train_step(m, crit, opt, img, txt, yi, yt, ip, micro_batch=0)
    with pytest.raises(RuntimeError, match="captions per image"):
        train_step(m, crit, opt, img, txt[:7], yi, yt[:7], ip, micro_batch=2)
    # tokens on the device WITHOUT host lengths are read back once for the batch; the chunk views then carry their lengths
    ld = train_step(m, crit, opt, img, txt.clone(), yi, yt, ip, micro_batch=3)
    torch.cuda.synchronize()
    assert all(np.isfinite(float(v)) for v in ld.values())


def test_chunked_step_keeps_one_chunk_of_stash(stream16):
    """12 blocks, 32 images: with ``micro_batch=8`` a quarter of the image tower's stash lives at a time, so the peak of
    allocated memory during the step is below the unchunked step's by more than HALF of the 32-image workspace."""
    from oracle import clip_oracle as O
    from clip_event_amd import synthetic as S
    from clip_event_amd._lib import lib
    from clip_event_amd.engine import train_step
    from clip_event_amd.losses import CriterionContrastive
    from clip_event_amd.optim import FusedAdam
    cfg = O.ClipConfig(64, 224, 12, 256, 32, 20, 512, 128, 2, 2)
    B = 32
    img = S.synthetic_images(B, cfg.image_resolution, seed=1).to(DEV)
    txt = S.synthetic_tokens(B, cfg.context_length, cfg.vocab_size, seed=2, min_len=2).to(DEV)
    yi, yt, ip = (t.to(DEV) for t in O.build_labels(B, 1, 0, True))
    crit = CriterionContrastive("ce")
    lib().ce_tower_workspace_bytes.restype = ctypes.c_size_t
    peaks, stash = {}, None
    for mb in (None, 8):
        m, _ = _mk(cfg, 3)                       # a fresh model: the workspace pool keeps its buffers
        opt = FusedAdam(m, lr=0.0, max_norm=1.0)
        m._ready()
        stash = int(lib().ce_tower_workspace_bytes(ctypes.byref(m._vdesc), ctypes.c_int(B)))
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        ld = train_step(m, crit, opt, img, txt, yi, yt, ip, micro_batch=mb)
        torch.cuda.synchronize()
        peaks[mb] = torch.cuda.max_memory_allocated() - base
        assert all(np.isfinite(float(v)) for v in ld.values())
        del m, opt, ld
        gc.collect()
        torch.cuda.empty_cache()
    print(f"[stash memory, 12 blocks, B={B}, stream16={stream16}] peak rise during the step: unchunked {peaks[None] / 2**20:.1f} MiB, "
          f"micro_batch=8 {peaks[8] / 2**20:.1f} MiB; image-tower workspace at B=32 {stash / 2**20:.1f} MiB")
    assert peaks[8] < peaks[None] - stash / 2


@pytest.mark.timeout(900)
@pytest.mark.parametrize("case", ["allreduce", "sharded"])
def test_two_rank_chunked_step_equals_the_two_rank_unchunked_step(case):
    """Two ranks on one GPU over gloo (tests/micro_batch_child.py): the global-batch step with ``micro_batch`` = half the
    per-rank batch against the SAME two ranks' unchunked step on the same shards -- every rank holds the same averaged
    gradient, losses within 3e-3, worst per-parameter rel-L2 2e-3 -- and one buffer length per step through
    ``GradSync._reduce_range``."""
    rcs, outs = run_ranks("micro_batch_child.py", case)
    print(outs[0][-3000:])
    assert rcs == [0, 0], "\n".join(o[-3000:] for o in outs)
    assert f"[{case}] OK" in outs[0]
