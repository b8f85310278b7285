"""GPU: the forward that keeps nothing for a backward.

* ``CE_EPI_BIAS_QGELU_BF16``: QuickGELU(acc + bias) alone, in every NT kernel family and on the fp8 path -- against fp32
  PyTorch with the bound the existing epilogue tests put on "gelu act" (3e-3 relative L2 after the bf16 store), and
  BIT-IDENTICAL to the activation ``CE_EPI_BIAS_GELU`` writes next to its derivative (same tile variant, same arithmetic).
* ``ce_tower_forward_infer`` against ``ce_tower_forward``: same launches over reused buffers, so the outputs are equal bit
  for bit -- dense and packed rows, pruned and full mode, both stream formats, bf16 and fp8 operands.
* through the model: features under ``torch.no_grad()`` equal the features with grad enabled, and do not allocate the
  activation stash."""
import ctypes

import numpy as np
import pytest
import torch

from tests.test_hip_ops import _q8_ref, _randn, _report

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(params=[False, True], ids=["stream32", "stream16"])
def stream16(request, monkeypatch):
    """Both residual-stream formats (fixture of tests/test_model_gpu.py)."""
    monkeypatch.setenv("CE_STREAM16", "1" if request.param else "0")
    return request.param


def _mk(cfg, seed):
    from oracle import clip_oracle as O
    from clip_event_amd.model import build_model
    sd = O.init_params(cfg, seed)
    m = build_model({k: v.clone() for k, v in sd.items()}).to(DEV)
    return m, sd


def _check_qgelu(tag, A, B, bias, acc):
    from clip_event_amd import ops, _lib as L
    dact, g = ops.gemm_nt(A, B, L.EPI_BIAS_GELU, bias=bias.to(DEV))
    act = ops.gemm_nt(A, B, L.EPI_BIAS_QGELU_BF16, bias=bias.to(DEV))
    torch.cuda.synchronize()
    h = acc + bias
    assert act.dtype == torch.bfloat16 and tuple(act.shape) == tuple(acc.shape)
    assert _report(f"{tag} qgelu act", act.float().cpu(), h * torch.sigmoid(1.702 * h))[1] < 3e-3
    differ = int((act.view(torch.int16) != g.view(torch.int16)).sum())
    print(f"[{tag}] elements that differ from BIAS_GELU's out2: {differ} of {act.numel()}")
    assert torch.equal(act, g)


@pytest.mark.parametrize("M,N,K", [(400, 512, 256), (1100, 768, 512), (2000, 520, 256), (12800, 768, 768), (3000, 2048, 512),
                                   (1300, 512, 192), (9000, 768, 256), (5000, 2304, 128), (20000, 3072, 64), (2000, 512, 64)])
def test_qgelu_epilogue_at_the_epilogue_test_shapes(M, N, K):
    """The shapes of tests/test_hip_ops.py::test_gemm_nt_epilogues (they reach every kernel family the policy picks)."""
    rng = np.random.default_rng(5 + M)
    a = _randn(rng, M, K).to(torch.bfloat16)
    b = _randn(rng, N, K, scale=K ** -0.5).to(torch.bfloat16)
    bias = _randn(rng, N)
    _check_qgelu(f"{M}x{N}x{K}", a.to(DEV), b.to(DEV), bias, a.float() @ b.float().t())


@pytest.mark.parametrize("variant", [5, 8, 32, 104, 160, 161, 162, 163, 164])
def test_qgelu_epilogue_in_every_forced_tile_variant(variant):
    """The variants of tests/test_hip_ops.py::test_gemm_nt_forced_tile_variants, same operands."""
    from clip_event_amd import _lib as L
    M, N, K = 2900, 1032, 192
    rng = np.random.default_rng(variant)
    a = _randn(rng, M, K).to(torch.bfloat16)
    b = _randn(rng, N, K, scale=K ** -0.5).to(torch.bfloat16)
    bias = _randn(rng, N)
    lib = L.lib()
    lib.ce_gemm_nt_tune(variant)
    try:
        _check_qgelu(f"v{variant}", a.to(DEV), b.to(DEV), bias, a.float() @ b.float().t())
    finally:
        lib.ce_gemm_nt_tune(0)


@pytest.mark.parametrize("M,N,K", [(400, 512, 256), (2000, 1024, 512), (18464, 4096, 1024)])
def test_qgelu_epilogue_on_the_fp8_path(M, N, K):
    """``ce_gemm_nt_fp8`` at the shape of test_gemm_nt_fp8_epilogues (gemm_nt8_kernel), at one that takes the single-round
    loader-wave kernel and at one that takes the persistent kernel with two tile heights."""
    from clip_event_amd import ops, _lib as L
    rng = np.random.default_rng(5)
    a = _randn(rng, M, K).to(torch.bfloat16)
    b = _randn(rng, N, K, scale=K ** -0.5).to(torch.bfloat16)
    qa, sa, fa = _q8_ref(a)
    qb, sb, fb = _q8_ref(b)
    acc = (fa @ fb.t()) * sa[:, None] * sb[None, :]
    bias = _randn(rng, N)
    A8, SA, B8, SB = qa.to(DEV), sa.to(DEV), qb.to(DEV), sb.to(DEV)
    dact, g = ops.gemm_nt_fp8(A8, SA, B8, SB, L.EPI_BIAS_GELU, bias=bias.to(DEV))
    act = ops.gemm_nt_fp8(A8, SA, B8, SB, L.EPI_BIAS_QGELU_BF16, bias=bias.to(DEV))
    torch.cuda.synchronize()
    h = acc + bias
    assert _report(f"fp8 {M}x{N}x{K} qgelu act", act.float().cpu(), h * torch.sigmoid(1.702 * h))[1] < 3e-3
    assert torch.equal(act, g)


# ---------------------------------------------------------------------------------------------------------------
# the tower runner


def _run_tower(m, desc, infer, batch, rows, cu, x0, sel, n_out):
    from clip_event_amd._lib import check, lib, ptr, stream
    cl = lib()
    size_fn = cl.ce_tower_infer_workspace_bytes if infer else cl.ce_tower_workspace_bytes
    size_fn.restype = ctypes.c_size_t
    nbytes = int(size_fn(ctypes.byref(desc), ctypes.c_int(batch)))
    assert nbytes > 0
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=DEV)      # whatever a reused buffer holds must not matter
    out = torch.empty((n_out, desc.width), dtype=x0.dtype, device=DEV)
    fn = cl.ce_tower_forward_infer if infer else cl.ce_tower_forward
    keep = x0.clone()
    check(fn(ctypes.byref(desc), ctypes.c_int(batch), ctypes.c_int(rows), ptr(cu), ptr(x0), ptr(ws), ptr(out), ptr(sel), stream()),
          fn.__name__)
    torch.cuda.synchronize()
    assert torch.equal(x0, keep), "x0 was overwritten"
    return out, nbytes


TOWER_CASES = {
    # name: (config, batch)       config = (embed, resolution, v_layers, v_width, patch, context, vocab, t_width, t_heads, t_layers)
    "tiny": ((64, 64, 2, 128, 32, 20, 512, 128, 2, 2), 4),
    "patch14_197": ((64, 196, 2, 128, 14, 20, 512, 128, 2, 2), 3),
    "text_packed": ((64, 64, 2, 128, 32, 77, 512, 128, 2, 3), 24),
}


@pytest.mark.parametrize("fp8", [0, 1])
@pytest.mark.parametrize("pruned", [True, False], ids=["pruned", "full"])
@pytest.mark.parametrize("case", sorted(TOWER_CASES))
def test_tower_forward_infer_equals_tower_forward(case, pruned, fp8, stream16):
    from oracle import clip_oracle as O
    from clip_event_amd import functional as F, synthetic as S
    cfg_t, B = TOWER_CASES[case]
    cfg = O.ClipConfig(*cfg_t)
    m, _ = _mk(cfg, 5)
    m.fp8 = fp8
    m._ready()
    assert bool(m.stream16) == stream16
    sdt = torch.float16 if stream16 else torch.float32
    rng = np.random.default_rng(17)
    if case == "text_packed":
        txt = S.synthetic_tokens(B, cfg.context_length, cfg.vocab_size, seed=11, min_len=1).to(DEV)
        pk = F.text_packing(m, txt)
        assert pk.cu is not None and pk.rows < B * cfg.context_length
        desc, rows, cu, sel = m._tdesc, pk.rows, pk.cu, pk.sel
    else:
        T = cfg.vision_tokens
        desc, rows, cu = m._vdesc, B * T, None
        sel = torch.arange(B, device=DEV, dtype=torch.int32) * T
    x0 = _randn(rng, rows, desc.width).to(DEV).to(sdt)
    if not pruned:
        sel = None
    n_out = B if pruned else rows
    ref, stash_bytes = _run_tower(m, desc, False, B, rows, cu, x0, sel, n_out)
    got, infer_bytes = _run_tower(m, desc, True, B, rows, cu, x0, sel, n_out)
    print(f"[{case} pruned={pruned} fp8={fp8} stream16={stream16}] workspace {infer_bytes} B against {stash_bytes} B; "
          f"max |d| {float((got.float() - ref.float()).abs().max()):.3e}")
    assert bool(torch.isfinite(ref.float()).all())
    assert torch.equal(got, ref)
    assert infer_bytes < stash_bytes


@pytest.mark.parametrize("fp8", [0, 1])
def test_features_without_grad_equal_features_with_grad(fp8, stream16):
    from oracle import clip_oracle as O
    from clip_event_amd import functional as F, synthetic as S
    cfg = O.ClipConfig(64, 64, 3, 128, 32, 20, 512, 128, 2, 2)
    m, _ = _mk(cfg, 7)
    m.fp8 = fp8
    img = S.synthetic_images(5, cfg.image_resolution, seed=3).to(DEV)
    txt = S.synthetic_tokens(15, cfg.context_length, cfg.vocab_size, seed=4, min_len=2).to(DEV)
    calls = []
    inner = F._tower_forward_infer

    def spy(model, desc, tag, *a):
        calls.append(tag)
        return inner(model, desc, tag, *a)

    F._tower_forward_infer = spy
    try:
        fi_g, ft_g, grid_g = m.encode_image(img), m.encode_text(txt), m.encode_image(img, use_grid=True)
        assert calls == [] and fi_g.requires_grad and ft_g.requires_grad
        both_g = m.encode_both(img, txt)
        with torch.no_grad():
            fi, ft, grid = m.encode_image(img), m.encode_text(txt), m.encode_image(img, use_grid=True)
            assert calls == ["vision", "text", "vision"]
            both = m.encode_both(img, txt)
            li, lt = m(img, txt)
        assert sorted(calls[3:]) == ["text", "text", "vision", "vision"]
    finally:
        F._tower_forward_infer = inner
    torch.cuda.synchronize()
    assert not fi.requires_grad and fi.grad_fn is None and not ft.requires_grad
    assert torch.equal(fi, fi_g.detach()) and torch.equal(ft, ft_g.detach()) and torch.equal(grid, grid_g.detach())
    assert torch.equal(both[0], both_g[0].detach()) and torch.equal(both[1], both_g[1].detach())
    assert torch.equal(both[0], fi) and torch.equal(both[1], ft)
    li_g, lt_g = m(img, txt)
    assert torch.equal(li, li_g.detach()) and torch.equal(lt, lt_g.detach())
    # and the pass with grad still differentiates: nothing of the forward-only path leaks into it
    (fi_g.sum() + ft_g.sum()).backward()
    torch.cuda.synchronize()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in m.parameters())


def test_zero_shot_runs_on_the_forward_only_tower():
    from oracle import clip_oracle as O
    from clip_event_amd import functional as F, synthetic as S
    from clip_event_amd.inference import zero_shot
    cfg = O.ClipConfig(64, 64, 2, 128, 32, 20, 512, 128, 2, 2)
    m, _ = _mk(cfg, 9)
    img = S.synthetic_images(3, cfg.image_resolution, seed=4)
    txt = S.synthetic_tokens(7, cfg.context_length, cfg.vocab_size, seed=5, min_len=2)
    calls = []
    inner = F._tower_forward_infer
    F._tower_forward_infer = lambda model, desc, tag, *a: (calls.append(tag), inner(model, desc, tag, *a))[1]
    try:
        scores, idx, probs = zero_shot(m, img.to(DEV), txt.to(DEV))
    finally:
        F._tower_forward_infer = inner
    assert sorted(calls) == ["text", "vision"] and tuple(probs.shape) == (3, 7)
    assert not any(k[0].endswith(("vision", "text")) for k in m._pool.free), "a training-sized stash was leased"


def test_no_grad_forward_does_not_allocate_the_stash(stream16):
    """12 blocks: across a ``no_grad`` encode_image the peak of allocated device memory rises by less than the tower's
    training workspace -- less than the stash alone, which a forward that always stashes has to allocate."""
    from oracle import clip_oracle as O
    from clip_event_amd import synthetic as S
    from clip_event_amd._lib import lib
    cfg = O.ClipConfig(64, 224, 12, 256, 32, 20, 512, 128, 2, 2)
    m, _ = _mk(cfg, 3)
    B = 32
    img = S.synthetic_images(B, cfg.image_resolution, seed=1).to(DEV)
    m._ready()                                   # flat buffers, operand copies: everything that is not per-forward
    lib().ce_tower_workspace_bytes.restype = ctypes.c_size_t
    stash = int(lib().ce_tower_workspace_bytes(ctypes.byref(m._vdesc), ctypes.c_int(B)))
    lib().ce_tower_infer_workspace_bytes.restype = ctypes.c_size_t
    infer = int(lib().ce_tower_infer_workspace_bytes(ctypes.byref(m._vdesc), ctypes.c_int(B)))
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    with torch.no_grad():
        f = m.encode_image(img)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    print(f"[no_grad encode_image, 12 blocks, B={B}, stream16={stream16}] peak rise {rise / 2**20:.1f} MiB; forward-only workspace "
          f"{infer / 2**20:.1f} MiB; training workspace {stash / 2**20:.1f} MiB")
    assert bool(torch.isfinite(f).all())
    assert rise < stash
