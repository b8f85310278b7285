"""CPU: the host side of running the image tower at another resolution -- the weight tables against torch's own
antialiased bicubic ``interpolate`` in fp64 (forward and autograd backward), the permanent resize of a state dict, and
``CLIP.set_image_size``'s validation and bookkeeping on a model that never sees a GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import image_size_ref as R

TINY = (128, 96, 2, 128, 16, 20, 512, 128, 2, 2)              # native grid 6, patch 16


def _interp(x, n_out):
    return F.interpolate(x, size=(n_out, n_out), mode="bicubic", antialias=True, align_corners=False)


@pytest.mark.parametrize("n_in,n_out", R.PAIRS)
def test_weights_equal_torch_interpolate_in_fp64(n_in, n_out):
    """Unit-normal data, max abs difference <= 1e-12 forward and backward (4.4e-15 measured; the margin covers another libm)."""
    from clip_event_amd.posembed import weights
    w = weights(n_in, n_out)
    assert w.dtype == np.float64 and w.shape == (n_out, n_in)
    assert np.abs(w - R.weights(n_in, n_out)).max() <= 1e-15          # the restatement of tests/image_size_ref.py
    g = torch.Generator().manual_seed(n_in * 100 + n_out)
    x = torch.randn(2, 3, n_in, n_in, dtype=torch.float64, generator=g, requires_grad=True)
    y = _interp(x, n_out)
    dy = torch.randn(y.shape, dtype=torch.float64, generator=g)
    y.backward(dy)
    fwd = np.einsum("ia,jb,ncab->ncij", w, w, x.detach().numpy())
    bwd = np.einsum("ia,jb,ncij->ncab", w, w, dy.numpy())
    e_f, e_b = np.abs(fwd - y.detach().numpy()).max(), np.abs(bwd - x.grad.numpy()).max()
    print(f"{n_in} -> {n_out}: forward {e_f:.2e}, backward {e_b:.2e}")
    assert e_f <= 1e-12 and e_b <= 1e-12


@pytest.mark.parametrize("n_in,n_out", R.PAIRS + [(1, 3), (3, 1), (63, 2), (2, 63)])
def test_rows_sum_to_one(n_in, n_out):
    """Each row is divided by its sum: the sum of the quotients is 1 within one rounding per tap."""
    from clip_event_amd.posembed import weights
    w = weights(n_in, n_out)
    taps = (w != 0).sum(axis=1).max()
    assert np.abs(w.sum(axis=1) - 1.0).max() <= taps * 2.0 ** -53


@pytest.mark.parametrize("n", [1, 2, 6, 7, 14, 24, 63])
def test_equal_grids_give_the_identity_exactly(n):
    from clip_event_amd.posembed import weights
    assert np.array_equal(weights(n, n), np.eye(n))


def _tiny_sd(seed=3):
    from oracle import clip_oracle as O
    return O.init_params(O.ClipConfig(*TINY), seed)


@pytest.mark.parametrize("size", [160, 64, 192])
def test_resize_visual_state_dict(size):
    from clip_event_amd.model import build_model
    from clip_event_amd.posembed import resize_visual_state_dict
    sd = _tiny_sd()
    out = resize_visual_state_dict(sd, size)
    g = size // 16
    pos, new = sd["visual.positional_embedding"], out["visual.positional_embedding"]
    assert new.shape == (g * g + 1, 128) and new.dtype == torch.float32
    assert set(out) == set(sd) and all(out[k] is sd[k] for k in sd if k != "visual.positional_embedding")
    assert sd["visual.positional_embedding"].shape == (37, 128)                       # the input is not modified
    # the class row is copied, not interpolated; the grid rows are F.interpolate's in fp32: both sides round a sum of at most 64
    # products of magnitude <= max|pos| with weights whose absolute row sums stay below 2 per axis
    assert torch.equal(new[0], pos[0])
    ref = _interp(pos[1:].reshape(1, 6, 6, 128).permute(0, 3, 1, 2), g).permute(0, 2, 3, 1).reshape(g * g, 128)
    err = float((new[1:] - ref).abs().max())
    bound = 66 * 2.0 ** -24 * 4 * float(pos.abs().max())
    print(f"{size} px: max |resized - F.interpolate| {err:.2e} (bound {bound:.2e})")
    assert err <= bound
    loud = dict(sd)                                   # a class row of 1e6 leaves every grid row as it was
    loud["visual.positional_embedding"] = torch.cat([torch.full((1, 128), 1e6), pos[1:]])
    assert torch.equal(resize_visual_state_dict(loud, size)["visual.positional_embedding"][1:], new[1:])
    # the result loads through build_model as a model that is native at the new size
    m = build_model({k: v.clone() for k, v in out.items()})
    v = m.visual
    assert (v.input_resolution, v.patch_num, v.native_resolution, v.native_patch_num) == (size, g, size, g)
    assert torch.equal(v.positional_embedding.detach(), new)


def test_resize_at_the_native_size_returns_the_same_table():
    from clip_event_amd.posembed import resize_visual_state_dict
    sd = _tiny_sd()
    out = resize_visual_state_dict(sd, 96)
    assert out is not sd and all(out[k] is sd[k] for k in sd)


def test_resize_refuses_a_bad_size():
    from clip_event_amd.posembed import resize_visual_state_dict
    with pytest.raises(ValueError, match="multiple of the patch size"):
        resize_visual_state_dict(_tiny_sd(), 100)


def test_set_image_size_validation_and_reporting():
    from clip_event_amd.model import build_model
    m = build_model(_tiny_sd())
    v = m.visual
    assert (v.input_resolution, v.patch_num, v.native_resolution, v.native_patch_num) == (96, 6, 96, 6)
    assert m.set_image_size(160) == 160
    assert (v.input_resolution, v.patch_num, v.native_resolution, v.native_patch_num) == (160, 10, 96, 6)
    assert v.positional_embedding.shape == (37, 128)
    assert v.patch_keep(0.5) == 50                                    # patch dropout counts the run grid's patches
    for bad in (100, 0, -16, 8):
        with pytest.raises(ValueError, match="multiple of the patch size"):
            m.set_image_size(bad)
    assert v.input_resolution == 160                                  # a refused size changes nothing
    assert m.set_image_size(63 * 16) == 1008                          # 3970 tokens
    with pytest.raises(ValueError, match="at most 4096"):
        m.set_image_size(64 * 16)                                     # 4097 tokens
    m.train()
    m.eval()
    assert v.input_resolution == 1008
    m.load_state_dict(_tiny_sd(seed=4))
    assert (v.input_resolution, v.patch_num) == (1008, 63)
    assert "visual.positional_embedding" in m.state_dict() and m.state_dict()["visual.positional_embedding"].shape == (37, 128)
    assert not any("size" in k or "resolution" in k for k in m.state_dict())
    assert m.set_image_size(None) == 96
    assert (v.input_resolution, v.patch_num) == (96, 6)
    assert m.set_image_size(96) == 96 and v.patch_num == 6


def test_no_library_call_on_a_cpu_model():
    """``set_image_size`` is bookkeeping only: the table is built by ``refresh_operands`` on the device."""
    from clip_event_amd import posembed
    from clip_event_amd.model import build_model
    calls = []
    orig = posembed.lib
    posembed.lib = lambda: calls.append(1) or orig()
    try:
        m = build_model(_tiny_sd())
        m.set_image_size(160)
        m.set_image_size(None)
    finally:
        posembed.lib = orig
    assert calls == []
