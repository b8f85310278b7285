"""The image tower's positional table on another patch grid.

``weights`` is the operator itself: the separable bicubic (``a = -0.5``), antialiased, ``align_corners=False`` resampling of
``torch.nn.functional.interpolate`` -- what open_clip's ``resize_pos_embed`` and timm's ``resample_abs_pos_embed`` apply --
as one dense matrix per axis, host arithmetic in fp64.  ``resample`` / ``resample_backward`` apply it (and its transpose) on
the device with the fp32 roundings of those matrices (``ce_pos_resample_fwd`` / ``ce_pos_resample_bwd``);
``resize_visual_state_dict`` applies the fp64 matrices on the host, once, to a state dict.
"""
from __future__ import annotations

import numpy as np
import torch

from ._lib import check, lib, ptr, stream

MAX_TOKENS = 4096        # the attention launchers' limit
MAX_GRID = 63            # the largest grid under it (63^2 + 1 = 3970), and the kernels' own argument check


def _cubic(x: np.ndarray) -> np.ndarray:
    """The cubic convolution kernel with ``a = -0.5`` (Keys), zero from 2 on."""
    a = -0.5
    x = np.abs(x)
    near = ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0
    far = (((x - 5.0) * x + 8.0) * x - 4.0) * a
    return np.where(x < 1.0, near, np.where(x < 2.0, far, 0.0))


def weights(n_in: int, n_out: int) -> np.ndarray:
    """fp64 [n_out, n_in]: row ``i`` holds the weights output cell ``i`` gives the ``n_in`` input cells of one axis.  When
    downsampling the support is stretched by the scale (the antialiasing); taps are clipped at the border and each row is
    divided by its sum.  ``n_in == n_out`` is the identity, exactly."""
    n_in, n_out = int(n_in), int(n_out)
    if n_in < 1 or n_out < 1:
        raise ValueError(f"grid sizes must be positive (got {n_in} -> {n_out})")
    scale = n_in / n_out
    support = 2.0 * scale if scale >= 1.0 else 2.0
    inv = 1.0 / scale if scale >= 1.0 else 1.0
    w = np.zeros((n_out, n_in), dtype=np.float64)
    for i in range(n_out):
        c = scale * (i + 0.5)
        lo = max(0, int(c - support + 0.5))
        hi = min(n_in, int(c + support + 0.5))
        j = np.arange(lo, hi, dtype=np.float64)
        row = _cubic((j - c + 0.5) * inv)
        w[i, lo:hi] = row / row.sum()
    return w


def check_image_size(size: int, patch: int) -> int:
    """The patch grid of a square ``size`` x ``size`` input; ValueError names the rule a bad size breaks."""
    size, patch = int(size), int(patch)
    if size <= 0 or size % patch:
        raise ValueError(f"the image size must be a positive multiple of the patch size {patch} (got {size})")
    g = size // patch
    if g * g + 1 > MAX_TOKENS:
        raise ValueError(f"an image of {size} px is {g * g + 1} tokens at patch size {patch}: at most {MAX_TOKENS} "
                         f"((size / patch)^2 + 1 <= {MAX_TOKENS})")
    return g


def grid_of(rows: int) -> int:
    """Grid side of a positional table with ``rows`` = g^2 + 1 rows."""
    g = int(round((rows - 1) ** 0.5))
    if g < 1 or g * g + 1 != rows:
        raise ValueError(f"a positional table has g*g + 1 rows (got {rows})")
    return g


_TABLES = {}


def device_tables(g_in: int, g_out: int, device):
    """``(wy, wx)``: the fp32 roundings of ``weights(g_in, g_out)`` on ``device``, cached per (grids, device).  The grids are
    square, so both axes share one table."""
    key = (int(g_in), int(g_out), str(device))
    t = _TABLES.get(key)
    if t is None:
        w = torch.from_numpy(weights(g_in, g_out).astype(np.float32)).to(device)
        t = _TABLES[key] = (w, w)
    return t


def _table(t: torch.Tensor, what: str, like: torch.Tensor = None, grid: int = None) -> torch.Tensor:
    """``t`` as the kernels need it: contiguous fp32 [g^2 + 1, D] on a GPU -- and, for an output, ``grid``'s rows and the
    width and device of ``like``: the kernels write rows x D floats behind the pointer they are given."""
    if t.dtype != torch.float32 or not t.is_contiguous() or t.dim() != 2 or not t.is_cuda:
        raise ValueError(f"{what} must be a contiguous fp32 matrix on the GPU (got {t.dtype} {tuple(t.shape)} on {t.device})")
    if like is not None and (tuple(t.shape) != (grid * grid + 1, like.shape[1]) or t.device != like.device):
        raise ValueError(f"{what} must be [{grid * grid + 1}, {like.shape[1]}] on {like.device} (got {tuple(t.shape)} on {t.device})")
    return t


def _grid(g) -> int:
    g = int(g)
    if not 1 <= g <= MAX_GRID:
        raise ValueError(f"a grid must lie in 1..{MAX_GRID} (got {g})")
    return g


def resample(pos: torch.Tensor, g_out: int, out: torch.Tensor = None) -> torch.Tensor:
    """Device op: ``pos`` fp32 [g_in^2 + 1, D] -> [g_out^2 + 1, D] (``out``, or a new tensor)."""
    g_in, D, g_out = _grid(grid_of(_table(pos, "resample: pos").shape[0])), pos.shape[1], _grid(g_out)
    if out is None:
        out = torch.empty(g_out * g_out + 1, D, dtype=torch.float32, device=pos.device)
    _table(out, "resample: out", pos, g_out)
    wy, wx = device_tables(g_in, g_out, pos.device)
    check(lib().ce_pos_resample_fwd(ptr(pos), g_in, ptr(wy), ptr(wx), ptr(out), int(g_out), D, stream()), "ce_pos_resample_fwd")
    return out


def resample_backward(dout: torch.Tensor, g_in: int, accumulate: bool = False, out: torch.Tensor = None) -> torch.Tensor:
    """Device op, the transpose: ``dout`` fp32 [g_out^2 + 1, D] -> [g_in^2 + 1, D]; stored into a new tensor, or stored /
    added (``accumulate``) into ``out``."""
    g_out, D, g_in = _grid(grid_of(_table(dout, "resample_backward: dout").shape[0])), dout.shape[1], _grid(g_in)
    if out is None:
        if accumulate:
            raise ValueError("resample_backward: accumulate needs the tensor to add to (out=)")
        out = torch.empty(g_in * g_in + 1, D, dtype=torch.float32, device=dout.device)
    _table(out, "resample_backward: out", dout, g_in)
    wy, wx = device_tables(g_in, g_out, dout.device)
    check(lib().ce_pos_resample_bwd(ptr(dout), g_out, ptr(wy), ptr(wx), ptr(out), int(g_in), D, int(bool(accumulate)), stream()),
          "ce_pos_resample_bwd")
    return out


def resample_host(pos: torch.Tensor, g_out: int) -> torch.Tensor:
    """The operator on the host with the fp64 tables, the result rounded to fp32 (any device in, CPU out)."""
    p = pos.detach().cpu().double().numpy()
    g_in, D = grid_of(p.shape[0]), p.shape[1]
    w = weights(g_in, g_out)
    grid = np.einsum("ia,jb,abd->ijd", w, w, p[1:].reshape(g_in, g_in, D)).reshape(g_out * g_out, D)
    return torch.from_numpy(np.concatenate([p[:1], grid]).astype(np.float32))


def resize_visual_state_dict(sd: dict, image_size: int) -> dict:
    """A copy of the state dict ``sd`` whose ``visual.positional_embedding`` has the grid of ``image_size``: the permanent form,
    what open_clip does at load time.  ``build_model`` of the result is a model that is native at the new size.  Host only;
    every other entry is the same object as in ``sd``; at the table's own size so is the table."""
    patch = int(sd["visual.conv1.weight"].shape[-1])
    g = check_image_size(image_size, patch)
    pos = sd["visual.positional_embedding"]
    out = dict(sd)
    if grid_of(pos.shape[0]) != g:
        out["visual.positional_embedding"] = resample_host(pos, g).to(dtype=pos.dtype)
    return out
