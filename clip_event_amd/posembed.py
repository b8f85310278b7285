"""The image tower's positional table on another patch grid.

``weights`` is the operator itself: the separable bicubic (``a = -0.5``), antialiased, ``align_corners=False`` resampling of
``torch.nn.functional.interpolate`` -- what open_clip's ``resize_pos_embed`` and timm's ``resample_abs_pos_embed`` apply --
as one dense matrix per axis, host arithmetic in fp64.  ``resample`` / ``resample_backward`` apply it (and its transpose) on
the device with the fp32 roundings of those matrices (``ce_pos_resample_fwd`` / ``ce_pos_resample_bwd``);
``resize_visual_state_dict`` applies the fp64 matrices on the host, once, to a state dict.

The text tower's table at another context length is the second half of the module: ``text_weights`` defines the
operator (leading rows copied, the rest stretched linearly; truncation when shorter), ``stretch`` / ``stretch_backward`` apply it
on the device (``ce_pos_stretch_fwd`` / ``ce_pos_stretch_bwd``), ``stretch_host`` / ``resize_text_state_dict`` on the host.
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


# ---- the text tower's positional table at another context length ----------------------------------------------

MIN_CONTEXT, MAX_CONTEXT = 2, 1024
DEFAULT_KEEP = 20


def check_context_length(T) -> int:
    """A run length of the text tower: an integer in 2 .. 1024 (SOT and EOT need two rows; the stretch kernels take 1024);
    ValueError otherwise."""
    if isinstance(T, bool) or not isinstance(T, (int, np.integer)):
        raise ValueError(f"the context length must be an integer (got {T!r})")
    T = int(T)
    if not MIN_CONTEXT <= T <= MAX_CONTEXT:
        raise ValueError(f"the context length must lie in {MIN_CONTEXT}..{MAX_CONTEXT} (got {T})")
    return T


def text_weights(t_in: int, t_out: int, keep: int = DEFAULT_KEEP) -> np.ndarray:
    """fp64 [t_out, t_in], the operator that takes a ``t_in``-row text positional table to ``t_out`` rows.

    ``t_out <= t_in``: row j is the unit row e_j (truncation; ``keep`` is ignored).  ``t_out > t_in``, with
    ``k = min(keep, t_in - 1)``: rows ``j < k`` are e_j (the leading positions are copied); row ``j >= k`` has the source
    coordinate ``u = k + (j - k) (t_in - k) / (t_out - k)``, ``i0 = floor(u)``, ``w = u - i0`` and carries ``1 - w`` on ``i0``
    and ``w`` on ``min(i0 + 1, t_in - 1)``.  Every row sums to 1 and has at most two non-zeros.  This definition is the
    contract: a linear stretch of the rows behind the first ``keep`` (77 -> 248 with keep 20 is exactly 4x)."""
    t_in, t_out, keep = int(t_in), int(t_out), int(keep)
    if t_in < 1 or t_out < 1 or keep < 0:
        raise ValueError(f"lengths must be positive and keep non-negative (got {t_in} -> {t_out}, keep {keep})")
    w = np.zeros((t_out, t_in), dtype=np.float64)
    if t_out <= t_in:
        w[np.arange(t_out), np.arange(t_out)] = 1.0
        return w
    k = min(keep, t_in - 1)
    for j in range(t_out):
        if j < k:
            w[j, j] = 1.0
            continue
        u = k + (j - k) * (t_in - k) / (t_out - k)
        i0 = int(np.floor(u))
        f = u - i0
        w[j, i0] += 1.0 - f
        w[j, min(i0 + 1, t_in - 1)] += f
    return w


def stretch_host(pos, t_out: int, keep: int = DEFAULT_KEEP) -> np.ndarray:
    """``text_weights(t_in, t_out, keep) @ pos`` in fp64 (tensor or array in, fp64 array out), each row formed as its one or
    two products, rounded separately, and their sum: a fixed arithmetic (a BLAS product may fuse the multiply-adds) that
    ``ce_pos_stretch_fwd`` repeats on the device, so the device table is the fp32 rounding of this one bit for bit."""
    p = pos.detach().cpu().double().numpy() if isinstance(pos, torch.Tensor) else np.asarray(pos, dtype=np.float64)
    i0, w, _ = stretch_tables(p.shape[0], t_out, keep)
    first = w[:, :1] * p[i0]
    return np.where(w[:, 1:] == 0.0, first, first + w[:, 1:] * p[np.minimum(i0 + 1, p.shape[0] - 1)])


def stretch_tables(t_in: int, t_out: int, keep: int = DEFAULT_KEEP):
    """The kernels' form of ``text_weights`` (host arrays): ``i0`` int32 [t_out] = each row's first non-zero, ``w`` fp64
    [t_out, 2] = its weight and the next column's (0 when the row has one non-zero), ``span`` int32 [t_in, 2] = the contiguous
    range [lo, hi) of run rows with a non-zero in each native column (empty: lo = hi)."""
    W = text_weights(t_in, t_out, keep)
    i0 = (W != 0).argmax(axis=1).astype(np.int32)
    nxt = np.minimum(i0 + 1, t_in - 1)
    rows = np.arange(t_out)
    w = np.stack([W[rows, i0], np.where(nxt > i0, W[rows, nxt], 0.0)], axis=1)
    span = np.zeros((t_in, 2), dtype=np.int32)
    for i in range(t_in):
        nz = np.flatnonzero(W[:, i])
        if nz.size:
            span[i] = (nz[0], nz[-1] + 1)
    return i0, w, span


_STRETCH = {}


def stretch_device_tables(t_in: int, t_out: int, keep: int, device):
    """``stretch_tables`` on ``device``, cached per (lengths, keep, device)."""
    key = (int(t_in), int(t_out), int(keep), str(device))
    t = _STRETCH.get(key)
    if t is None:
        t = _STRETCH[key] = tuple(torch.from_numpy(a).to(device) for a in stretch_tables(t_in, t_out, keep))
    return t


def _text_table(t: torch.Tensor, what: str, rows: int = None, like: torch.Tensor = None) -> torch.Tensor:
    if t.dtype != torch.float32 or not t.is_contiguous() or t.dim() != 2 or not t.is_cuda:
        raise ValueError(f"{what} must be a contiguous fp32 matrix on the GPU (got {t.dtype} {tuple(t.shape)} on {t.device})")
    if like is not None and (tuple(t.shape) != (rows, like.shape[1]) or t.device != like.device):
        raise ValueError(f"{what} must be [{rows}, {like.shape[1]}] on {like.device} (got {tuple(t.shape)} on {t.device})")
    return t


def _length(t) -> int:
    t = int(t)
    if not 1 <= t <= MAX_CONTEXT:
        raise ValueError(f"a table length must lie in 1..{MAX_CONTEXT} (got {t})")
    return t


def stretch(pos: torch.Tensor, t_out: int, keep: int = DEFAULT_KEEP, out: torch.Tensor = None) -> torch.Tensor:
    """Device op: ``pos`` fp32 [t_in, D] -> [t_out, D] (``out``, or a new tensor): ``text_weights`` applied in fp64 and rounded to
    fp32 once, i.e. the fp32 rounding of ``stretch_host``."""
    t_in, D, t_out = _length(_text_table(pos, "stretch: pos").shape[0]), pos.shape[1], _length(t_out)
    if out is None:
        out = torch.empty(t_out, D, dtype=torch.float32, device=pos.device)
    _text_table(out, "stretch: out", t_out, pos)
    i0, w, _ = stretch_device_tables(t_in, t_out, keep, pos.device)
    check(lib().ce_pos_stretch_fwd(ptr(pos), t_in, ptr(i0), ptr(w), ptr(out), t_out, D, stream()), "ce_pos_stretch_fwd")
    return out


def stretch_backward(dout: torch.Tensor, t_in: int, keep: int = DEFAULT_KEEP, accumulate: bool = False,
                     out: torch.Tensor = None) -> torch.Tensor:
    """Device op, the transpose: ``dout`` fp32 [t_out, D] -> [t_in, D]; stored into a new tensor, or stored / added
    (``accumulate``) into ``out``."""
    t_out, D, t_in = _length(_text_table(dout, "stretch_backward: dout").shape[0]), dout.shape[1], _length(t_in)
    if out is None:
        if accumulate:
            raise ValueError("stretch_backward: accumulate needs the tensor to add to (out=)")
        out = torch.empty(t_in, D, dtype=torch.float32, device=dout.device)
    _text_table(out, "stretch_backward: out", t_in, dout)
    i0, w, span = stretch_device_tables(t_in, t_out, keep, dout.device)
    check(lib().ce_pos_stretch_bwd(ptr(dout), t_out, ptr(i0), ptr(w), ptr(span), ptr(out), t_in, D, int(bool(accumulate)),
                                   stream()), "ce_pos_stretch_bwd")
    return out


def resize_text_state_dict(sd: dict, T: int, keep: int = DEFAULT_KEEP) -> dict:
    """A copy of the state dict ``sd`` whose ``positional_embedding`` has ``T`` rows (``stretch_host`` rounded to the table's
    dtype): the permanent form -- ``build_model`` of the result is a model that is native at ``T``.  Host only; every other
    entry is the same object as in ``sd``; at the table's own length so is the table."""
    T = check_context_length(T)
    pos = sd["positional_embedding"]
    out = dict(sd)
    if pos.shape[0] != T:
        out["positional_embedding"] = torch.from_numpy(stretch_host(pos, T, keep)).to(dtype=pos.dtype)
    return out
