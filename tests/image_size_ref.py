"""Numpy restatement of the positional-table resampling, independent of clip_event_amd/posembed.py: the weight
tables written out tap by tap, the operator and its transpose as fp64 products, and the per-element rounding bounds of the fp32
kernels."""
import numpy as np

U = 2.0 ** -24                     # unit roundoff of fp32
# the grid pairs the tables are checked on (upsampling, antialiased downsampling, non-integer ratios, a single cell)
PAIRS = [(7, 14), (7, 4), (7, 10), (16, 24), (24, 16), (14, 5), (7, 2), (7, 1), (6, 4), (6, 10), (6, 12)]


def cubic(x: float) -> float:
    a, x = -0.5, abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0
    if x < 2.0:
        return (((x - 5.0) * x + 8.0) * x - 4.0) * a
    return 0.0


def weights(n_in: int, n_out: int) -> np.ndarray:
    """fp64 [n_out, n_in], one scalar at a time."""
    scale = n_in / n_out
    support = 2.0 * scale if scale >= 1.0 else 2.0
    inv = 1.0 / scale if scale >= 1.0 else 1.0
    w = np.zeros((n_out, n_in))
    for i in range(n_out):
        c = scale * (i + 0.5)
        lo = max(0, int(c - support + 0.5))
        hi = min(n_in, int(c + support + 0.5))
        taps = [cubic((j - c + 0.5) * inv) for j in range(lo, hi)]
        total = sum(taps)
        for j, t in zip(range(lo, hi), taps):
            w[i, j] = t / total
    return w


def tables32(g_in: int, g_out: int) -> np.ndarray:
    """What the device receives: the fp32 rounding of ``weights``, as fp64 numbers."""
    return weights(g_in, g_out).astype(np.float32).astype(np.float64)


def forward(pos: np.ndarray, w: np.ndarray) -> np.ndarray:
    """``pos`` [g_in^2 + 1, D] -> [g_out^2 + 1, D] in fp64 with the table ``w`` [g_out, g_in] on both axes."""
    g_out, g_in = w.shape
    p = np.asarray(pos, dtype=np.float64)
    grid = np.einsum("ia,jb,abd->ijd", w, w, p[1:].reshape(g_in, g_in, -1)).reshape(g_out * g_out, -1)
    return np.concatenate([p[:1], grid])


def backward(dout: np.ndarray, w: np.ndarray) -> np.ndarray:
    """The transpose: ``dout`` [g_out^2 + 1, D] -> [g_in^2 + 1, D]."""
    g_out, g_in = w.shape
    d = np.asarray(dout, dtype=np.float64)
    grid = np.einsum("ia,jb,ijd->abd", w, w, d[1:].reshape(g_out, g_out, -1)).reshape(g_in * g_in, -1)
    return np.concatenate([d[:1], grid])


def forward_bound(pos: np.ndarray, w: np.ndarray) -> np.ndarray:
    """Per element ``(k + 2) u sum |wy| |wx| |x|``: ``k`` counts the non-zero terms of that element's two nested sums (the inner
    sums' terms plus the outer sum's), the standard bound of recursive summation with one rounding per product.  Row 0 is a copy:
    bound 0."""
    a = np.abs(w)
    nz = (w != 0).sum(axis=1)                                     # taps per output index
    k = nz[:, None] * nz[None, :] + nz[:, None]                   # [i, j]: taps_y * taps_x inner terms + taps_y outer terms
    mag = forward(np.abs(pos), a)
    out = np.zeros_like(mag)
    out[1:] = ((k.reshape(-1) + 2) * U)[:, None] * mag[1:]
    return out


def backward_bound(dout: np.ndarray, w: np.ndarray, base: np.ndarray = None) -> np.ndarray:
    """The same for the transpose; with ``base`` (accumulate = 1) one more addition per element, row 0 included."""
    a = np.abs(w)
    nz = (w != 0).sum(axis=0)                                     # output cells that read each input index
    k = nz[:, None] * nz[None, :] + nz[:, None]
    mag = backward(np.abs(dout), a)
    out = np.zeros_like(mag)
    out[1:] = ((k.reshape(-1) + 2) * U)[:, None] * mag[1:]
    if base is not None:
        out = out + U * (mag + np.abs(base)) + out * U
    return out
