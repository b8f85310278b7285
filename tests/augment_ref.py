"""CPU reference (TEST INFRASTRUCTURE ONLY) of the training augmentation: Pillow's pixel arithmetic restated
in numpy (``Blend.c``, ``Convert.c``, ``ImageEnhance``; tests/test_augment_cpu.py pins every function against Pillow
itself, bit for bit), the pipeline ``augment`` computes, and the planner's draws written out a second time.  The
resampling is ``oracle.preprocess_oracle.resize_bicubic_u8``."""
import math

import numpy as np

from oracle import preprocess_oracle as P

F32, F64 = np.float32, np.float64
OPS = ("brightness", "contrast", "saturation", "hue")
SALT = 0x85A308D3


def luma(img):
    """``convert("L")``: uint8 [..., 3] -> uint8 [...]."""
    v = img.astype(np.int64)
    return ((19595 * v[..., 0] + 38470 * v[..., 1] + 7471 * v[..., 2] + 0x8000) >> 16).astype(np.uint8)


def blend(deg, px, f):
    """``Image.blend(deg, px, f)`` (Blend.c) on uint8 arrays of one shape; every operation in float32."""
    f = F32(f)
    t = deg.astype(F32) + f * (px.astype(np.int32) - deg.astype(np.int32)).astype(F32)
    assert t.dtype == F32
    if F32(0) <= f <= F32(1):
        return t.astype(np.int32).astype(np.uint8)
    return np.where(t <= 0, 0, np.where(t >= 255, 255, t.astype(np.int32))).astype(np.uint8)


def brightness(img, f):
    return blend(np.zeros_like(img), img, f)


def saturation(img, f):
    return blend(np.repeat(luma(img)[..., None], 3, axis=-1), img, f)


def contrast_mean(img):
    """``int(ImageStat.Stat(img.convert("L")).mean[0] + 0.5)`` in integers."""
    total, n = int(luma(img).astype(np.int64).sum()), img.shape[0] * img.shape[1]
    return (2 * total + n) // (2 * n)


def contrast(img, f):
    return blend(np.full_like(img, contrast_mean(img)), img, f)


def rgb_to_hsv(img):
    """``convert("HSV")`` (Convert.c rgb2hsv_row)."""
    r, g, b = img[..., 0], img[..., 1], img[..., 2]
    maxc, minc = np.maximum(r, np.maximum(g, b)), np.minimum(r, np.minimum(g, b))
    flat = maxc == minc
    with np.errstate(divide="ignore", invalid="ignore"):
        cr = (maxc.astype(np.int32) - minc).astype(F32)
        s = cr / maxc.astype(F32)
        rc = (maxc.astype(np.int32) - r).astype(F32) / cr
        gc = (maxc.astype(np.int32) - g).astype(F32) / cr
        bc = (maxc.astype(np.int32) - b).astype(F32) / cr
        h = np.where(r == maxc, bc - gc,
                     np.where(g == maxc, (2.0 + rc.astype(F64) - bc.astype(F64)).astype(F32),
                              (4.0 + gc.astype(F64) - rc.astype(F64)).astype(F32)))
        h = np.fmod(h.astype(F64) / 6.0 + 1.0, 1.0).astype(F32)
        H = np.clip(np.nan_to_num(h.astype(F64) * 255.0).astype(np.int64), 0, 255)
        S = np.clip(np.nan_to_num(s.astype(F64) * 255.0).astype(np.int64), 0, 255)
    H, S = np.where(flat, 0, H), np.where(flat, 0, S)
    return np.stack([H, S, maxc], axis=-1).astype(np.uint8)


def _rnd(x):
    return np.clip(np.floor(x.astype(F64) + 0.5).astype(np.int64), 0, 255)


def hsv_to_rgb(hsv):
    """``convert("RGB")`` of an HSV image (Convert.c hsv2rgb)."""
    H, S, V = hsv[..., 0], hsv[..., 1], hsv[..., 2]
    fh = H.astype(F32) * F32(6) / F32(255)
    i = np.floor(fh)
    f = fh - i
    fs = S.astype(F32) / F32(255)
    v = V.astype(F32)
    one = F32(1)
    p = _rnd(v * (one - fs))
    q = _rnd(v * (one - fs * f))
    t = _rnd(v * (one - fs * (one - f)))
    v = V.astype(np.int64)
    k = i.astype(np.int64) % 6
    table = [(v, t, p), (q, v, p), (p, v, t), (p, q, v), (t, p, v), (v, p, q)]
    out = np.empty(hsv.shape, dtype=np.int64)
    for c in range(3):
        out[..., c] = np.select([k == j for j in range(6)], [table[j][c] for j in range(6)])
        out[..., c] = np.where(S == 0, v, out[..., c])
    return out.astype(np.uint8)


def hue(img, shift):
    hsv = rgb_to_hsv(img)
    hsv[..., 0] = ((hsv[..., 0].astype(np.int64) + int(shift)) % 256).astype(np.uint8)
    return hsv_to_rgb(hsv)


def apply_op(img, name, value):
    return {"brightness": brightness, "contrast": contrast, "saturation": saturation, "hue": hue}[name](img, value)


def crop_resize(img, box, n_px):
    """``Image.crop(box).resize((n_px, n_px), BICUBIC)``, box = (x0, y0, x1, y1)."""
    x0, y0, x1, y1 = box
    return P.resize_bicubic_u8(np.ascontiguousarray(img[y0:y1, x0:x1]), n_px, n_px)


def augment_u8(img, box, flip=False, ops=(), grey=False, n_px=224):
    """The 8-bit image after crop + resize, flip, the op list in its order, greyscale."""
    x = crop_resize(img, box, n_px)
    if flip:
        x = np.ascontiguousarray(x[:, ::-1])
    for name, value in ops:
        x = apply_op(x, name, value)
    if grey:
        x = np.repeat(luma(x)[..., None], 3, axis=-1)
    return x


def augment(img, box, flip=False, ops=(), grey=False, n_px=224):
    """float32 [3, n_px, n_px]: ``augment_u8`` then ToTensor and Normalize as in ``oracle.preprocess_oracle.transform``."""
    t = augment_u8(img, box, flip, ops, grey, n_px).astype(F32) / F32(255.0)
    t = (t - P.MEAN[None, None, :]) / P.STD[None, None, :]
    return np.ascontiguousarray(t.transpose(2, 0, 1)).astype(F32)


# ---------------------------------------------------------------------------------------------------------------
# the planner, a second time (plain Python integers)


def fmix32(h):
    h &= 0xFFFFFFFF
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & 0xFFFFFFFF
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & 0xFFFFFFFF
    return h ^ (h >> 16)


def uniform(seed_r, draw, sample, slot):
    k = fmix32((seed_r + SALT) & 0xFFFFFFFF)
    for v in (draw, sample, slot):
        k = fmix32(k ^ (v & 0xFFFFFFFF))
    return k / 4294967296.0


def plan_one(seed_r, draw, sample, W, H, scale=(0.9, 1.0), ratio=(3 / 4, 4 / 3), hflip=0.0, color_jitter=None,
             color_jitter_prob=0.8, gray_scale_prob=0.0):
    """(box, flip, ops, grey, fell_back) of one image; slots as in DESIGN 4j."""
    u = lambda slot: uniform(seed_r, draw, sample, slot)
    box, fell_back = None, False
    for t in range(10):
        area = W * H * (scale[0] + (scale[1] - scale[0]) * u(16 + 4 * t))
        aspect = math.exp(math.log(ratio[0]) + (math.log(ratio[1]) - math.log(ratio[0])) * u(17 + 4 * t))
        w, h = int(round(math.sqrt(area * aspect))), int(round(math.sqrt(area / aspect)))
        if 0 < w <= W and 0 < h <= H:
            y0, x0 = int(u(18 + 4 * t) * (H - h + 1)), int(u(19 + 4 * t) * (W - w + 1))
            box = (x0, y0, x0 + w, y0 + h)
            break
    if box is None:
        fell_back = True
        if W / H < ratio[0]:
            w, h = W, int(round(W / ratio[0]))
        elif W / H > ratio[1]:
            w, h = int(round(H * ratio[1])), H
        else:
            w, h = W, H
        x0, y0 = (W - w) // 2, (H - h) // 2
        box = (x0, y0, x0 + w, y0 + h)
    flip = u(2) < hflip
    ops = []
    if color_jitter is not None and u(0) < color_jitter_prob:
        order = sorted(range(4), key=lambda k: (u(7 + k), k))
        for k in order:
            v = color_jitter[k]
            if v == 0:
                continue
            if k < 3:
                lo = max(0.0, 1.0 - v)
                ops.append((OPS[k], float(F32(lo + (1.0 + v - lo) * u(3 + k)))))
            else:
                ops.append((OPS[k], int((-v + 2.0 * v * u(3 + k)) * 255) % 256))
    grey = u(1) < gray_scale_prob
    return box, flip, ops, grey, fell_back
