"""On-device image preprocessing: ``clip._transform`` (clip.py:62-69) and the object-patch path
(dataset_voa.py:195-233) for a batch of decoded uint8 images resident in HBM.

The reference runs PIL + torchvision per image on the host (``num_workers=0``, train.py:212); here the host only
fills one small geometry record per output (sizes are integers known from the image headers) and three HIP
launches do the rest, bit for bit (Pillow's bicubic resampling incl. its 8-bit intermediate and fixed-point taps,
torchvision's size / crop rules, ``/255`` and ``(x - mean) / std`` in correctly rounded fp32).

``augment`` / ``Augment`` are the training-time counterpart (open_clip's ``image_transform(is_train=True)``): random resized
crop, flip, colour jitter and greyscale on the same images, equally bit for bit, with replayable draws.
"""
from __future__ import annotations

import ctypes
import math
from ctypes import c_float, c_int, c_long, c_void_p
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from ._lib import check, lib, ptr, stream

MEAN = (0.48145466, 0.4578275, 0.40821073)
STD = (0.26862954, 0.26130258, 0.27577711)


class _Desc(ctypes.Structure):
    """``ce_preproc_desc`` of include/clip_event_hip.h."""
    _fields_ = [("src", c_void_p), ("pitch", c_long), ("x0", c_int), ("y0", c_int), ("w", c_int), ("h", c_int),
                ("ow", c_int), ("oh", c_int), ("left", c_int), ("top", c_int), ("row0", c_int), ("rows", c_int),
                ("tmp_off", c_long)]


def resized_size(w: int, h: int, n_px: int) -> Tuple[int, int]:
    """torchvision ``Resize(n_px)``: shorter side -> n_px, longer ``int(n_px * long / short)``; no-op if already so."""
    if (w <= h and w == n_px) or (h <= w and h == n_px):
        return w, h
    if w < h:
        return n_px, int(n_px * h / w)
    return int(n_px * w / h), n_px


def crop_offsets(ow: int, oh: int, n_px: int) -> Tuple[int, int]:
    """torchvision ``CenterCrop``: ``int(round((size - n_px) / 2.0))`` (round half to even)."""
    return int(round((ow - n_px) / 2.0)), int(round((oh - n_px) / 2.0))


def _bounds(in_size: int, out_size: int, xx: int) -> Tuple[int, int]:
    """First source index and tap count of output index ``xx`` (Pillow ``precompute_coeffs``)."""
    if in_size == out_size:
        return xx, 1
    scale = in_size / out_size
    support = 2.0 * max(scale, 1.0)
    center = (xx + 0.5) * scale
    lo = max(int(center - support + 0.5), 0)
    hi = min(int(center + support + 0.5), in_size)
    return lo, hi - lo


def _checked(images, what: str):
    """The batch as a list of uint8 [H, W, 3] tensors with dense pixels on one GPU (copies made where needed), and that GPU."""
    if not images:
        raise ValueError(f"{what}: empty batch")
    dev = images[0].device
    if dev.type != "cuda":
        raise RuntimeError(f"{what} runs on the GPU: move the decoded images there first (no CPU fallback)")
    images = list(images)
    for i, im in enumerate(images):
        if im.dtype != torch.uint8 or im.dim() != 3 or im.shape[2] != 3 or im.device != dev:
            raise ValueError(f"{what}: images must be uint8 [H, W, 3] tensors on one GPU")
        if im.stride(2) != 1 or im.stride(1) != 3:
            images[i] = im.contiguous()
    return images, dev


def preprocess(images: Sequence[torch.Tensor], rois: Optional[Sequence[Optional[Sequence[Tuple[int, int, int, int]]]]] = None,
               n_px: int = 224) -> torch.Tensor:
    """``images``: uint8 HWC RGB tensors on the GPU (any sizes).  ``rois`` (optional, per image): list of
    ``(x0, y0, x1, y1)`` boxes inside the image; each image then yields the whole-image tensor FOLLOWED by one tensor
    per box, in that order (dataset_voa.py:195-233).  Returns fp32 ``[n_out, 3, n_px, n_px]``."""
    images, dev = _checked(images, "preprocess")
    regions = []
    for i, im in enumerate(images):
        H, W = int(im.shape[0]), int(im.shape[1])
        boxes = [(0, 0, W, H)] + [tuple(int(v) for v in b) for b in ((rois[i] or []) if rois is not None else [])]
        for (x0, y0, x1, y1) in boxes:
            if not (0 <= x0 < x1 <= W and 0 <= y0 < y1 <= H):
                raise ValueError(f"preprocess: box {(x0, y0, x1, y1)} is not inside the {W}x{H} image")
            regions.append((im, x0, y0, x1 - x0, y1 - y0))
    n_out = len(regions)
    descs = (_Desc * n_out)()
    tmp_bytes, max_rows, max_scale = 0, 1, 1.0
    for o, (im, x0, y0, w, h) in enumerate(regions):
        ow, oh = resized_size(w, h, n_px)
        left, top = crop_offsets(ow, oh, n_px)
        r_first, _ = _bounds(h, oh, top)
        r_last, cnt = _bounds(h, oh, top + n_px - 1)
        rows = r_last + cnt - r_first
        d = descs[o]
        d.src, d.pitch = im.data_ptr(), im.stride(0)
        d.x0, d.y0, d.w, d.h, d.ow, d.oh, d.left, d.top = x0, y0, w, h, ow, oh, left, top
        d.row0, d.rows, d.tmp_off = r_first, rows, tmp_bytes
        tmp_bytes += rows * n_px * 3
        max_rows = max(max_rows, rows)
        max_scale = max(max_scale, w / ow, h / oh)
    kmax = int(math.ceil(2.0 * max_scale)) * 2 + 1
    cl = lib()
    table = torch.empty(cl.ce_preprocess_table_bytes(n_out, n_px, kmax), dtype=torch.uint8, device=dev)
    tmp = torch.empty(max(tmp_bytes, 1), dtype=torch.uint8, device=dev)
    out = torch.empty(n_out, 3, n_px, n_px, dtype=torch.float32, device=dev)
    descs_d = torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8).to(dev)
    mean = (c_float * 3)(*MEAN)
    std = (c_float * 3)(*STD)
    check(cl.ce_preprocess(ptr(descs_d), n_out, n_px, kmax, max_rows, ptr(table), ptr(tmp),
                           ptr(out), mean, std, stream()), "ce_preprocess")
    out._keepalive = (descs_d, table, tmp, list(images))   # until the stream has consumed them
    return out


# ---------------------------------------------------------------------------------------------------------------------
# Training augmentation: open_clip's ``image_transform(is_train=True)`` -- ``RandomResizedCrop(n_px, scale,
# ratio, BICUBIC)``, then the ``--aug-cfg`` extras ``ColorJitter`` (applied with a probability) and ``RandomGrayscale`` --
# plus a horizontal flip, bit for bit with torchvision's PIL path, with counter-based draws.

OPS = ("brightness", "contrast", "saturation", "hue")       # CE_AUG_* of include/clip_event_hip.h
AUG_SALT = 0x85A308D3                                        # patch dropout's is 0x9E3779B9: independent draws under one seed
MAX_N_PX = 2896                                              # 255 * n_px^2 fits the int32 luma sum
# slots of one (draw, sample): the three decisions, the four factors, the four permutation keys, then ten crop tries
SLOT_JITTER, SLOT_GREY, SLOT_FLIP, SLOT_FACTOR, SLOT_ORDER, SLOT_CROP, CROP_TRIES = 0, 1, 2, 3, 7, 16, 10
N_SLOTS = SLOT_CROP + 4 * CROP_TRIES


class _AugDesc(ctypes.Structure):
    """``ce_augment_desc`` of include/clip_event_hip.h."""
    _fields_ = [("flip", c_int), ("grey", c_int), ("n_ops", c_int), ("op", c_int * 4), ("factor", c_float * 4)]


def _fmix32(h: int) -> int:
    """murmur3 finaliser, as in csrc/embed.hip."""
    h &= 0xFFFFFFFF
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & 0xFFFFFFFF
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & 0xFFFFFFFF
    return h ^ (h >> 16)


def _fmix32_array(h: np.ndarray) -> np.ndarray:
    """``_fmix32`` on uint32 values held in a uint64 array (no product is lost)."""
    m = np.uint64(0xFFFFFFFF)
    h = h & m
    h = h ^ (h >> np.uint64(16))
    h = (h * np.uint64(0x85EBCA6B)) & m
    h = h ^ (h >> np.uint64(13))
    h = (h * np.uint64(0xC2B2AE35)) & m
    return h ^ (h >> np.uint64(16))


def _op_list(ops) -> List[Tuple[int, float]]:
    """``[(name, value), ...]`` checked and as ``(CE_AUG_* code, float32 factor)``."""
    ops = list(ops or [])
    if len(ops) > 4:
        raise ValueError(f"augment: {len(ops)} ops in one list (at most 4)")
    out = []
    for name, value in ops:
        if name not in OPS:
            raise ValueError(f"augment: unknown op '{name}' (one of {OPS})")
        if value < 0:
            raise ValueError(f"augment: negative factor {value} for {name}")
        if name == "hue" and (int(value) != value or value > 255):
            raise ValueError(f"augment: the hue shift is an integer 0..255 of the 8-bit hue, not {value}")
        out.append((OPS.index(name), float(np.float32(value))))
    if sum(1 for code, _ in out if code == 1) > 1:
        raise ValueError("augment: contrast listed twice (its mean is taken once per image)")
    return out


def augment(images: Sequence[torch.Tensor], boxes: Sequence[Tuple[int, int, int, int]], flip: Optional[Sequence[bool]] = None,
            ops: Optional[Sequence[Optional[Sequence[Tuple[str, float]]]]] = None, grey: Optional[Sequence[bool]] = None,
            n_px: int = 224) -> torch.Tensor:
    """The explicit form of the training transform: output ``i`` is ``images[i].crop(boxes[i])`` (``(x0, y0, x1, y1)`` inside
    the image, any size) resized to ``n_px`` x ``n_px`` (BICUBIC), mirrored if ``flip[i]``, put through ``ops[i]`` =
    ``[(name, value), ...]`` in that order (``brightness`` / ``contrast`` / ``saturation`` with an enhancement factor >= 0,
    ``hue`` with the integer shift 0..255 of the 8-bit hue; at most four, contrast at most once), turned grey if
    ``grey[i]``, then ``ToTensor`` and ``Normalize``.  The same tensor may be listed several times.  Returns fp32
    ``[n_out, 3, n_px, n_px]``, bit for bit what Pillow / torchvision give."""
    images, dev = _checked(images, "augment")
    n_out = len(images)
    if not 0 < n_px <= MAX_N_PX:
        raise ValueError(f"augment: n_px {n_px} outside 1..{MAX_N_PX}")
    for name, arg in (("boxes", boxes), ("flip", flip), ("ops", ops), ("grey", grey)):
        if (arg is not None or name == "boxes") and len(arg) != n_out:
            raise ValueError(f"augment: {len(arg)} {name} for {n_out} images")
    descs, augs = (_Desc * n_out)(), (_AugDesc * n_out)()
    tmp_bytes, max_rows, max_scale = 0, 1, 1.0
    for o, im in enumerate(images):
        H, W = int(im.shape[0]), int(im.shape[1])
        x0, y0, x1, y1 = (int(v) for v in boxes[o])
        if not (0 <= x0 < x1 <= W and 0 <= y0 < y1 <= H):
            raise ValueError(f"augment: box {(x0, y0, x1, y1)} is not inside the {W}x{H} image")
        w, h = x1 - x0, y1 - y0
        r_last, cnt = _bounds(h, n_px, n_px - 1)
        d = descs[o]
        d.src, d.pitch = im.data_ptr(), im.stride(0)
        d.x0, d.y0, d.w, d.h, d.ow, d.oh, d.left, d.top = x0, y0, w, h, n_px, n_px, 0, 0
        d.row0, d.rows, d.tmp_off = 0, r_last + cnt, tmp_bytes          # output row 0 reads region row 0
        tmp_bytes += d.rows * n_px * 3
        max_rows = max(max_rows, d.rows)
        max_scale = max(max_scale, w / n_px, h / n_px)
        a = augs[o]
        a.flip, a.grey = int(bool(flip[o])) if flip is not None else 0, int(bool(grey[o])) if grey is not None else 0
        listed = _op_list(ops[o]) if ops is not None else []
        a.n_ops = len(listed)
        for i, (code, value) in enumerate(listed):
            a.op[i], a.factor[i] = code, value
    kmax = int(math.ceil(2.0 * max_scale)) * 2 + 1
    cl = lib()
    work = torch.empty(cl.ce_augment_workspace_bytes(n_out, n_px, kmax, tmp_bytes), dtype=torch.uint8, device=dev)
    out = torch.empty(n_out, 3, n_px, n_px, dtype=torch.float32, device=dev)
    both = torch.frombuffer(bytearray(bytes(descs) + bytes(augs)), dtype=torch.uint8).to(dev)
    augs_d = both[ctypes.sizeof(descs):]
    mean = (c_float * 3)(*MEAN)
    std = (c_float * 3)(*STD)
    check(cl.ce_augment(ptr(both), ptr(augs_d), ctypes.addressof(augs), n_out, n_px, kmax, max_rows, ptr(work), ptr(out),
                        mean, std, stream()), "ce_augment")
    out._keepalive = (both, work, images)   # until the stream has consumed them
    return out


class Augment:
    """open_clip's training-time image transform on the device, with replayable draws::

        aug = Augment(224, hflip=0.5, color_jitter=(0.32, 0.32, 0.32, 0.08), gray_scale_prob=0.2, seed=seed, rank=rank)
        x = aug(images, draw=step)              # fp32 [B, 3, 224, 224]

    ``scale``, ``ratio``: ``RandomResizedCrop``'s; ``hflip``: probability of a horizontal flip; ``color_jitter``: ``(brightness,
    contrast, saturation, hue)`` of torchvision's ``ColorJitter`` (hue <= 0.5), applied with probability
    ``color_jitter_prob``; ``gray_scale_prob``: ``RandomGrayscale``'s.  Every uniform is a hash of (seed, rank, draw, sample,
    slot) -- no generator, no state besides the draw counter: a pass can be replayed, rows ``k..`` of a plan are the plan
    at ``sample0=k``, and the ranks of one ``seed`` draw differently."""

    def __init__(self, n_px: int = 224, scale=(0.9, 1.0), ratio=(3 / 4, 4 / 3), hflip: float = 0.0, color_jitter=None,
                 color_jitter_prob: float = 0.8, gray_scale_prob: float = 0.0, seed: int = 0, rank: int = 0):
        from .functional import patch_keep_seed
        if not 0 < n_px <= MAX_N_PX:
            raise ValueError(f"Augment: n_px {n_px} outside 1..{MAX_N_PX}")
        if not (len(scale) == 2 and 0 < scale[0] <= scale[1]) or not (len(ratio) == 2 and 0 < ratio[0] <= ratio[1]):
            raise ValueError(f"Augment: scale {scale} / ratio {ratio} must be (lo, hi) with 0 < lo <= hi")
        for name, p in (("hflip", hflip), ("color_jitter_prob", color_jitter_prob), ("gray_scale_prob", gray_scale_prob)):
            if not 0.0 <= p <= 1.0:
                raise ValueError(f"Augment: {name} {p} is not a probability")
        if color_jitter is not None:
            color_jitter = tuple(float(v) for v in color_jitter)
            if len(color_jitter) != 4 or min(color_jitter) < 0 or color_jitter[3] > 0.5:
                raise ValueError(f"Augment: color_jitter {color_jitter} must be (brightness, contrast, saturation, hue), "
                                 "all >= 0 and hue <= 0.5")
        self.n_px, self.scale, self.ratio = int(n_px), (float(scale[0]), float(scale[1])), (float(ratio[0]), float(ratio[1]))
        self.hflip, self.color_jitter, self.color_jitter_prob = float(hflip), color_jitter, float(color_jitter_prob)
        self.gray_scale_prob = float(gray_scale_prob)
        self.seed, self.rank = int(seed), int(rank)
        self._base_seed = patch_keep_seed(seed, rank)
        self._base = _fmix32(self._base_seed + AUG_SALT)
        self.draw = 0

    def _uniforms(self, draw: int, sample0: int, n: int) -> np.ndarray:
        """``u[i][slot]`` of the samples ``sample0 .. sample0 + n - 1`` of pass ``draw``: key / 2^32, exact in a double."""
        samples = np.arange(n, dtype=np.uint64) + np.uint64(int(sample0) & 0xFFFFFFFF)
        c = _fmix32_array(np.uint64(_fmix32(self._base ^ (int(draw) & 0xFFFFFFFF))) ^ samples)
        keys = _fmix32_array(c[:, None] ^ np.arange(N_SLOTS, dtype=np.uint64)[None, :])
        return keys.astype(np.float64) / 4294967296.0

    def _boxes(self, sizes: Sequence[Tuple[int, int]], table: np.ndarray) -> List[Tuple[int, int, int, int]]:
        """torchvision ``RandomResizedCrop.get_params`` for every image: the ten tries at once, the first that fits taken."""
        (s0, s1), (r0, r1) = self.scale, self.ratio
        l0, l1 = math.log(r0), math.log(r1)
        u = table[:, SLOT_CROP:].reshape(len(sizes), CROP_TRIES, 4)
        W, H = (np.array(v, dtype=np.int64)[:, None] for v in zip(*sizes))
        area = (W * H) * (s0 + (s1 - s0) * u[:, :, 0])
        # (math.exp, not numpy's: numpy's vector exp may differ from it in the last place, and a plan must not depend on that)
        aspect = np.array([math.exp(v) for v in (l0 + (l1 - l0) * u[:, :, 1]).ravel().tolist()]).reshape(area.shape)
        w, h = np.rint(np.sqrt(area * aspect)).astype(np.int64), np.rint(np.sqrt(area / aspect)).astype(np.int64)
        fits = (0 < w) & (w <= W) & (0 < h) & (h <= H)
        y0, x0 = (u[:, :, 2] * (H - h + 1)).astype(np.int64), (u[:, :, 3] * (W - w + 1)).astype(np.int64)
        first, rows = fits.argmax(axis=1), np.arange(len(sizes))
        boxes = np.stack([x0, y0, x0 + w, y0 + h], axis=-1)[rows, first].tolist()
        for i in np.flatnonzero(~fits.any(axis=1)).tolist():          # no try fitted: the centre crop clamped to the ratio range
            Wi, Hi = int(W[i, 0]), int(H[i, 0])
            if Wi / Hi < r0:
                wi, hi = Wi, int(round(Wi / r0))
            elif Wi / Hi > r1:
                wi, hi = int(round(Hi * r1)), Hi
            else:
                wi, hi = Wi, Hi
            bx, by = (Wi - wi) // 2, (Hi - hi) // 2
            boxes[i] = [bx, by, bx + wi, by + hi]
        return [tuple(b) for b in boxes]

    def _jitters(self, table: np.ndarray) -> List[List[Tuple[str, float]]]:
        """torchvision ``ColorJitter.get_params`` + ``forward`` for every image: the ops whose setting is non-zero, in a drawn
        order (ascending order key, ties by op index), with drawn factors."""
        v = np.array(self.color_jitter)
        lo = np.maximum(0.0, 1.0 - v[:3])
        factor = (lo + (1.0 + v[:3] - lo) * table[:, SLOT_FACTOR:SLOT_FACTOR + 3]).astype(np.float32).astype(np.float64).tolist()
        shift = (((-v[3] + 2.0 * v[3] * table[:, SLOT_FACTOR + 3]) * 255).astype(np.int64) % 256).tolist()       # truncates toward zero
        order = np.argsort(table[:, SLOT_ORDER:SLOT_ORDER + 4], axis=1, kind="stable").tolist()
        live = [x != 0 for x in self.color_jitter]
        return [[(OPS[k], f[k] if k < 3 else s) for k in o if live[k]] for f, s, o in zip(factor, shift, order)]

    def plan(self, sizes: Sequence[Tuple[int, int]], draw: int, sample0: int = 0):
        """``(boxes, flips, ops, greys)`` for images of ``sizes`` = ``[(w, h), ...]``, the samples ``sample0..`` of pass
        ``draw``: host arithmetic, no GPU.  They are ``augment``'s arguments."""
        sizes = [(int(W), int(H)) for (W, H) in sizes]
        if not sizes:
            return [], [], [], []
        if min(min(s) for s in sizes) <= 0:
            raise ValueError(f"Augment.plan: image sizes {sizes}")
        table = self._uniforms(draw, sample0, len(sizes))
        flips, greys = (table[:, SLOT_FLIP] < self.hflip).tolist(), (table[:, SLOT_GREY] < self.gray_scale_prob).tolist()
        ops = [[] for _ in sizes]
        if self.color_jitter is not None:
            jittered = (table[:, SLOT_JITTER] < self.color_jitter_prob).tolist()
            ops = [o if j else [] for o, j in zip(self._jitters(table), jittered)]
        return self._boxes(sizes, table), flips, ops, greys

    def __call__(self, images: Sequence[torch.Tensor], draw: Optional[int] = None, sample0: int = 0) -> torch.Tensor:
        """Plan and run.  ``draw=None`` uses the object's own counter and advances it."""
        if draw is None:
            draw = self.draw
            self.draw += 1
        boxes, flips, ops, greys = self.plan([(int(im.shape[1]), int(im.shape[0])) for im in images], draw, sample0)
        return augment(images, boxes, flips, ops, greys, self.n_px)

    def state_dict(self) -> dict:
        return {"draw": self.draw}

    def load_state_dict(self, state: dict) -> None:
        self.draw = int(state["draw"])
