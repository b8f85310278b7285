"""Training augmentation, CPU: the numpy restatement of Pillow's pixel arithmetic (tests/augment_ref.py)
against Pillow itself, bit for bit, and the planner ``preprocess.Augment.plan`` (pure host arithmetic, no GPU)."""
import math

import numpy as np
import pytest

from tests import augment_ref as R

FACTORS = (0, 0.3, 0.68, 1, 1.0001, 1.32, 2.5)
JITTER = (0.32, 0.32, 0.32, 0.08)


def _img(w, h, seed):
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, size=(h // 8 + 2, w // 8 + 2, 3), dtype=np.uint8)
    img = np.kron(base, np.ones((8, 8, 1), dtype=np.uint8))[:h, :w]
    return np.clip(img.astype(np.int32) + rng.integers(-20, 21, size=img.shape), 0, 255).astype(np.uint8)


# ---------------------------------------------------------------------------------------------------------------
# 1. the restatement against Pillow


@pytest.fixture(scope="module")
def all_colours():
    v = np.arange(1 << 24, dtype=np.uint32)
    return np.stack([(v >> 16) & 255, (v >> 8) & 255, v & 255], axis=-1).astype(np.uint8).reshape(4096, 4096, 3)


@pytest.mark.parametrize("f", FACTORS)
def test_blend_matches_pillow_on_every_pair(f):
    """``Image.blend`` is what the three enhancers call: all 65,536 (deg, px) pairs through it, then each enhancer on
    images built so that its degenerate image takes every value."""
    from PIL import Image, ImageEnhance
    deg, px = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    ref = np.asarray(Image.blend(Image.fromarray(deg), Image.fromarray(px), f))
    assert np.array_equal(R.blend(deg, px, f), ref)
    rgb = np.stack([px, deg, px[::-1]], axis=-1)                        # every px on R; luma sweeps with G
    im = Image.fromarray(rgb)
    assert np.array_equal(R.brightness(rgb, f), np.asarray(ImageEnhance.Brightness(im).enhance(f)))
    assert np.array_equal(R.saturation(rgb, f), np.asarray(ImageEnhance.Color(im).enhance(f)))
    for mean in range(0, 256, 5):                                       # Contrast: one degenerate value per image
        one = np.stack([np.arange(256, dtype=np.uint8)] * 3, axis=-1)[None].copy()
        pad = np.full((60, 256, 3), mean, dtype=np.uint8)               # drags the mean luma towards `mean`
        img = np.concatenate([one, pad], axis=0)
        assert np.array_equal(R.contrast(img, f), np.asarray(ImageEnhance.Contrast(Image.fromarray(img)).enhance(f))), mean


def test_enhancers_match_pillow_on_random_images():
    from PIL import Image, ImageEnhance
    for seed, (w, h) in enumerate([(53, 37), (224, 224), (31, 64)]):
        img = _img(w, h, seed)
        im = Image.fromarray(img)
        for f in FACTORS + (0.9, 1.7):
            assert np.array_equal(R.brightness(img, f), np.asarray(ImageEnhance.Brightness(im).enhance(f)))
            assert np.array_equal(R.contrast(img, f), np.asarray(ImageEnhance.Contrast(im).enhance(f)))
            assert np.array_equal(R.saturation(img, f), np.asarray(ImageEnhance.Color(im).enhance(f)))


def test_luma_matches_pillow_on_every_colour(all_colours):
    from PIL import Image
    assert np.array_equal(R.luma(all_colours), np.asarray(Image.fromarray(all_colours).convert("L")))


def test_rgb_to_hsv_matches_pillow_on_every_colour(all_colours):
    from PIL import Image
    ref = np.asarray(Image.fromarray(all_colours).convert("HSV"))
    assert int((R.rgb_to_hsv(all_colours) != ref).any(-1).sum()) == 0


def test_hsv_to_rgb_matches_pillow_on_every_colour(all_colours):
    from PIL import Image
    ref = np.asarray(Image.fromarray(all_colours, mode="HSV").convert("RGB"))
    assert int((R.hsv_to_rgb(all_colours) != ref).any(-1).sum()) == 0


def test_hue_shift_matches_torchvisions_pil_path():
    """torchvision ``_functional_pil.adjust_hue``: split HSV, add uint8(hue_factor * 255) to H with wrap-around, merge."""
    from PIL import Image
    img = _img(64, 48, 9)
    for shift in (0, 1, 20, 128, 235, 255):
        h, s, v = Image.fromarray(img).convert("HSV").split()
        np_h = np.array(h, dtype=np.uint8)
        with np.errstate(over="ignore"):
            np_h += np.uint8(shift)
        ref = np.asarray(Image.merge("HSV", (Image.fromarray(np_h, "L"), s, v)).convert("RGB"))
        assert np.array_equal(R.hue(img, shift), ref), shift


@pytest.mark.parametrize("w,h,box,n", [(50, 40, (3, 5, 47, 38), 32), (33, 70, (0, 10, 33, 60), 33), (17, 23, (2, 3, 15, 20), 32),
                                       (100, 80, (10, 0, 100, 71), 33), (300, 260, (20, 10, 290, 250), 224),
                                       (32, 32, (0, 0, 32, 32), 32)])
def test_crop_resize_flip_matches_pillow(w, h, box, n):
    from PIL import Image
    img = _img(w, h, 3 * w + h)
    ref = np.asarray(Image.fromarray(img).crop(box).resize((n, n), Image.BICUBIC).transpose(Image.FLIP_LEFT_RIGHT))
    assert np.array_equal(R.augment_u8(img, box, flip=True, n_px=n), ref)
    assert np.array_equal(R.augment_u8(img, box, flip=False, n_px=n), ref[:, ::-1])


def test_whole_pipeline_matches_pillow():
    """crop, resize, flip, four ops in an order, greyscale, ToTensor, Normalize: the reference against Pillow + torch."""
    import torch
    from PIL import Image, ImageEnhance
    from oracle import preprocess_oracle as P
    img, box = _img(90, 70, 4), (5, 8, 80, 66)
    im = Image.fromarray(img).crop(box).resize((48, 48), Image.BICUBIC).transpose(Image.FLIP_LEFT_RIGHT)
    im = ImageEnhance.Color(im).enhance(1.2)
    im = ImageEnhance.Contrast(im).enhance(0.75)
    h, s, v = im.convert("HSV").split()
    np_h = np.array(h, dtype=np.uint8)
    with np.errstate(over="ignore"):
        np_h += np.uint8(240)
    im = Image.merge("HSV", (Image.fromarray(np_h, "L"), s, v)).convert("RGB")
    im = ImageEnhance.Brightness(im).enhance(1.25)
    grey = np.asarray(im.convert("L"))
    t = torch.from_numpy(np.stack([grey] * 3)).to(torch.float32).div(255)
    ref = t.sub_(torch.tensor(P.MEAN).view(3, 1, 1)).div_(torch.tensor(P.STD).view(3, 1, 1)).numpy()
    ops = [("saturation", 1.2), ("contrast", 0.75), ("hue", 240), ("brightness", 1.25)]
    assert np.array_equal(R.augment(img, box, True, ops, True, 48), ref)


# ---------------------------------------------------------------------------------------------------------------
# 2. the planner

SIZES = [(640, 480), (375, 500), (224, 224), (100, 80), (33, 70), (1024, 683)]


def _aug(**kw):
    from clip_event_amd.preprocess import Augment
    return Augment(**kw)


def test_augment_exists_with_open_clips_defaults():
    a = _aug()
    assert (a.n_px, a.scale, a.ratio, a.hflip, a.color_jitter, a.color_jitter_prob, a.gray_scale_prob) == \
        (224, (0.9, 1.0), (3 / 4, 4 / 3), 0.0, None, 0.8, 0.0)
    boxes, flips, ops, greys = a.plan(SIZES, draw=0)
    assert not any(flips) and not any(greys) and all(o == [] for o in ops) and len(boxes) == len(SIZES)


@pytest.mark.parametrize("scale,ratio", [((0.9, 1.0), (3 / 4, 4 / 3)), ((0.08, 1.0), (3 / 4, 4 / 3)), ((0.5, 0.5), (1.0, 1.0))])
def test_boxes_lie_inside_and_respect_scale_and_ratio(scale, ratio):
    a = _aug(scale=scale, ratio=ratio, seed=3)
    accepted = 0
    for draw in range(40):
        boxes, *_ = a.plan(SIZES, draw)
        for (W, H), (x0, y0, x1, y1), i in zip(SIZES, boxes, range(len(SIZES))):
            assert 0 <= x0 < x1 <= W and 0 <= y0 < y1 <= H
            w, h = x1 - x0, y1 - y0
            if R.plan_one(a._base_seed, draw, i, W, H, scale, ratio)[4]:
                continue                                    # no try fitted: the clamped centre crop, checked below
            accepted += 1
            # w = round(sqrt(area * aspect)), h = round(sqrt(area / aspect)): each side is within 1/2 of its real value
            assert (w - 0.5) / (h + 0.5) <= ratio[1] and (w + 0.5) / (h - 0.5) >= ratio[0]
            assert (w - 0.5) * (h - 0.5) <= scale[1] * W * H and (w + 0.5) * (h + 0.5) >= scale[0] * W * H
    assert accepted > 100


def test_fallback_for_a_ten_to_one_image():
    a = _aug(seed=1)
    for draw in range(8):
        (box,), *_ = a.plan([(1000, 100)], draw)
        assert box == (433, 0, 566, 100)                    # h = H, w = round(100 * 4/3) = 133, centred
        (box,), *_ = a.plan([(100, 1000)], draw)
        assert box == (0, 433, 100, 566)                    # w = W, h = round(100 / (3/4)) = 133
        assert R.plan_one(a._base_seed, draw, 0, 1000, 100)[4]


def test_plan_equals_its_restatement():
    kw = dict(scale=(0.3, 1.0), hflip=0.5, color_jitter=JITTER, gray_scale_prob=0.2, seed=11, rank=2)
    a = _aug(**kw)
    for draw in (0, 1, 77, 2 ** 31 + 5):
        boxes, flips, ops, greys = a.plan(SIZES, draw, sample0=5)
        for i, (W, H) in enumerate(SIZES):
            box, flip, op, grey, _ = R.plan_one(a._base_seed, draw, 5 + i, W, H, kw["scale"], (3 / 4, 4 / 3), 0.5, JITTER, 0.8, 0.2)
            assert (boxes[i], flips[i], ops[i], greys[i]) == (box, flip, op, grey)


def test_replay_slicing_draws_and_ranks():
    kw = dict(scale=(0.3, 1.0), hflip=0.5, color_jitter=JITTER, gray_scale_prob=0.2, seed=7)
    a, b = _aug(**kw), _aug(**kw)
    sizes = SIZES * 3
    p = a.plan(sizes, draw=5)
    assert p == b.plan(sizes, draw=5) == a.plan(sizes, draw=5)                          # replay
    for k in (1, 4, 17):
        assert tuple(x[k:] for x in p) == a.plan(sizes[k:], draw=5, sample0=k)          # rows k.. = plan at sample0 = k
    assert p != a.plan(sizes, draw=6) and p[0] != a.plan(sizes, draw=6)[0]
    assert p != _aug(rank=1, **kw).plan(sizes, draw=5)
    assert p != _aug(**{**kw, "seed": 8}).plan(sizes, draw=5)


def test_draw_counter_and_state_dict():
    a = _aug(seed=2)
    assert a.draw == 0 and a.state_dict() == {"draw": 0}
    a.load_state_dict({"draw": 41})
    assert a.draw == 41 and _aug(seed=2).plan(SIZES, 41) == a.plan(SIZES, a.draw)


def test_salt_differs_from_patch_dropouts():
    from clip_event_amd import preprocess
    assert preprocess.AUG_SALT == R.SALT and preprocess.AUG_SALT != 0x9E3779B9


def test_factors_frequencies_and_orders():
    n = 4096
    a = _aug(hflip=0.5, color_jitter=(0.4, 0.4, 0.4, 0.1), color_jitter_prob=0.8, gray_scale_prob=0.2, seed=5)
    _, flips, ops, greys = a.plan([(64, 48)] * n, draw=3)
    for p, hits in ((0.5, sum(flips)), (0.8, sum(1 for o in ops if o)), (0.2, sum(greys))):
        assert abs(hits / n - p) <= 4 * math.sqrt(p * (1 - p) / n), (p, hits / n)
    orders = set()
    for o in ops:
        if not o:
            continue
        assert sorted(name for name, _ in o) == sorted(R.OPS)
        orders.add(tuple(name for name, _ in o if name != "hue"))
        for name, v in o:
            if name == "hue":
                assert isinstance(v, int) and (0 <= v <= int(0.1 * 255) or 256 - int(0.1 * 255) <= v <= 255)
            else:
                assert np.float32(0.6) <= np.float32(v) <= np.float32(1.4) and np.float32(v) == v
    assert len(orders) == 6                                                             # all six orders of three ops
    b = _aug(color_jitter=(1.5, 0.0, 0.2, 0.0), color_jitter_prob=1.0)
    _, _, ops, _ = b.plan([(64, 48)] * 512, draw=0)
    assert all(sorted(name for name, _ in o) == ["brightness", "saturation"] for o in ops)     # zero settings are left out
    assert min(v for o in ops for name, v in o if name == "brightness") >= 0.0                 # U[max(0, 1 - 1.5), 2.5]
    assert max(v for o in ops for name, v in o if name == "brightness") > 1.5


@pytest.mark.parametrize("kw", [dict(n_px=0), dict(n_px=2897), dict(scale=(0.0, 1.0)), dict(scale=(1.0, 0.5)), dict(ratio=(2.0, 1.0)),
                                dict(hflip=1.5), dict(color_jitter_prob=-0.1), dict(gray_scale_prob=2), dict(color_jitter=(0.1, 0.1, 0.1)),
                                dict(color_jitter=(0.1, 0.1, 0.1, 0.6)), dict(color_jitter=(-0.1, 0.1, 0.1, 0.1))])
def test_bad_settings_raise(kw):
    with pytest.raises(ValueError, match="Augment"):
        _aug(**kw)


def test_op_list_errors_raise():
    from clip_event_amd.preprocess import _op_list
    assert _op_list([("hue", 128), ("contrast", 0.5)]) == [(3, 128.0), (1, 0.5)] and _op_list(None) == []
    with pytest.raises(ValueError, match="at most 4"):
        _op_list([("brightness", 1.0)] * 5)
    with pytest.raises(ValueError, match="contrast listed twice"):
        _op_list([("contrast", 1.0), ("hue", 3), ("contrast", 0.5)])
    with pytest.raises(ValueError, match="negative factor"):
        _op_list([("saturation", -0.5)])
    with pytest.raises(ValueError, match="unknown op"):
        _op_list([("sharpness", 1.0)])
    with pytest.raises(ValueError, match="hue shift"):
        _op_list([("hue", 0.25)])


# ---------------------------------------------------------------------------------------------------------------
# 3. the entry point's own argument checks (they return before any launch: no GPU is touched)


def test_library_rejects_bad_op_lists_and_sizes():
    import ctypes
    from clip_event_amd._lib import lib
    from clip_event_amd.preprocess import _AugDesc, _Desc
    cl = lib()
    descs, augs, buf = (_Desc * 2)(), (_AugDesc * 2)(), (ctypes.c_float * 8)()
    host = lambda x: ctypes.addressof(x)

    def call(n_px=32):
        return cl.ce_augment(host(descs), host(augs), host(augs), 2, n_px, 5, 32, host(buf), host(buf), buf, buf, None)

    augs[1].n_ops, augs[1].op[0], augs[1].op[1], augs[1].op[2] = 3, 1, 0, 1
    augs[1].factor[0] = augs[1].factor[1] = augs[1].factor[2] = 1.0
    assert call() == -22 and b"contrast 2 times" in cl.ce_last_error()
    augs[1].op[2] = 2
    assert call(2897) == -22 and b"2896" in cl.ce_last_error()
    augs[1].factor[1] = -0.5
    assert call() == -22 and b"negative factor" in cl.ce_last_error()
    augs[1].factor[1], augs[1].n_ops = 1.0, 5
    assert call() == -22 and b"5 ops" in cl.ce_last_error()
    augs[1].n_ops, augs[0].flip = 3, 2
    assert call() == -22 and b"flip" in cl.ce_last_error()
    assert ctypes.sizeof(_AugDesc) == 44
    table = cl.ce_preprocess_table_bytes(3, 32, 5)
    up = lambda v: (v + 255) // 256 * 256
    assert cl.ce_augment_workspace_bytes(3, 32, 5, 1000) == up(table) + up(12) + up(3 * 32 * 32 * 3) + up(1000)
    assert cl.ce_augment_workspace_bytes(0, 32, 5, 1000) == 0
