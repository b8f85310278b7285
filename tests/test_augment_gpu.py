"""Training augmentation, GPU: ``preprocess.augment`` (ce_augment) against the numpy restatement of Pillow
(tests/augment_ref.py, itself pinned to Pillow by tests/test_augment_cpu.py): identical fp32 bits."""
import numpy as np
import pytest
import torch

from oracle import preprocess_oracle as P
from tests import augment_ref as R

pytestmark = pytest.mark.gpu

SOURCES = {"a": (50, 40), "b": (33, 70), "c": (32, 32), "d": (17, 23), "e": (100, 80), "k": (24, 20)}
ALL4 = [("brightness", 1.25), ("contrast", 0.7), ("saturation", 1.4), ("hue", 20)]
# (source, box, flip, ops, grey): every output a different op list
CASES = [
    ("a", (3, 5, 47, 38), False, [], False),
    ("a", (0, 0, 50, 40), True, [], False),                                        # shares its source with the one above
    ("b", (0, 10, 33, 60), False, [("brightness", 0.6)], False),
    ("b", (1, 0, 32, 70), True, [("brightness", 1.0)], False),
    ("e", (10, 0, 100, 71), False, [("brightness", 1.7)], False),                  # clips at 255
    ("c", (0, 0, 32, 32), True, [("contrast", 0.5)], False),
    ("c", (0, 0, 32, 32), False, [("contrast", 1.0)], False),
    ("e", (0, 9, 90, 80), True, [("contrast", 1.8)], False),                       # clips at both ends
    ("a", (5, 0, 45, 40), False, [("saturation", 0.3)], False),
    ("a", (5, 0, 45, 40), True, [("saturation", 1.0)], False),
    ("e", (20, 10, 80, 70), False, [("saturation", 2.5)], False),
    ("d", (2, 3, 15, 20), False, [("hue", 1)], False),                             # a box smaller than n_px: upsampled
    ("d", (0, 0, 17, 23), True, [("hue", 128)], False),
    ("e", (0, 0, 100, 80), False, [("hue", 255)], False),
    ("b", (0, 20, 33, 64), False, [("brightness", 1.5), ("contrast", 0.6)], False),
    ("b", (0, 20, 33, 64), False, [("contrast", 0.6), ("brightness", 1.5)], False),
    ("e", (7, 3, 97, 75), True, ALL4, False),
    ("e", (7, 3, 97, 75), False, [ALL4[3], ALL4[2], ALL4[1], ALL4[0]], False),
    ("k", (0, 0, 24, 20), False, [("contrast", 0.0)], False),                      # constant image: its mean everywhere
    ("a", (0, 2, 48, 40), True, [("saturation", 1.3), ("hue", 240)], True),        # greyscale after jitter
    ("d", (1, 1, 16, 22), False, [], True),
]


def _img(name):
    w, h = SOURCES[name]
    if name == "k":
        return np.broadcast_to(np.array([200, 90, 31], dtype=np.uint8), (h, w, 3)).copy()
    rng = np.random.default_rng(w * 131 + h)
    base = rng.integers(0, 256, size=(h // 8 + 2, w // 8 + 2, 3), dtype=np.uint8)
    img = np.kron(base, np.ones((8, 8, 1), dtype=np.uint8))[:h, :w]
    return np.clip(img.astype(np.int32) + rng.integers(-20, 21, size=img.shape), 0, 255).astype(np.uint8)


@pytest.fixture(scope="module")
def sources():
    host = {name: _img(name) for name in SOURCES}
    return host, {name: torch.from_numpy(a).to("cuda:0") for name, a in host.items()}


def _run(sources, cases, n_px):
    from clip_event_amd.preprocess import augment
    _, dev = sources
    out = augment([dev[c[0]] for c in cases], [c[1] for c in cases], [c[2] for c in cases], [c[3] for c in cases],
                  [c[4] for c in cases], n_px=n_px)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("n_px", [32, 33])
def test_ragged_batch_matches_reference_bit_for_bit(sources, n_px):
    """21 outputs over six sources; n_px = 33 has a middle column the flip maps to itself."""
    host, _ = sources
    refs = [R.augment(host[s], box, flip, ops, grey, n_px) for (s, box, flip, ops, grey) in CASES]
    assert not np.array_equal(refs[14], refs[15])           # the contrast mean is taken after the ops before it
    got = _run(sources, CASES, n_px)
    assert got.shape == (len(CASES), 3, n_px, n_px) and got.dtype == np.float32
    for i, ref in enumerate(refs):
        assert np.array_equal(got[i], ref), (i, CASES[i], int((got[i] != ref).sum()), float(np.abs(got[i] - ref).max()))
    again = _run(sources, CASES, n_px)                      # the luma sums are zeroed by the call itself
    assert np.array_equal(got, again)


def test_contrast_mean_is_assembled_across_workgroups():
    """n_px = 224: 196 workgroups per image add to one sum; contrast second in the list; one output without contrast."""
    from clip_event_amd.preprocess import augment
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, size=(260, 300, 3), dtype=np.uint8)
    img[:, :150] //= 3                                      # a mean luma far from 128 and an uneven image
    ops = [("brightness", 1.3), ("contrast", 0.6), ("saturation", 1.2)]
    dev = torch.from_numpy(img).to("cuda:0")
    out = augment([dev, dev], [(20, 10, 290, 250), (0, 0, 300, 260)], [True, False], [ops, [("hue", 77)]], None, n_px=224)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.array_equal(got[0], R.augment(img, (20, 10, 290, 250), True, ops, False, 224))
    assert np.array_equal(got[1], R.augment(img, (0, 0, 300, 260), False, [("hue", 77)], False, 224))


def test_colour_lattice_through_hue_and_saturation():
    """A 64 x 64 x 64 lattice of the colour cube (grey axis, ties of the maximum, 0 and 255 included) as a 512 x 512 image,
    taken at its own size (the resampling is the identity), so that every lattice colour reaches the HSV and blend code."""
    from clip_event_amd.preprocess import augment
    lv = np.rint(np.linspace(0, 255, 64)).astype(np.uint8)
    r, g, b = np.meshgrid(lv, lv, lv, indexing="ij")
    img = np.stack([r, g, b], axis=-1).reshape(512, 512, 3)
    lists = [[("hue", 0)], [("hue", 85)], [("hue", 200), ("saturation", 1.6)], [("saturation", 0.45), ("hue", 131)]]
    dev = torch.from_numpy(img).to("cuda:0")
    out = augment([dev] * len(lists), [(0, 0, 512, 512)] * len(lists), None, lists, None, n_px=512)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    for i, ops in enumerate(lists):
        ref = R.augment(img, (0, 0, 512, 512), False, ops, False, 512)
        assert np.array_equal(got[i], ref), (ops, int((got[i] != ref).sum()))


def test_whole_square_image_without_ops_equals_preprocess():
    from clip_event_amd.preprocess import augment, preprocess
    rng = np.random.default_rng(2)
    sq = torch.from_numpy(rng.integers(0, 256, size=(64, 64, 3), dtype=np.uint8)).to("cuda:0")
    for n_px in (32, 64, 33):
        a, b = augment([sq], [(0, 0, 64, 64)], n_px=n_px), preprocess([sq], n_px=n_px)
        assert torch.equal(a, b), n_px


def test_augment_object_runs_its_own_plan_and_replays(sources):
    from clip_event_amd.preprocess import Augment, augment
    host, dev = sources
    names = ["a", "b", "c", "d", "e", "e", "a"]
    images = [dev[n] for n in names]
    aug = Augment(33, scale=(0.3, 1.0), hflip=0.5, color_jitter=(0.4, 0.4, 0.4, 0.1), gray_scale_prob=0.2, seed=3, rank=1)
    plan = aug.plan([SOURCES[n] for n in names], draw=6)
    assert any(plan[1]) and any(plan[2])
    x = aug(images, draw=6)
    assert torch.equal(x, augment(images, *plan, n_px=33))
    for i, n in enumerate(names):
        assert np.array_equal(x[i].cpu().numpy(), R.augment(host[n], plan[0][i], plan[1][i], plan[2][i], plan[3][i], 33)), i
    assert torch.equal(x, aug(images, draw=6)) and not torch.equal(x, aug(images, draw=7))
    assert torch.equal(x[3:], aug(images[3:], draw=6, sample0=3))
    aug.load_state_dict({"draw": 6})
    assert torch.equal(x, aug(images)) and aug.draw == 7 and torch.equal(aug(images), aug(images, draw=7))


def test_augment_rejects_bad_input(sources):
    from clip_event_amd.preprocess import augment
    _, dev = sources
    a = dev["a"]
    with pytest.raises(ValueError, match="not inside"):
        augment([a], [(0, 0, 51, 40)])
    with pytest.raises(ValueError, match="at most 4"):
        augment([a], [(0, 0, 50, 40)], ops=[[("brightness", 1.0)] * 5])
    with pytest.raises(ValueError, match="contrast listed twice"):
        augment([a], [(0, 0, 50, 40)], ops=[[("contrast", 1.0), ("contrast", 1.1)]])
    with pytest.raises(ValueError, match="negative factor"):
        augment([a], [(0, 0, 50, 40)], ops=[[("saturation", -1.0)]])
    with pytest.raises(ValueError, match="2 boxes for 1 images"):
        augment([a], [(0, 0, 50, 40)] * 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        augment([a.cpu()], [(0, 0, 50, 40)])
    with pytest.raises(ValueError, match="uint8"):
        augment([a.float()], [(0, 0, 50, 40)])
