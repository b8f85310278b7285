"""Patch dropout without a GPU: statistics of the counter-based sampler (the numpy restatement of the hash that
tests/test_patch_dropout_ops.py holds ``ce_patch_keep`` to), the per-rank seed, the keep-count rule and the argument checks
that run before anything touches the device."""
import numpy as np
import pytest
import torch

from tests import patch_dropout_ref as R

CASES = [(49, 24), (36, 18), (576, 288), (196, 49)]


@pytest.mark.parametrize("N,keep", CASES)
def test_every_patch_is_kept_at_the_nominal_rate(N, keep):
    """Over draws 0..63 x samples 0..63 (n = 4096 keep sets) per seed, every patch's kept frequency lies within
    5 sqrt(q (1 - q) / n) of q = keep / N: five standard deviations of a binomial frequency."""
    q, n = keep / N, 64 * 64
    bound = 5.0 * np.sqrt(q * (1.0 - q) / n)
    for seed in (0, 1, 12345):
        sets = R.keep_sets(seed, range(64), range(64), N, keep).reshape(n, keep)
        assert (np.diff(sets, axis=1) > 0).all() and sets.min() >= 0 and sets.max() < N
        freq = np.bincount(sets.reshape(-1), minlength=N) / n
        dev = np.abs(freq - q).max()
        print(f"N={N} keep={keep} seed={seed}: largest deviation {dev:.4f} = {dev / (bound / 5):.2f} sigma (bound {bound:.4f})")
        assert dev <= bound


@pytest.mark.parametrize("N,keep", CASES)
def test_samples_and_draws_get_different_sets(N, keep):
    sets = R.keep_sets(0, [0, 1], range(256), N, keep)
    d0 = {tuple(r) for r in sets[0]}
    d1 = {tuple(r) for r in sets[1]}
    assert len(d0) == 256 and len(d1) == 256          # samples 0..255: pairwise different
    assert not (d0 & d1)                              # draw 0 and draw 1 share none


def test_keep_tables_are_consistent():
    idx, inv = R.keep_tables(7, 3, 100, 5, 36, 18)
    for b in range(5):
        assert (inv[b] >= 0).sum() == 18
        assert (inv[b, idx[b]] == np.arange(18)).all()
    # sample0 shifts the sample index: rows 2.. of a pass at 100 are rows 0.. of a pass at 102
    assert (R.keep_tables(7, 3, 102, 3, 36, 18)[0] == idx[2:]).all()


def test_patch_keep_seed():
    from clip_event_amd.functional import patch_keep_seed
    assert patch_keep_seed(5, 0) == 5
    for seed in (0, 1, 12345, 2 ** 32 - 1):
        for rank in range(8):
            assert patch_keep_seed(seed, rank) == (seed + rank * 0x632BE5AB) % 2 ** 32
    assert len({patch_keep_seed(0, r) for r in range(64)}) == 64


def _model():
    from clip_event_amd.model import CLIP
    return CLIP(128, 96, 2, 128, 16, 20, 512, 128, 2, 2)


def test_keep_count_rule():
    m = _model()
    assert m.visual.patch_dropout == 0.0 and m.patch_draw == 0 and not m.drops_patches()
    for p, want in ((0.0, 36), (0.25, 27), (0.5, 18), (0.75, 9), (0.99, 1)):
        m.set_patch_dropout(p, seed=3)
        assert m.visual.patch_dropout == p and m.patch_seed == 3
        assert m.visual.patch_keep() == want == max(1, int(36 * (1 - p)))
    m.train()
    assert m.drops_patches()
    with m.no_patch_dropout():
        assert not m.drops_patches()
    m.eval()
    assert not m.drops_patches()


@pytest.mark.parametrize("p", [-0.1, 1.0, 1.5, float("nan")])
def test_rate_outside_range_raises(p):
    m = _model()
    with pytest.raises(ValueError):
        m.set_patch_dropout(p)
    assert m.visual.patch_dropout == 0.0


def test_draw_counter_and_pin():
    m = _model()
    assert m.next_patch_draw() == (0, 0) and m.patch_draw == 1
    with m.pinned_patch_draw(9, sample0=4):
        assert m.next_patch_draw() == (9, 4) and m.next_patch_draw() == (9, 4)
        with m.pinned_patch_draw(2):
            assert m.next_patch_draw() == (2, 0)
        assert m.next_patch_draw() == (9, 4)
    assert m.patch_draw == 1 and m.next_patch_draw() == (1, 0)


def test_state_stays_out_of_the_state_dict():
    m = _model()
    keys = set(m.state_dict())
    m.set_patch_dropout(0.5, seed=11)
    m.next_patch_draw()
    assert set(m.state_dict()) == keys and not any("patch_d" in k or "patch_seed" in k for k in keys)


@pytest.mark.parametrize("bad", [
    [[0, 1, 2]],                                      # one row for two images
    [[0, 1, 2], [0, 1]],                              # ragged
    [[0, 2, 1], [0, 1, 2]],                           # not ascending
    [[0, 1, 1], [0, 1, 2]],                           # repeated
    [[0, 1, 36], [0, 1, 2]],                          # out of range
    [[-1, 1, 2], [0, 1, 2]],
    [[0.0, 1.0, 2.0], [0.0, 1.0, 2.0]],               # not integers
    [0, 1, 2],                                        # not [B, keep]
    [[], []],                                         # nothing kept
])
def test_malformed_host_keep_idx_raises(bad):
    m = _model()
    img = torch.zeros(2, 3, 96, 96)
    with pytest.raises(ValueError):
        m.encode_image(img, keep_idx=bad)
    with pytest.raises(ValueError):
        m.encode_both(img, torch.zeros(2, 20, dtype=torch.long), keep_idx=bad)


def test_host_keep_idx_forms():
    m = _model()
    good = [[0, 5, 35], [1, 2, 3]]
    for form in (good, np.asarray(good), torch.tensor(good), torch.tensor(good, dtype=torch.int32)):
        out = m._check_keep_idx(form, 2, False)
        assert out.dtype == np.int32 and out.tolist() == good


def test_keep_idx_with_grid_raises():
    m = _model()
    img = torch.zeros(2, 3, 96, 96)
    with pytest.raises(ValueError):
        m.encode_image(img, use_grid=True, keep_idx=[[0, 1], [2, 3]])
    with pytest.raises(ValueError):
        m.encode_both(img, torch.zeros(2, 20, dtype=torch.long), use_grid=True, keep_idx=[[0, 1], [2, 3]])
