"""Host side of the text tower's context-length switch: the operator ``posembed.text_weights``, its host
application, the permanent form, the argument check, the routing function and the model's attributes.  No GPU."""
import numpy as np
import pytest
import torch

from clip_event_amd import posembed
from clip_event_amd.functional import text_tower_tokens

PAIRS = [(77, 248, 20), (77, 160, 20), (77, 78, 76), (20, 50, 8), (77, 1024, 20), (77, 32, 20), (77, 77, 20), (2, 3, 0), (77, 300, 0)]


@pytest.mark.parametrize("t_in,t_out,keep", PAIRS)
def test_text_weights_rows(t_in, t_out, keep):
    W = posembed.text_weights(t_in, t_out, keep)
    assert W.dtype == np.float64 and W.shape == (t_out, t_in)
    assert np.abs(W.sum(axis=1) - 1.0).max() <= 1e-15
    assert ((W != 0).sum(axis=1) <= 2).all() and (W >= 0).all()
    k = min(keep, t_in - 1, t_out) if t_out > t_in else t_out
    assert np.array_equal(W[:k], np.eye(t_in)[:k])
    # the non-zeros of a row are neighbours and the rows walk the table in order
    first = (W != 0).argmax(axis=1)
    last = t_in - 1 - (W != 0)[:, ::-1].argmax(axis=1)
    assert (last - first <= 1).all() and (np.diff(first) >= 0).all()


def test_shorter_is_truncation_and_keep_is_ignored():
    for keep in (0, 20, 500):
        assert np.array_equal(posembed.text_weights(77, 32, keep), np.eye(77)[:32])
        assert np.array_equal(posembed.text_weights(77, 77, keep), np.eye(77))


def test_77_to_248_keep_20_is_the_four_fold_stretch():
    W = posembed.text_weights(77, 248, 20)
    ref = np.zeros((248, 77))
    ref[:20, :20] = np.eye(20)
    for i in range(57):
        for r in range(4):
            ref[20 + 4 * i + r, 20 + i] += 1 - r / 4
            ref[20 + 4 * i + r, min(21 + i, 76)] += r / 4
    assert np.array_equal(W, ref)


def test_keep_is_clamped_below_the_table_length():
    assert np.array_equal(posembed.text_weights(77, 100, 77), posembed.text_weights(77, 100, 76))
    assert np.array_equal(posembed.text_weights(77, 100, 10 ** 6), posembed.text_weights(77, 100, 76))
    W = posembed.text_weights(77, 100, 76)
    assert np.array_equal(W[:76], np.eye(77)[:76]) and (W[76:, 75] == 0).all()


def test_stretch_host_is_the_matrix_product():
    P = torch.randn(77, 24, generator=torch.Generator().manual_seed(0))
    for t_out, keep in ((248, 20), (32, 20), (78, 76)):
        got = posembed.stretch_host(P, t_out, keep)
        assert got.dtype == np.float64 and got.shape == (t_out, 24)
        W, p = posembed.text_weights(77, t_out, keep), P.double().numpy()
        # two products and a sum per element, in either arithmetic (fused or not): three fp64 roundings of at most |W| @ |P|
        assert (np.abs(got - W @ p) <= 3 * 2.0 ** -53 * (np.abs(W) @ np.abs(p))).all()
        unit = np.flatnonzero((W == 1.0).any(axis=1))
        assert np.array_equal(got[unit], p[W[unit].argmax(axis=1)])


def test_stretch_tables_are_the_operator():
    """The kernels' form (first non-zero, two weights, column spans) reproduces the dense matrix."""
    for t_in, t_out, keep in PAIRS:
        W = posembed.text_weights(t_in, t_out, keep)
        i0, w, span = posembed.stretch_tables(t_in, t_out, keep)
        R = np.zeros_like(W)
        for j in range(t_out):
            R[j, i0[j]] += w[j, 0]
            R[j, min(i0[j] + 1, t_in - 1)] += w[j, 1]
        assert np.array_equal(R, W) and w.dtype == np.float64
        for i in range(t_in):
            assert np.array_equal(np.flatnonzero(W[:, i]), np.arange(span[i, 0], span[i, 1]))


def test_resize_text_state_dict_changes_only_the_table():
    from oracle import clip_oracle as O
    sd = O.init_params(O.ClipConfig(64, 64, 2, 128, 32, 77, 512, 128, 2, 3), 5)
    out = posembed.resize_text_state_dict(sd, 248)
    assert sorted(out) == sorted(sd)
    for k in sd:
        if k != "positional_embedding":
            assert out[k] is sd[k]
    pos = out["positional_embedding"]
    assert tuple(pos.shape) == (248, 128) and pos.dtype == sd["positional_embedding"].dtype
    ref = torch.from_numpy(posembed.stretch_host(sd["positional_embedding"], 248, 20)).to(pos.dtype)
    assert torch.equal(pos, ref) and torch.equal(pos[:20], sd["positional_embedding"][:20])
    assert posembed.resize_text_state_dict(sd, 77)["positional_embedding"] is sd["positional_embedding"]
    assert tuple(sd["positional_embedding"].shape) == (77, 128)


def test_check_context_length():
    assert posembed.check_context_length(2) == 2 and posembed.check_context_length(1024) == 1024
    assert posembed.check_context_length(np.int64(248)) == 248
    for bad in (1, 0, -5, 1025, 77.0, 77.5, "77", None, True):
        with pytest.raises(ValueError):
            posembed.check_context_length(bad)


@pytest.mark.parametrize("run,longest,packed,want", [(77, 77, True, 77), (248, 100, True, 128), (248, 129, True, 248),
                                                     (248, 50, False, 248), (128, 128, True, 128), (248, 128, True, 128),
                                                     (129, 129, True, 129), (32, 10, True, 32)])
def test_text_tower_tokens(run, longest, packed, want):
    assert text_tower_tokens(run, longest, packed) == want


def test_model_attributes_follow_the_switch():
    from oracle import clip_oracle as O
    from clip_event_amd.model import build_model
    cfg = O.ClipConfig(64, 64, 2, 128, 32, 77, 512, 128, 2, 3)
    m = build_model(O.init_params(cfg, 5))
    assert m.context_length == m.native_context_length == 77
    assert m.set_context_length(248) == 248
    assert m.context_length == 248 and m.native_context_length == 77
    sd = m.state_dict()
    assert tuple(sd["positional_embedding"].shape) == (77, 128)
    assert not any("context" in k for k in sd)
    m.train()
    m.eval()
    m.load_state_dict(sd)
    assert m.context_length == 248
    assert m.set_context_length(32, keep=5) == 32 and m.context_length == 32
    for bad in (1, 1025, 77.0):
        with pytest.raises(ValueError):
            m.set_context_length(bad)
    assert m.context_length == 32                                # a refused length changes nothing
    assert m.set_context_length(None) == 77 and m.context_length == 77
    assert m.set_context_length(77) == 77
    long_native = build_model(posembed.resize_text_state_dict(O.init_params(cfg, 5), 248))
    assert long_native.context_length == long_native.native_context_length == 248
