"""The positional-table resampling at the op level (csrc/posembed.hip: ``ce_pos_resample_fwd`` / ``ce_pos_resample_bwd``) against
the fp64 product with the SAME fp32 tables, element by element, under the summation bound tests/image_size_ref.py states --
nothing is measured.  NaN sentinels stand before and after every buffer, operands included; every overwritten output starts as
NaN.  A CPU test runs the checker on an fp32 emulation of the kernels' summation order and on corrupted results."""
import numpy as np
import pytest
import torch

from tests import image_size_ref as R

DEV = "cuda:0"
GRIDS = [(6, 4), (6, 10), (6, 12), (7, 14), (1, 3), (3, 1), (63, 2)]
DIMS = (4, 128, 768)
PAD = 64                      # floats of sentinel on either side: the guarded view stays 16-byte aligned
EINVAL = -22


def _values(g_in, g_out, D, seed):
    rng = np.random.default_rng(seed)
    pos = rng.standard_normal((g_in * g_in + 1, D)).astype(np.float32)
    dout = rng.standard_normal((g_out * g_out + 1, D)).astype(np.float32)
    base = rng.standard_normal((g_in * g_in + 1, D)).astype(np.float32)
    return pos, dout, base


def _within(got, ref, bound):
    """(elements over their bound, worst |err| / bound over the elements with a non-zero bound; exact where the bound is 0)."""
    err = np.abs(got.astype(np.float64) - ref)
    over = int((err > bound).sum())
    nz = bound > 0
    return over, float((err[nz] / bound[nz]).max()) if nz.any() else 0.0


# ---- CPU: the checker ---------------------------------------------------------------------------------------------------------

def _emulate_fwd(pos, w32):
    """fp32, both sums ascending, zero taps skipped, no fused multiply-add."""
    g_out, g_in = w32.shape
    out = np.empty((g_out * g_out + 1, pos.shape[1]), np.float32)
    out[0] = pos[0]
    for i in range(g_out):
        for j in range(g_out):
            acc = np.zeros(pos.shape[1], np.float32)
            for a in np.flatnonzero(w32[i]):
                inner = np.zeros(pos.shape[1], np.float32)
                for b in np.flatnonzero(w32[j]):
                    inner = inner + w32[j, b] * pos[1 + a * g_in + b]
                acc = acc + w32[i, a] * inner
            out[1 + i * g_out + j] = acc
    return out


@pytest.mark.parametrize("g_in,g_out", [(6, 4), (6, 10), (7, 14), (1, 3), (3, 1)])
def test_checker_passes_an_fp32_emulation_and_flags_corruptions(g_in, g_out):
    D = 8
    pos, _, _ = _values(g_in, g_out, D, 1)
    w32 = R.weights(g_in, g_out).astype(np.float32)
    w = w32.astype(np.float64)
    ref, bound = R.forward(pos, w), R.forward_bound(pos, w)
    out = _emulate_fwd(pos, w32)
    over, worst = _within(out, ref, bound)
    print(f"{g_in} -> {g_out}: emulation worst |err| / bound {worst:.3f}")
    assert over == 0 and worst < 1.0
    assert np.array_equal(out[0], pos[0]) and float(bound[0].max()) == 0.0
    if g_in > 1 and g_out > 1:                          # (one output cell reads the grid symmetrically)
        grid = pos[1:].astype(np.float64).reshape(g_in, g_in, D)                   # the input grid read transposed
        swapped = np.concatenate([pos[:1].astype(np.float64), np.einsum("ia,jb,bad->ijd", w, w, grid).reshape(g_out * g_out, D)])
        assert _within(swapped.astype(np.float32), ref, bound)[0] > 0
    unnormalised = R.forward(pos, w * (1 + 2.0 ** -12))                            # tables a little off
    assert _within(unnormalised.astype(np.float32), ref, bound)[0] > 0
    bad = out.copy()
    bad[0, 0] = np.nextafter(bad[0, 0], np.float32(np.inf))                        # the class row is a copy: one ulp is flagged
    assert _within(bad, ref, bound)[0] == 1


# ---- GPU ----------------------------------------------------------------------------------------------------------------------

class Guarded:
    """A device fp32 buffer between two NaN sentinels."""

    def __init__(self, values=None, shape=None):
        shape = values.shape if values is not None else shape
        n = int(np.prod(shape))
        self.raw = torch.full((n + 2 * PAD,), float("nan"), dtype=torch.float32, device=DEV)
        self.view = self.raw[PAD: PAD + n].view(*shape)
        if values is not None:
            self.view.copy_(torch.from_numpy(np.ascontiguousarray(values)))

    def intact(self):
        return bool(torch.isnan(self.raw[:PAD]).all() and torch.isnan(self.raw[-PAD:]).all())

    def numpy(self):
        return self.view.detach().cpu().numpy().copy()


def _fwd(pos, g_in, w, out, g_out, D):
    from clip_event_amd._lib import lib, ptr, stream
    return lib().ce_pos_resample_fwd(ptr(pos), g_in, ptr(w), ptr(w), ptr(out), g_out, D, stream())


def _bwd(dout, g_out, w, dpos, g_in, D, accumulate):
    from clip_event_amd._lib import lib, ptr, stream
    return lib().ce_pos_resample_bwd(ptr(dout), g_out, ptr(w), ptr(w), ptr(dpos), g_in, D, accumulate, stream())


@pytest.mark.gpu
@pytest.mark.parametrize("g_in,g_out", GRIDS)
def test_resample_against_fp64_element_by_element(g_in, g_out):
    for D in DIMS:
        pos, dout, base = _values(g_in, g_out, D, 100 * g_in + g_out)
        w32 = R.weights(g_in, g_out).astype(np.float32)
        w = w32.astype(np.float64)
        d_pos, d_dout, d_w = Guarded(pos), Guarded(dout), Guarded(w32)
        # forward, twice, into NaN-filled outputs
        outs = [Guarded(shape=(g_out * g_out + 1, D)) for _ in range(2)]
        for o in outs:
            assert _fwd(d_pos.view, g_in, d_w.view, o.view, g_out, D) == 0
        torch.cuda.synchronize()
        out = outs[0].numpy()
        assert np.array_equal(out.view(np.int32), outs[1].numpy().view(np.int32))
        f_bound = R.forward_bound(pos, w)
        over, worst_f = _within(out, R.forward(pos, w), f_bound)
        assert over == 0 and np.array_equal(out[0], pos[0]), (D, over, worst_f)
        # backward: accumulate = 0 overwrites NaN (twice: the same bits), accumulate = 1 adds to known values
        stores = [Guarded(shape=(g_in * g_in + 1, D)) for _ in range(2)]
        for o in stores:
            assert _bwd(d_dout.view, g_out, d_w.view, o.view, g_in, D, 0) == 0
        added = Guarded(base)
        assert _bwd(d_dout.view, g_out, d_w.view, added.view, g_in, D, 1) == 0
        torch.cuda.synchronize()
        dpos = stores[0].numpy()
        assert np.array_equal(dpos.view(np.int32), stores[1].numpy().view(np.int32))
        ref_b, b_bound = R.backward(dout, w), R.backward_bound(dout, w)
        over, worst_b = _within(dpos, ref_b, b_bound)
        assert over == 0 and np.array_equal(dpos[0], dout[0]), (D, over, worst_b)
        over, worst_a = _within(added.numpy(), base.astype(np.float64) + ref_b, R.backward_bound(dout, w, base))
        assert over == 0, (D, over, worst_a)
        # the adjoint identity on the outputs, in fp64: <R x, y> = <x, R^T y> within the two bounds
        lhs = float((out.astype(np.float64) * dout).sum())
        rhs = float((pos.astype(np.float64) * dpos).sum())
        slack = float((f_bound * np.abs(dout)).sum() + (b_bound * np.abs(pos)).sum())
        assert abs(lhs - rhs) <= slack, (D, lhs, rhs, slack)
        for buf in [d_pos, d_dout, d_w, added] + outs + stores:
            assert buf.intact()
        assert np.array_equal(d_pos.numpy(), pos) and np.array_equal(d_dout.numpy(), dout) and np.array_equal(d_w.numpy(), w32)
        print(f"{g_in} -> {g_out}, D = {D}: worst |err| / bound forward {worst_f:.3f}, backward {worst_b:.3f}, accumulated "
              f"{worst_a:.3f}; adjoint |lhs - rhs| / slack {abs(lhs - rhs) / slack:.3f}")


@pytest.mark.gpu
def test_equal_grids_copy_the_table_bit_for_bit():
    g, D = 7, 128
    pos, dout, _ = _values(g, g, D, 5)
    w = Guarded(np.eye(g, dtype=np.float32))
    d_pos, d_dout, out, dpos = Guarded(pos), Guarded(dout), Guarded(shape=pos.shape), Guarded(shape=pos.shape)
    assert _fwd(d_pos.view, g, w.view, out.view, g, D) == 0
    assert _bwd(d_dout.view, g, w.view, dpos.view, g, D, 0) == 0
    torch.cuda.synchronize()
    assert np.array_equal(out.numpy(), pos) and np.array_equal(dpos.numpy(), dout)


@pytest.mark.gpu
def test_python_ops_use_the_cached_fp32_tables():
    from clip_event_amd import posembed
    g_in, g_out, D = 6, 10, 128
    pos, dout, base = _values(g_in, g_out, D, 9)
    w = R.tables32(g_in, g_out)
    t = torch.from_numpy(pos).to(DEV)
    out = posembed.resample(t, g_out)
    assert tuple(out.shape) == (g_out * g_out + 1, D)
    assert _within(out.cpu().numpy(), R.forward(pos, w), R.forward_bound(pos, w))[0] == 0
    d = torch.from_numpy(dout).to(DEV)
    stored = posembed.resample_backward(d, g_in)
    assert _within(stored.cpu().numpy(), R.backward(dout, w), R.backward_bound(dout, w))[0] == 0
    acc = torch.from_numpy(base).to(DEV)
    assert posembed.resample_backward(d, g_in, accumulate=True, out=acc) is acc
    assert _within(acc.cpu().numpy(), base.astype(np.float64) + R.backward(dout, w), R.backward_bound(dout, w, base))[0] == 0
    assert posembed.device_tables(g_in, g_out, t.device)[0] is posembed.device_tables(g_in, g_out, t.device)[0]
    with pytest.raises(ValueError, match="accumulate needs"):
        posembed.resample_backward(d, g_in, accumulate=True)
    with pytest.raises(ValueError, match="g\\*g \\+ 1 rows"):
        posembed.resample(t[:-1].contiguous(), g_out)
    # an output the kernel would write past the end of, or into the wrong type, is refused before the call
    for bad in (torch.empty(g_out * g_out, D, device=DEV), torch.empty(g_out * g_out + 1, D - 4, device=DEV),
                torch.empty(g_out * g_out + 1, D, device=DEV, dtype=torch.float16), torch.empty(g_out * g_out + 1, D),
                torch.empty(g_out * g_out + 1, 2 * D, device=DEV)[:, :D]):
        with pytest.raises(ValueError, match="resample: out"):
            posembed.resample(t, g_out, out=bad)
    with pytest.raises(ValueError, match="resample_backward: out"):
        posembed.resample_backward(d, g_in, out=torch.empty(g_in * g_in, D, device=DEV))
    for g in (0, -1, 64):
        with pytest.raises(ValueError, match="1..63"):
            posembed.resample(t, g)
        with pytest.raises(ValueError, match="1..63"):
            posembed.resample_backward(d, g)


@pytest.mark.gpu
def test_bad_arguments_return_einval_and_launch_nothing():
    from clip_event_amd._lib import lib
    g_in, g_out, D = 6, 10, 8
    pos, dout, _ = _values(g_in, g_out, D, 3)
    d_pos, d_dout, w = Guarded(pos), Guarded(dout), Guarded(R.weights(g_in, g_out).astype(np.float32))
    out, dpos = Guarded(shape=(g_out * g_out + 1, D)), Guarded(shape=(g_in * g_in + 1, D))
    off = out.raw[PAD + 1: PAD + 1 + out.view.numel()]                            # 4 bytes off a 16-byte boundary

    def fwd(pos=d_pos.view, g_in=g_in, wy=w.view, wx=w.view, out=out.view, g_out=g_out, D=D):
        from clip_event_amd._lib import ptr, stream
        return lib().ce_pos_resample_fwd(ptr(pos), g_in, ptr(wy), ptr(wx), ptr(out), g_out, D, stream())

    def bwd(dout=d_dout.view, g_out=g_out, wy=w.view, wx=w.view, dpos=dpos.view, g_in=g_in, D=D, accumulate=0):
        from clip_event_amd._lib import ptr, stream
        return lib().ce_pos_resample_bwd(ptr(dout), g_out, ptr(wy), ptr(wx), ptr(dpos), g_in, D, accumulate, stream())

    bad = [dict(g_in=0), dict(g_in=64), dict(g_in=-1), dict(g_out=0), dict(g_out=64), dict(D=0), dict(D=6), dict(D=-4),
           dict(wy=None), dict(wx=None)]
    for kw in bad + [dict(pos=None), dict(out=None), dict(out=off)]:
        assert fwd(**kw) == EINVAL, kw
        assert "ce_pos_resample_fwd" in lib().ce_last_error().decode(), kw
    for kw in bad + [dict(dout=None), dict(dpos=None), dict(dpos=off[: dpos.view.numel()]), dict(accumulate=2), dict(accumulate=-1)]:
        assert bwd(**kw) == EINVAL, kw
        assert "ce_pos_resample_bwd" in lib().ce_last_error().decode(), kw
    torch.cuda.synchronize()
    assert bool(torch.isnan(out.raw).all()) and bool(torch.isnan(dpos.raw).all())     # nothing was launched
    assert fwd() == 0 and bwd() == 0                                                  # and the good call still goes through
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out.view).all()) and bool(torch.isfinite(dpos.view).all()) and out.intact() and dpos.intact()
