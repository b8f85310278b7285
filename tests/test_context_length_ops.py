"""``ce_pos_stretch_fwd`` / ``ce_pos_stretch_bwd`` (the text positional table at another context length) against
``W @ P`` / ``W^T @ dT`` in fp64 with W = ``posembed.text_weights``.

Bounds, per element, u = 2^-24 the fp32 unit roundoff; they are what a kernel that rounds the weights to fp32 and works in fp32
would need.  Forward: a row has at most two terms; each would carry the rounding of its weight (u) and of its product (u), the sum
one more: 3 u (|W| @ |P|) to first order, asserted at 4 u.  A unit row is a copy: bit-exact.  Backward: a column with n_c non-zeros
sums n_c terms in order, each with its weight's rounding (u), the running sum n_c roundings of at most the final magnitude:
(n_c + 1) u to first order, asserted at (n_c + 2) u (|W|^T @ |dT|).  The kernels keep the weights in fp64, work in fp64 and round
once, so they sit near u / 2 of the result; the forward is moreover the fp32 rounding of ``stretch_host``, bit for bit, which is
what lets a model at ``set_context_length(T)`` equal a twin that is native at ``T`` (tests/test_context_length_gpu.py)."""
import numpy as np
import pytest
import torch

from clip_event_amd import posembed

DEV = "cuda:0"
U = 2.0 ** -24
SENTINEL = -2.0 ** 30
GUARD = 8              # floats; keeps the live part 16-byte aligned behind a 32-byte guard
SHAPES = [(77, 248, 20, 128), (77, 32, 20, 64), (20, 50, 8, 64), (77, 78, 76, 64)]


def _guarded(rows, D, fill=None):
    """(flat buffer with GUARD sentinels on either side, its live [rows, D] view)."""
    buf = torch.full((rows * D + 2 * GUARD,), SENTINEL, dtype=torch.float32, device=DEV)
    live = buf[GUARD:GUARD + rows * D].view(rows, D)
    if fill is not None:
        live.copy_(fill)
    return buf, live


def _guards_ok(buf):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all())


def _case(t_in, t_out, keep, D):
    g = torch.Generator().manual_seed(1000 * t_in + t_out + keep)
    P = torch.randn(t_in, D, generator=g)
    dT = torch.randn(t_out, D, generator=g)
    base = torch.randn(t_in, D, generator=g)
    return posembed.text_weights(t_in, t_out, keep), P, dT, base


@pytest.mark.gpu
@pytest.mark.parametrize("t_in,t_out,keep,D", SHAPES)
def test_stretch_forward_against_fp64(t_in, t_out, keep, D):
    W, P, _, _ = _case(t_in, t_out, keep, D)
    pbuf, p = _guarded(t_in, D, P)
    obuf, out = _guarded(t_out, D, torch.full((t_out, D), float("nan")))
    posembed.stretch(p, t_out, keep, out=out)
    first = out.clone()
    posembed.stretch(p, t_out, keep, out=out)
    torch.cuda.synchronize()
    assert torch.equal(first.view(torch.int32), out.view(torch.int32)), "two calls, different bits"
    assert _guards_ok(pbuf) and _guards_ok(obuf) and torch.equal(p.cpu(), P)
    got, ref = out.cpu().double().numpy(), W @ P.double().numpy()
    bound = 4 * U * (np.abs(W) @ P.abs().double().numpy())
    err = np.abs(got - ref)
    print(f"[stretch fwd {t_in}->{t_out} keep {keep}] worst error / bound {np.nanmax(err / np.maximum(bound, 1e-300)):.3f}")
    assert not np.isnan(got).any() and (err <= bound).all()
    unit = np.flatnonzero((W == 1.0).any(axis=1))
    assert unit.size >= min(keep, t_in - 1, t_out)
    src = W[unit].argmax(axis=1)
    assert torch.equal(out.cpu()[unit].view(torch.int32), P[src].view(torch.int32)), "unit rows must be copies"
    host = torch.from_numpy(posembed.stretch_host(P, t_out, keep).astype(np.float32))
    assert torch.equal(out.cpu().view(torch.int32), host.view(torch.int32)), "the table is the fp32 rounding of stretch_host"


@pytest.mark.gpu
@pytest.mark.parametrize("t_in,t_out,keep,D", SHAPES)
@pytest.mark.parametrize("accumulate", (0, 1))
def test_stretch_backward_against_fp64(t_in, t_out, keep, D, accumulate):
    W, _, dT, base = _case(t_in, t_out, keep, D)
    dbuf, d = _guarded(t_out, D, dT)
    start = base if accumulate else torch.full((t_in, D), float("nan"))
    gbuf, grad = _guarded(t_in, D, start)
    posembed.stretch_backward(d, t_in, keep, accumulate=bool(accumulate), out=grad)
    first = grad.clone()
    grad.copy_(start)
    posembed.stretch_backward(d, t_in, keep, accumulate=bool(accumulate), out=grad)
    torch.cuda.synchronize()
    assert torch.equal(first.view(torch.int32), grad.view(torch.int32)), "two calls, different bits"
    assert _guards_ok(dbuf) and _guards_ok(gbuf) and torch.equal(d.cpu(), dT)
    got = grad.cpu().double().numpy()
    ref = W.T @ dT.double().numpy()
    n_c = (W != 0).sum(axis=0)[:, None]
    bound = (n_c + 2) * U * (np.abs(W).T @ dT.abs().double().numpy())
    if accumulate:         # one more fp32 add, onto the base
        ref = ref + base.double().numpy()
        bound = bound + U * np.abs(ref)
    err = np.abs(got - ref)
    print(f"[stretch bwd {t_in}->{t_out} keep {keep} acc {accumulate}] worst error / bound "
          f"{np.nanmax(err / np.maximum(bound, 1e-300)):.3f}")
    assert not np.isnan(got).any() and (err <= bound).all()
    if t_out < t_in and not accumulate:
        assert (got[t_out:] == 0).all()        # truncation: the rows behind the run length get no gradient
