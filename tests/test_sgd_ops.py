"""Op-level checks of clip + SGD with momentum (csrc/optim.hip: ``ce_sgd_step`` / ``ce_sgd_step_tiles``) against an fp64
restatement of the kernel's element function, in the style of tests/test_embed_optim_ops.py (whose helpers are imported):
element-wise bounds from the count of fp32 roundings, bit-equality where a kernel only rounds or moves, and sentinel guard
elements behind every buffer."""
import math
from ctypes import c_float, c_int, c_long, c_void_p

import numpy as np
import pytest
import torch

from tests.test_embed_optim_ops import (DEV, LR, MAX_NORM, TILE_MATS, TILE_N, TILE_SEGS, U, _adam_state, _dev, _lib, _same_bits,
                                        _within)

gpu = pytest.mark.gpu

# hyper-parameters as the kernel receives them (fp32); the references use the same fp32-rounded values
MU, DAMP, WD = (float(np.float32(x)) for x in (0.9, 0.1, 0.1))

# (name, momentum, dampening, nesterov)
VARIANTS = [("plain", MU, 0.0, False), ("nesterov", MU, 0.0, True), ("dampening", MU, DAMP, False), ("momentum0", 0.0, 0.0, False)]
SGD_GRID = [(clip, wd, step, var) for clip in ("active", "inactive", "none") for wd in (0.0, WD) for step in (1, 2) for var in VARIANTS]


def sgd_ref(p, g, buf, sumsq, wd, mu, damp, nesterov, first, lr=LR):
    """fp64 restatement of optim.hip's sgd_elem (torch.optim.SGD behind the clip): g = g coef with coef = min(1, max_norm /
    (sqrt(sumsq) + 1e-6)) (1 without sumsq); g += wd p; with momentum buf = first ? g : mu buf + (1 - damp) g and the update is
    buf (nesterov: g + mu buf), without it g; p -= lr update.  Returns (p, buf, b_mag, u_mag): the sizes of the terms that make
    up the new buffer and the update.  ``buf`` comes back unchanged when mu == 0."""
    p, g, buf = (t.double() for t in (p, g, buf))
    coef = 1.0 if sumsq is None else min(1.0, MAX_NORM / (math.sqrt(sumsq) + 1e-6))
    ge = g * coef + wd * p
    gmag = (g * coef).abs() + wd * p.abs()
    if mu != 0:
        if first:
            buf, b_mag = ge, gmag
        else:
            b_mag = mu * buf.abs() + (1 - damp) * gmag
            buf = mu * buf + (1 - damp) * ge
        upd, u_mag = (ge + mu * buf, gmag + mu * b_mag) if nesterov else (buf, b_mag)
    else:
        upd, b_mag, u_mag = ge, gmag, gmag
    return p - lr * upd, buf, b_mag, u_mag


def _sgd_bounds(ref, lr=LR):
    """Element bounds on (p, buf) of the fp32 kernel against sgd_ref, counted as tests/test_embed_optim_ops._adam_bounds counts:
    the buffer is a handful of fp32 roundings (clip coefficient, scaling, decay, dampening, the multiply-add) of terms of size
    b_mag: 2^-20 of it (16 ulp); p within 2 ulp of p plus 2^-19 of lr u_mag (the update's own relative error)."""
    p, _, b_mag, u_mag = ref
    return 2 * U * p.abs() + 2.0 ** -19 * lr * u_mag, 2.0 ** -20 * b_mag


def _sgd_state(n, step, clip, seed):
    """(p, g, buf, sumsq or None) from the Adam tests' generator: gradient norm 10 x / 0.5 x max_norm; at step 2 a momentum
    buffer like an earlier step's, at step 1 none (zeros here; the GPU tests poison it, the first step must overwrite it)."""
    p, g, m, _, sumsq = _adam_state(n, step, clip, seed)
    return p, g, m, sumsq


def test_sgd_reference_matches_torch():
    """CPU cross-check of the fp64 restatement: torch.nn.utils.clip_grad_norm_ + torch.optim.SGD(foreach=False) on fp32 copies
    land within the kernel's bounds over the whole grid (n = 999).  Measured: worst error / bound 0.49 (p), 0.17 (buf)."""
    worst = {"p": 0.0, "buf": 0.0}
    for clip, wd, step, (name, mu, damp, nesterov) in SGD_GRID:
        p0, g0, b0, sumsq = _sgd_state(999, step, clip, 5)
        param = torch.nn.Parameter(p0.clone())
        param.grad = g0.clone()
        if sumsq is not None:
            torch.nn.utils.clip_grad_norm_([param], MAX_NORM)
        opt = torch.optim.SGD([param], lr=LR, momentum=mu, dampening=damp, weight_decay=wd, nesterov=nesterov, foreach=False)
        if step > 1 and mu != 0:
            opt.state[param] = {"momentum_buffer": b0.clone()}
        opt.step()
        ref = sgd_ref(p0, g0, b0, sumsq, wd, mu, damp, nesterov, first=step == 1)
        bp, bb = _sgd_bounds(ref)
        checks = [("p", param.detach(), ref[0], bp)]
        if mu != 0:
            checks.append(("buf", opt.state[param]["momentum_buffer"], ref[1], bb))
        else:
            assert "momentum_buffer" not in opt.state[param] or opt.state[param]["momentum_buffer"] is None
        for what, got, want, bound in checks:
            err = (got.double() - want).abs()
            ratio = float((err / bound.clamp_min(1e-300)).max())
            worst[what] = max(worst[what], ratio)
            assert bool((err <= bound).all()), (clip, wd, step, name, what, ratio)
    print(f"[sgd_ref vs torch] worst |err| / bound: p {worst['p']:.3f}, buf {worst['buf']:.3f}")


def _call_flat(cl, ptr, stream, p, g, buf, p16, n, ss, wd, mu, damp, nesterov, first):
    return cl.ce_sgd_step(ptr(p), ptr(g), ptr(buf) if buf is not None else c_void_p(0), ptr(p16), c_long(n),
                          ptr(ss) if ss is not None else c_void_p(0), c_float(MAX_NORM), c_float(LR), c_float(mu), c_float(damp),
                          c_float(wd), c_int(int(nesterov)), c_int(int(first)), stream())


def _job_table(mats, p16, wts):
    from clip_event_amd._lib import TransposeJob
    jobs, tiles = (TransposeJob * len(mats))(), 0
    for i, ((off, r, c), wt) in enumerate(zip(mats, wts)):
        jobs[i].src, jobs[i].dst = p16.data_ptr() + 2 * off, wt.data_ptr()
        jobs[i].rows, jobs[i].cols, jobs[i].tile_start = r, c, tiles
        tiles += ((r + 63) // 64) * ((c + 63) // 64)
    return torch.frombuffer(bytearray(bytes(jobs)), dtype=torch.uint8).to(DEV), tiles


def _call_tiles(cl, ptr, stream, p, g, buf, p16, tab, njobs, tiles, seg_tab, ss, wd, mu, damp, nesterov, first):
    return cl.ce_sgd_step_tiles(ptr(p), ptr(g), ptr(buf) if buf is not None else c_void_p(0), ptr(p16),
                                ptr(tab) if tab is not None else c_void_p(0), c_int(njobs), c_int(tiles), ptr(seg_tab),
                                c_int(seg_tab.shape[0]), ptr(ss) if ss is not None else c_void_p(0), c_float(MAX_NORM), c_float(LR),
                                c_float(mu), c_float(damp), c_float(wd), c_int(int(nesterov)), c_int(int(first)), stream())


POISON = 3.0        # content of the momentum buffer before a FIRST step: must be overwritten, never read


@gpu
@pytest.mark.parametrize("n", [7171, 5, 1000003])
def test_sgd_step_against_fp64(n):
    """``ce_sgd_step`` (flat) over the grid clip active / inactive / off (sumsq NULL) x weight decay 0 / 0.1 x step 1 / 2 x
    {plain, nesterov, dampening 0.1, momentum 0 with buf = NULL}, n with n % 4 != 0 and n % 2048 != 0: the momentum buffer and
    the masters element-wise against sgd_ref (_sgd_bounds); the bf16 mirror bit-equal to the masters' RNE cast; the guard
    elements behind every buffer untouched; the gradient not written."""
    cl, ptr, stream = _lib()
    for clip, wd, step, (name, mu, damp, nesterov) in SGD_GRID:
        first = step == 1
        p0, g0, b0, sumsq = _sgd_state(n, step, clip, n + step)
        ref = sgd_ref(p0, g0, b0, sumsq, wd, mu, damp, nesterov, first)
        bstart = torch.full_like(b0, POISON) if first else b0
        p, g, buf = [torch.cat([t, torch.full((6,), 4.0)]).to(DEV) for t in (p0, g0, bstart)]
        p16 = torch.full((n + 6,), 4.0, device=DEV, dtype=torch.bfloat16)
        ss = torch.tensor([sumsq], device=DEV) if sumsq is not None else None
        rc = _call_flat(cl, ptr, stream, p, g, buf if mu != 0 else None, p16, n, ss, wd, mu, damp, nesterov, first)
        torch.cuda.synchronize()
        assert rc == 0, cl.ce_last_error()
        tag = f"sgd n={n} clip={clip} wd={wd} step={step} {name}"
        bp, bb = _sgd_bounds(ref)
        if mu != 0:
            _within(buf[:n].cpu(), ref[1], bb, f"{tag} momentum_buffer")
        else:
            assert torch.equal(buf[:n].cpu(), bstart)
        _within(p[:n].cpu(), ref[0], bp, f"{tag} master")
        assert _same_bits(p16[:n], p[:n].to(torch.bfloat16))
        assert torch.equal(g[:n].cpu(), g0)
        for t in (p, g, buf):
            assert bool((t[n:] == 4.0).all())
        assert bool((p16[n:] == 4.0).all())


@gpu
def test_sgd_step_tiles_against_fp64():
    """``ce_sgd_step_tiles`` over the matrix / segment layout of test_adam_step_tiles_against_fp64 for the same grid: the same
    bounds, the mirror bit-equal to the masters' cast, every W^T copy bit-equal to the mirror's transpose, the 8 elements outside
    every matrix and segment untouched in p / buf / mirror."""
    cl, ptr, stream = _lib()
    n, N = TILE_N + 8, TILE_N
    seg_tab = torch.tensor(TILE_SEGS, dtype=torch.int64).to(DEV)
    for clip, wd, step, (name, mu, damp, nesterov) in SGD_GRID:
        first = step == 1
        p0, g0, b0, sumsq = _sgd_state(n, step, clip, 77 + step)
        ref = sgd_ref(p0, g0, b0, sumsq, wd, mu, damp, nesterov, first)
        bstart = torch.full_like(b0, POISON) if first else b0
        p, g, buf = _dev(p0, g0, bstart)
        p16 = torch.full((n,), 4.0, device=DEV, dtype=torch.bfloat16)
        wts = [torch.full((c, r), -4.0, device=DEV, dtype=torch.bfloat16) for _, r, c in TILE_MATS]
        tab, tiles = _job_table(TILE_MATS, p16, wts)
        ss = torch.tensor([sumsq], device=DEV) if sumsq is not None else None
        rc = _call_tiles(cl, ptr, stream, p, g, buf if mu != 0 else None, p16, tab, len(TILE_MATS), tiles, seg_tab, ss, wd, mu, damp,
                         nesterov, first)
        torch.cuda.synchronize()
        assert rc == 0, cl.ce_last_error()
        tag = f"sgd tiles clip={clip} wd={wd} step={step} {name}"
        bp, bb = _sgd_bounds(tuple(t[:N] for t in ref))
        if mu != 0:
            _within(buf[:N].cpu(), ref[1][:N], bb, f"{tag} momentum_buffer")
        else:
            assert torch.equal(buf.cpu(), bstart)
        _within(p[:N].cpu(), ref[0][:N], bp, f"{tag} master")
        assert _same_bits(p16[:N], p[:N].to(torch.bfloat16))
        for t, t0 in ((p, p0), (buf, bstart), (g, g0)):
            assert torch.equal(t[N:].cpu(), t0[N:])
        assert torch.equal(g.cpu(), g0)
        assert bool((p16[N:] == 4.0).all())
        for (off, r, c), wt in zip(TILE_MATS, wts):
            assert _same_bits(wt, p16[off:off + r * c].view(r, c).t()), (r, c)
