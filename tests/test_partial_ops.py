"""Op-level checks of the table-driven optimiser kernels of partial fine-tuning (csrc/optim.hip): ``ce_sumsq_segments`` and the
grouped update ``ce_adam_step_groups`` / ``ce_sgd_step_groups``, in the style of tests/test_embed_optim_ops.py and
tests/test_sgd_ops.py, whose grids, layout, fp64 restatements and bounds are imported."""
import ctypes
from ctypes import c_float, c_int, c_void_p

import numpy as np
import pytest
import torch

from tests.test_embed_optim_ops import (ADAM_GRID, B1, B2, DEV, EPS, LR, MAX_NORM, TILE_MATS, TILE_N, TILE_SEGS, U, _adam_bounds,
                                        _adam_state, _dev, _gen, _lib, _same_bits, _within, adam_ref)
from tests.test_sgd_ops import POISON, SGD_GRID, _call_tiles, _job_table, _sgd_bounds, sgd_ref

gpu = pytest.mark.gpu


def _null(t):
    return c_void_p(t.data_ptr()) if t is not None else c_void_p(0)


def _groups(rows):
    from clip_event_amd.optim import OptimGroup
    return (OptimGroup * len(rows))(*[OptimGroup(lr, wd, int(dec), 0) for lr, wd, dec in rows])


def _job_table_groups(mats, p16, wts, groups):
    """tests.test_sgd_ops._job_table with the group of every job in ``pad_``."""
    from clip_event_amd._lib import TransposeJob
    jobs, tiles = (TransposeJob * len(mats))(), 0
    for i, ((off, r, c), wt) in enumerate(zip(mats, wts)):
        jobs[i].src, jobs[i].dst = p16.data_ptr() + 2 * off, wt.data_ptr()
        jobs[i].rows, jobs[i].cols, jobs[i].tile_start, jobs[i].pad_ = r, c, tiles, groups[i]
        tiles += ((r + 63) // 64) * ((c + 63) // 64)
    return torch.frombuffer(bytearray(bytes(jobs)), dtype=torch.uint8).to(DEV), tiles


def _adam_groups(cl, ptr, stream, p, g, m, v, p16, tab, njobs, tiles, seg_tab, seg_group, ss, groups, step):
    return cl.ce_adam_step_groups(ptr(p), ptr(g), ptr(m), ptr(v), ptr(p16), _null(tab), c_int(njobs), c_int(tiles), ptr(seg_tab),
                                  c_int(seg_tab.shape[0]), _null(seg_group), _null(ss), c_float(MAX_NORM), groups, c_int(len(groups)),
                                  c_float(B1), c_float(B2), c_float(EPS), c_int(step), stream())


def _sgd_groups(cl, ptr, stream, p, g, buf, p16, tab, njobs, tiles, seg_tab, seg_group, ss, groups, mu, damp, nesterov, first):
    return cl.ce_sgd_step_groups(ptr(p), ptr(g), _null(buf), ptr(p16), _null(tab), c_int(njobs), c_int(tiles), ptr(seg_tab),
                                 c_int(seg_tab.shape[0]), _null(seg_group), _null(ss), c_float(MAX_NORM), groups, c_int(len(groups)),
                                 c_float(mu), c_float(damp), c_int(int(nesterov)), c_int(int(first)), stream())


# ---- ce_sumsq_segments -------------------------------------------------------------------------------------------------------

# chunk lengths 4, 2044 and 65536, and one range of 132072 elements cut into three chunks (65536 + 65536 + 1000)
SUMSQ_CHUNKS = [(8, 12), (100, 2144), (4096, 69632), (70000, 135536), (135536, 201072), (201072, 202072)]
SUMSQ_N = 202100


def _poisoned(values):
    """``values`` inside SUMSQ_CHUNKS, NaN everywhere else."""
    g = torch.full((SUMSQ_N,), float("nan"), device=DEV)
    for lo, hi in SUMSQ_CHUNKS:
        g[lo:hi] = values[lo:hi]
    return g


@gpu
def test_sumsq_segments_exact_on_exactly_summable_data():
    """``ce_sumsq_segments`` adds sum g^2 over the table into *out.  Entries in {0, +-1/4, +-1/2} as in
    test_sumsq_exact_on_exactly_summable_data: every square and partial sum is a multiple of 1/16 below 2^20, exact in fp32 in any
    order, so the result EQUALS the fp64 sum plus the non-zero start -- a dropped or doubled element shows, and an element read
    outside the table makes the result NaN.  The first and the last element of every chunk are non-zero."""
    cl, ptr, stream = _lib()
    vals = torch.randint(-2, 3, (SUMSQ_N,), generator=_gen(91), device=DEV).float() / 4
    for lo, hi in SUMSQ_CHUNKS:
        vals[lo] = vals[hi - 1] = 0.5
    g = _poisoned(vals)
    tab = torch.tensor(SUMSQ_CHUNKS, dtype=torch.int64).to(DEV)
    out = torch.tensor([1.5, 7.0], device=DEV)
    assert cl.ce_sumsq_segments(ptr(g), ptr(tab), c_int(len(SUMSQ_CHUNKS)), ptr(out), stream()) == 0, cl.ce_last_error()
    torch.cuda.synchronize()
    want = 1.5 + sum(float((vals[lo:hi].double() ** 2).sum()) for lo, hi in SUMSQ_CHUNKS)
    assert float(out[0]) == want and float(out[1]) == 7.0, (float(out[0]), want)


@gpu
def test_sumsq_segments_against_fp64():
    """The same on normal data, with test_sumsq_against_fp64's bound: positive terms, one workgroup and one atomic per chunk:
    rel error <= (chunks + 16) 2^-24 of the total."""
    cl, ptr, stream = _lib()
    vals = torch.randn(SUMSQ_N, generator=_gen(92), device=DEV)
    g = _poisoned(vals)
    tab = torch.tensor(SUMSQ_CHUNKS, dtype=torch.int64).to(DEV)
    out = torch.tensor([3.0], device=DEV)
    assert cl.ce_sumsq_segments(ptr(g), ptr(tab), c_int(len(SUMSQ_CHUNKS)), ptr(out), stream()) == 0, cl.ce_last_error()
    torch.cuda.synchronize()
    want = 3.0 + sum(float((vals[lo:hi].double() ** 2).sum()) for lo, hi in SUMSQ_CHUNKS)
    rel = abs(float(out[0]) - want) / want
    bound = (len(SUMSQ_CHUNKS) + 16) * U
    print(f"[sumsq_segments] rel {rel:.2e} (bound {bound:.2e})")
    assert rel <= bound


# ---- one group, not decoupled: the bits of the ungrouped entry points ------------------------------------------------------------

def _tile_run(n, call):
    """One run over the TILE_* layout: fresh mirror (4.0) and W^T copies (-4.0), ``call(p16, wts)`` -> rc."""
    p16 = torch.full((n,), 4.0, device=DEV, dtype=torch.bfloat16)
    wts = [torch.full((c, r), -4.0, device=DEV, dtype=torch.bfloat16) for _, r, c in TILE_MATS]
    rc = call(p16, wts)
    torch.cuda.synchronize()
    return rc, p16, wts


@gpu
def test_one_group_adam_leaves_the_bits_of_the_ungrouped_step():
    """``ce_adam_step_groups`` with one group that is not decoupled against ``ce_adam_step_tiles`` over ADAM_GRID on the TILE_*
    layout: masters, both moments, the mirror, every W^T copy and the 8 guard elements bit for bit (segment_group NULL and a
    table of zeros alike)."""
    cl, ptr, stream = _lib()
    n = TILE_N + 8
    seg_tab = torch.tensor(TILE_SEGS, dtype=torch.int64).to(DEV)
    zeros = torch.zeros(len(TILE_SEGS), dtype=torch.int32, device=DEV)
    for clip, wd, step in ADAM_GRID:
        p0, g0, m0, v0, sumsq = _adam_state(n, step, clip, 77 + step)
        ss = torch.tensor([sumsq], device=DEV) if sumsq is not None else None
        outs = []
        for form in ("tiles", "groups", "groups+table"):
            p, g, m, v = _dev(p0, g0, m0, v0)

            def call(p16, wts):
                tab, tiles = _job_table(TILE_MATS, p16, wts)
                if form == "tiles":
                    return cl.ce_adam_step_tiles(ptr(p), ptr(g), ptr(m), ptr(v), ptr(p16), ptr(tab), c_int(len(TILE_MATS)), c_int(tiles),
                                                 ptr(seg_tab), c_int(len(TILE_SEGS)), _null(ss), c_float(MAX_NORM), c_float(LR), c_float(B1),
                                                 c_float(B2), c_float(EPS), c_float(wd), c_int(step), stream())
                return _adam_groups(cl, ptr, stream, p, g, m, v, p16, tab, len(TILE_MATS), tiles, seg_tab,
                                    zeros if form == "groups+table" else None, ss, _groups([(LR, wd, 0)]), step)
            rc, p16, wts = _tile_run(n, call)
            assert rc == 0, cl.ce_last_error()
            outs.append((p, m, v, p16, *wts))
        for other in outs[1:]:
            for i, (a, b) in enumerate(zip(other, outs[0])):
                assert _same_bits(a, b), (clip, wd, step, i)
        assert torch.equal(outs[1][0][TILE_N:].cpu(), p0[TILE_N:]) and bool((outs[1][3][TILE_N:] == 4.0).all())


@gpu
def test_one_group_sgd_leaves_the_bits_of_the_ungrouped_step():
    """The same for ``ce_sgd_step_groups`` against ``ce_sgd_step_tiles`` over SGD_GRID (momentum 0: no buffer)."""
    cl, ptr, stream = _lib()
    n = TILE_N + 8
    seg_tab = torch.tensor(TILE_SEGS, dtype=torch.int64).to(DEV)
    for clip, wd, step, (name, mu, damp, nesterov) in SGD_GRID:
        first = step == 1
        p0, g0, b0, _, sumsq = _adam_state(n, step, clip, 77 + step)
        bstart = torch.full_like(b0, POISON) if first else b0
        ss = torch.tensor([sumsq], device=DEV) if sumsq is not None else None
        outs = []
        for form in ("tiles", "groups"):
            p, g, buf = _dev(p0, g0, bstart)
            b = buf if mu != 0 else None

            def call(p16, wts):
                tab, tiles = _job_table(TILE_MATS, p16, wts)
                if form == "tiles":
                    return _call_tiles(cl, ptr, stream, p, g, b, p16, tab, len(TILE_MATS), tiles, seg_tab, ss, wd, mu, damp, nesterov, first)
                return _sgd_groups(cl, ptr, stream, p, g, b, p16, tab, len(TILE_MATS), tiles, seg_tab, None, ss, _groups([(LR, wd, 0)]),
                                   mu, damp, nesterov, first)
            rc, p16, wts = _tile_run(n, call)
            assert rc == 0, cl.ce_last_error()
            outs.append((p, buf, p16, *wts))
        for i, (a, b) in enumerate(zip(outs[1], outs[0])):
            assert _same_bits(a, b), (clip, wd, step, name, i)
        assert torch.equal(outs[1][0][TILE_N:].cpu(), p0[TILE_N:]) and bool((outs[1][2][TILE_N:] == 4.0).all())


# ---- three groups, a frozen matrix and a frozen segment --------------------------------------------------------------------------

# The 8 x 8 matrix and the segment (16452, 16500) are in no table.  Groups: 0 = the grid's weight decay at LR; 1 = half the rate and
# no decay; 2 = twice the rate, decay 0.05 -- decoupled for Adam.  Scalars as the kernel receives them (fp32).
FROZEN_MAT, FROZEN_SEG = 1, 2
LIVE_MATS = [(m, g) for i, (m, g) in enumerate(zip(TILE_MATS, (1, 0, 2))) if i != FROZEN_MAT]
LIVE_SEGS = [(s, g) for i, (s, g) in enumerate(zip(TILE_SEGS, (0, 1, 0, 2, 0))) if i != FROZEN_SEG]
LR1, LR2, WD2 = (float(np.float32(x)) for x in (LR * 0.5, LR * 2, 0.05))


def _group_rows(wd, decoupled):
    return [(LR, wd, 0), (LR1, 0.0, 0), (LR2, WD2, int(decoupled))]


def _element_scalars(n, rows):
    """Per element: learning rate, weight decay, decoupled flag (fp64) and whether anything updates it."""
    lr, wd, dec, live = torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64), \
        torch.zeros(n, dtype=torch.bool)
    ranges = [((off, off + r * c), g) for (off, r, c), g in LIVE_MATS] + LIVE_SEGS
    for (lo, hi), g in ranges:
        assert not bool(live[lo:hi].any())
        lr[lo:hi], wd[lo:hi], dec[lo:hi], live[lo:hi] = rows[g][0], rows[g][1], float(rows[g][2]), True
    return lr, wd, dec, live


def _all_segments():
    """The live ranges, matrices included, as segments of at most 2048 elements with their groups."""
    segs, groups = [], []
    for (lo, hi), g in sorted([((off, off + r * c), g) for (off, r, c), g in LIVE_MATS] + LIVE_SEGS):
        for c in range(lo, hi, 2048):
            segs.append((c, min(c + 2048, hi)))
            groups.append(g)
    return torch.tensor(segs, dtype=torch.int64).to(DEV), torch.tensor(groups, dtype=torch.int32).to(DEV)


def _frozen_gradient(g0, live):
    g = g0.clone()
    g[:TILE_N][~live[:TILE_N]] = float("nan")
    return g


def _check_untouched(tag, live, pairs, p16, wts):
    """Frozen ranges and the guard elements: the start bits in every fp32 buffer, the sentinel in the mirror and in the frozen
    matrix's W^T copy."""
    dead = ~live
    for name, t, t0 in pairs:
        assert _same_bits(t.cpu()[dead], t0[dead]), (tag, name)
    assert bool((p16.cpu()[dead] == 4.0).all()), tag
    assert bool((wts[FROZEN_MAT] == -4.0).all()), tag


@gpu
def test_three_group_adam_against_fp64():
    """``ce_adam_step_groups`` with three groups (distinct lr / weight decay, one decoupled = AdamW) over ADAM_GRID, the 8 x 8 matrix
    and one segment frozen with NaN gradients: every updated element against adam_ref with ITS group's scalars within _adam_bounds
    -- adam_ref's update is linear in the rate, so it is rescaled by lr / LR; the decoupled group has p (1 - lr wd) in front and
    no decay in the gradient, and one more U |p| on p for that multiply-add's rounding.  The mirror is the cast, W^T the transpose;
    frozen p / m / v / mirror / W^T and the guards keep their bits; the tile + segment form equals the segments-only form."""
    cl, ptr, stream = _lib()
    n, N = TILE_N + 8, TILE_N
    seg_tab = torch.tensor([s for s, _ in LIVE_SEGS], dtype=torch.int64).to(DEV)
    seg_group = torch.tensor([g for _, g in LIVE_SEGS], dtype=torch.int32).to(DEV)
    all_segs, all_groups = _all_segments()
    for clip, wd, step in ADAM_GRID:
        rows = _group_rows(wd, True)
        lr_e, wd_e, dec_e, live = _element_scalars(n, rows)
        p0, g0, m0, v0, sumsq = _adam_state(n, step, clip, 177 + step)
        ss = torch.tensor([sumsq], device=DEV) if sumsq is not None else None
        ref = adam_ref(p0, g0, m0, v0, sumsq, wd_e * (1 - dec_e), step)
        p_ref = p0.double() * (1 - dec_e * lr_e * wd_e) + (ref[0] - p0.double()) * (lr_e / LR)
        ref = (p_ref, ref[1], ref[2], ref[3], ref[4], ref[5], ref[6] * lr_e / LR)
        bp, bm, bv = _adam_bounds(ref)
        bp = bp + dec_e * U * p_ref.abs()
        outs = {}
        for form in ("tiles", "segments"):
            p, g, m, v = _dev(p0, _frozen_gradient(g0, live), m0, v0)

            def call(p16, wts):
                if form == "segments":
                    return _adam_groups(cl, ptr, stream, p, g, m, v, p16, None, 0, 0, all_segs, all_groups, ss, _groups(rows), step)
                tab, tiles = _job_table_groups([mat for mat, _ in LIVE_MATS], p16, [wts[0], wts[2]], [gr for _, gr in LIVE_MATS])
                return _adam_groups(cl, ptr, stream, p, g, m, v, p16, tab, len(LIVE_MATS), tiles, seg_tab, seg_group, ss, _groups(rows), step)
            rc, p16, wts = _tile_run(n, call)
            assert rc == 0, cl.ce_last_error()
            outs[form] = (p, m, v, p16)
            tag = f"adam groups {form} clip={clip} wd={wd} step={step}"
            _check_untouched(tag, live, (("p", p, p0), ("m", m, m0), ("v", v, v0)), p16, wts)
            for name, t, want, bound in (("exp_avg", m, ref[1], bm), ("exp_avg_sq", v, ref[2], bv), ("master", p, ref[0], bp)):
                _within(t.cpu()[live], want[live], bound[live], f"{tag} {name}")
            assert _same_bits(p16.cpu()[live], p.cpu()[live].to(torch.bfloat16)), tag
            if form == "tiles":
                for (off, r, c), wt in ((TILE_MATS[0], wts[0]), (TILE_MATS[2], wts[2])):
                    assert _same_bits(wt, p16[off:off + r * c].view(r, c).t()), (tag, r, c)
        for a, b in zip(outs["tiles"], outs["segments"]):
            assert _same_bits(a, b), (clip, wd, step)


@gpu
def test_three_group_sgd_against_fp64():
    """The same for ``ce_sgd_step_groups`` over SGD_GRID against sgd_ref / _sgd_bounds with every element's own lr and weight decay
    (no decoupled form: SGD has none)."""
    cl, ptr, stream = _lib()
    n, N = TILE_N + 8, TILE_N
    seg_tab = torch.tensor([s for s, _ in LIVE_SEGS], dtype=torch.int64).to(DEV)
    seg_group = torch.tensor([g for _, g in LIVE_SEGS], dtype=torch.int32).to(DEV)
    all_segs, all_groups = _all_segments()
    for clip, wd, step, (name, mu, damp, nesterov) in SGD_GRID:
        first = step == 1
        rows = _group_rows(wd, False)
        lr_e, wd_e, _, live = _element_scalars(n, rows)
        p0, g0, b0, _, sumsq = _adam_state(n, step, clip, 177 + step)
        bstart = torch.full_like(b0, POISON) if first else b0
        ss = torch.tensor([sumsq], device=DEV) if sumsq is not None else None
        ref = sgd_ref(p0, g0, b0, sumsq, wd_e, mu, damp, nesterov, first, lr=lr_e)
        bp, bb = _sgd_bounds(ref, lr=lr_e)
        outs = {}
        for form in ("tiles", "segments"):
            p, g, buf = _dev(p0, _frozen_gradient(g0, live), bstart)
            b = buf if mu != 0 else None

            def call(p16, wts):
                if form == "segments":
                    return _sgd_groups(cl, ptr, stream, p, g, b, p16, None, 0, 0, all_segs, all_groups, ss, _groups(rows), mu, damp,
                                       nesterov, first)
                tab, tiles = _job_table_groups([mat for mat, _ in LIVE_MATS], p16, [wts[0], wts[2]], [gr for _, gr in LIVE_MATS])
                return _sgd_groups(cl, ptr, stream, p, g, b, p16, tab, len(LIVE_MATS), tiles, seg_tab, seg_group, ss, _groups(rows), mu,
                                   damp, nesterov, first)
            rc, p16, wts = _tile_run(n, call)
            assert rc == 0, cl.ce_last_error()
            outs[form] = (p, buf, p16)
            tag = f"sgd groups {form} clip={clip} wd={wd} step={step} {name}"
            _check_untouched(tag, live, (("p", p, p0), ("buf", buf, bstart)), p16, wts)
            if mu != 0:
                _within(buf.cpu()[live], ref[1][live], bb[live], f"{tag} momentum_buffer")
            else:
                assert torch.equal(buf.cpu(), bstart)
            _within(p.cpu()[live], ref[0][live], bp[live], f"{tag} master")
            assert _same_bits(p16.cpu()[live], p.cpu()[live].to(torch.bfloat16)), tag
            if form == "tiles":
                for (off, r, c), wt in ((TILE_MATS[0], wts[0]), (TILE_MATS[2], wts[2])):
                    assert _same_bits(wt, p16[off:off + r * c].view(r, c).t()), (tag, r, c)
        for a, b in zip(outs["tiles"], outs["segments"]):
            assert _same_bits(a, b), (clip, wd, step, name)
