"""Op-level checks of the weight EMA carried by the optimiser kernels (csrc/optim.hip: the ``_ema`` twin of every step entry
point, and ``ce_swap_cast_bf16``) in the style of tests/test_sgd_ops.py, whose helpers and those of
tests/test_embed_optim_ops.py and tests/test_partial_ops.py are imported: an fp64 restatement of the element function with a
bound counted from its fp32 roundings, bit-equality wherever a kernel only moves or must not differ, sentinels behind every
buffer."""
import functools
from ctypes import c_float, c_int, c_long, c_void_p

import numpy as np
import pytest
import torch

from tests.test_embed_optim_ops import (B1, B2, DEV, EPS, LR, MAX_NORM, TILE_MATS, TILE_N, TILE_SEGS, U, _adam_state, _lib,
                                        _same_bits, _within)
from tests.test_partial_ops import LIVE_MATS, LIVE_SEGS, _element_scalars, _group_rows, _groups, _job_table_groups
from tests.test_sgd_ops import MU, POISON, WD, _job_table

gpu = pytest.mark.gpu

# the rates as the kernels receive them (fp32); the references use the same fp32-rounded values
RATES = [float(np.float32(r)) for r in (1.0, 0.1, 1e-4)]
KINDS = ("adam", "sgd", "sgd0")             # Adam; SGD with momentum 0.9; SGD with momentum 0 (no buffer)
EMA_GRID = [(kind, step, clip, rate) for step in (1, 2) for clip in ("active", "none") for kind in KINDS for rate in RATES]
EINVAL = -22


def ema_ref(e, p_new, rate):
    """fp64 restatement of optim.hip's ema_elem: e + rate (p_new - e)."""
    e, p_new = e.double(), p_new.double()
    return e + rate * (p_new - e)


def _ema_bound(ref, e, p_new, rate):
    """Element bound on the fp32 average against ema_ref, from ema_elem's two roundings (|d1|, |d2|, |d3| <= U = 2^-24).
    Below a rate of 0.5 the kernel forms d = (p - e)(1 + d1), then the multiply-add (e + d rate)(1 + d2): the result is
    ref (1 + d2) + rate (p - e) d1 (1 + d2).  From 0.5 on it forms t = d (1 - rate) -- 1 - rate is exact for an fp32 rate in
    [0.5, 1] -- with one more rounding, then (p - t)(1 + d3): ref (1 + d3) - (1 - rate)(p - e)(d1 + d2 + d1 d2)(1 + d3).  Either way
    |error| <= U |ref| + 2 U w |p - e| with w = min(rate, 1 - rate), up to second-order terms, for which the whole is widened by
    2^-20 of itself.  At rate 1 this is U |ref| (and the test asks for equality there anyway)."""
    w = min(rate, 1.0 - rate)
    return (1 + 2.0 ** -20) * (U * ref.abs() + 2 * U * w * (p_new.double() - e.double()).abs())


def _ema_start(p0, seed):
    """An average like one that trails the masters: p0 plus noise of half the masters' own size."""
    gen = torch.Generator().manual_seed(1000 + seed)
    return p0 + torch.randn(p0.shape, generator=gen) * 0.01


@functools.lru_cache(maxsize=4)
def _start(n, step, clip, seed):
    """(p, g, m, v, sumsq or None, e) of the Adam tests' generator plus a starting average, computed once per case and shared by
    the kinds and rates of a grid (host tensors; nobody writes them)."""
    p0, g0, m0, v0, sumsq = _adam_state(n, step, clip, seed)
    return p0, g0, m0, v0, sumsq, _ema_start(p0, seed)


def test_ema_reference_matches_torch_lerp():
    """CPU cross-check of the restatement and its bound: ``torch.Tensor.lerp_`` on fp32 copies (the same two-branch form) lands
    within _ema_bound for rates 1.0, 0.1 and 1e-4 over the Adam tests' state generator, n = 999; rate 1 gives the end point
    itself."""
    worst = 0.0
    for rate in RATES:
        for seed in (5, 6):
            p0, g0, _, _, _ = _adam_state(999, 2, "active", seed)
            p_new = p0 - LR * g0                          # any fp32 vector near p0 serves as "the masters after the step"
            e0 = _ema_start(p0, seed)
            got = e0.clone().lerp_(p_new, rate)
            ref = ema_ref(e0, p_new, rate)
            bound = _ema_bound(ref, e0, p_new, rate)
            err = (got.double() - ref).abs()
            ratio = float((err / bound.clamp_min(1e-300)).max())
            worst = max(worst, ratio)
            assert bool((err <= bound).all()), (rate, seed, ratio)
            if rate == 1.0:
                assert torch.equal(got, p_new)
    print(f"[ema_ref vs torch lerp_] worst |err| / bound {worst:.3f}")


# ---- calling the twelve entry points -----------------------------------------------------------------------------------------------

def _null(t):
    return c_void_p(t.data_ptr()) if t is not None else c_void_p(0)


def _state_of(kind, step, p0, m0, v0):
    """The state streams of ``kind`` at ``step`` as host tensors: Adam's two moments; SGD's momentum buffer, poisoned before a
    first step (it must be overwritten, never read); nothing for momentum 0."""
    if kind == "adam":
        return [m0, v0]
    if kind == "sgd":
        return [torch.full_like(m0, POISON) if step == 1 else m0]
    return []


def _tail(kind, step, groups=None):
    """The scalar arguments between ``sumsq, max_norm`` and the EMA pair: ungrouped with lr / weight decay, grouped with the
    table in their place."""
    if kind == "adam":
        own = (c_float(B1), c_float(B2), c_float(EPS))
        if groups is not None:
            return (groups, c_int(len(groups)), *own, c_int(step))
        return (c_float(LR), *own, c_float(WD), c_int(step))
    mu = MU if kind == "sgd" else 0.0
    if groups is not None:
        return (groups, c_int(len(groups)), c_float(mu), c_float(0.0), c_int(0), c_int(int(step == 1)))
    return (c_float(LR), c_float(mu), c_float(0.0), c_float(WD), c_int(0), c_int(int(step == 1)))


def _step(kind, form, p, g, state, p16, ss, step, ema=None, rate=None, n=None, tables=None, groups=None, with_ema=True):
    """One launch of the ``form`` ("flat" / "tiles" / "groups") entry point of ``kind``; with ``with_ema`` its _ema twin (``ema``
    may then be None: the argument check).  ``tables`` = (jobs, njobs, tiles, seg_tab, seg_group)."""
    cl, ptr, stream = _lib()
    stem = {"adam": "ce_adam_step", "sgd": "ce_sgd_step", "sgd0": "ce_sgd_step"}[kind] + {"flat": "", "tiles": "_tiles", "groups": "_groups"}[form]
    st = [ptr(t) for t in state] if kind != "sgd0" else [c_void_p(0)]
    args = [ptr(p), ptr(g), *st, ptr(p16)]
    if form == "flat":
        args.append(c_long(n))
    else:
        jobs, njobs, tiles, seg_tab, seg_group = tables
        args += [_null(jobs), c_int(njobs), c_int(tiles), _null(seg_tab), c_int(seg_tab.shape[0] if seg_tab is not None else 0)]
        if form == "groups":
            args.append(_null(seg_group))
    args += [_null(ss), c_float(MAX_NORM), *_tail(kind, step, groups if form == "groups" else None)]
    if with_ema:
        args += [_null(ema), c_float(rate)]
        stem += "_ema"
    rc = getattr(cl, stem)(*args, stream())
    torch.cuda.synchronize()
    return rc


def _guarded(t, guard=6):
    return torch.cat([t, torch.full((guard,), 4.0)]).to(DEV)


def _check_average(tag, e, e0, p_out, rate):
    """The average against ema_ref of the kernel's OWN fp32 masters; rate 1: their bits."""
    if rate == 1.0:
        assert _same_bits(e, p_out), tag
        return
    ref = ema_ref(e0, p_out, rate)
    _within(e, ref, _ema_bound(ref, e0, p_out, rate), f"{tag} average")


# ---- 1. against the fp64 restatement -----------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("n", [5, 7171, 1000003])
def test_ema_step_flat_against_fp64(n):
    """The flat ``_ema`` entry points over EMA_GRID (Adam / SGD with momentum / SGD without; step 1 / 2; clip active / off; rates
    1, 0.1, 1e-4), n with n % 4 != 0 and n % 2048 != 0: masters, state and mirror carry the bits of the entry point without EMA
    on the same inputs; the average is within _ema_bound of ema_ref(e0, the kernel's own masters); rate 1 copies; the guard
    elements behind every buffer, the average included, are intact and the gradient is not written."""
    for kind, step, clip, rate in EMA_GRID:
        p0, g0, m0, v0, sumsq, e0 = _start(n, step, clip, n + step)
        ss = torch.tensor([sumsq], device=DEV) if sumsq is not None else None
        outs = []
        for with_ema in (False, True):
            p, g, e = _guarded(p0), _guarded(g0), _guarded(e0)
            state = [_guarded(t) for t in _state_of(kind, step, p0, m0, v0)]
            p16 = torch.full((n + 6,), 4.0, device=DEV, dtype=torch.bfloat16)
            rc = _step(kind, "flat", p, g, state, p16, ss, step, e, rate, n=n, with_ema=with_ema)
            assert rc == 0, _lib()[0].ce_last_error()
            outs.append((p, *state, p16, g, e))
        tag = f"ema flat n={n} {kind} step={step} clip={clip} rate={rate}"
        for a, b in zip(outs[0][:-1], outs[1][:-1]):
            assert _same_bits(a, b), tag                                   # guards included
        plain_e, (p, e) = outs[0][-1], (outs[1][0], outs[1][-1])
        assert _same_bits(plain_e[:n].cpu(), e0) and torch.equal(outs[1][-2][:n].cpu(), g0)
        assert not _same_bits(p[:n].cpu(), p0)
        assert bool((e[n:] == 4.0).all()) and bool((p[n:] == 4.0).all()) and bool((outs[1][-3][n:] == 4.0).all())
        _check_average(tag, e[:n], e0.to(DEV), p[:n], rate)


def _tile_tables(p16, wts):
    jobs, tiles = _job_table(TILE_MATS, p16, wts)
    return jobs, len(TILE_MATS), tiles, torch.tensor(TILE_SEGS, dtype=torch.int64).to(DEV), None


def _fresh_tiles(n):
    p16 = torch.full((n,), 4.0, device=DEV, dtype=torch.bfloat16)
    wts = [torch.full((c, r), -4.0, device=DEV, dtype=torch.bfloat16) for _, r, c in TILE_MATS]
    return p16, wts


@gpu
def test_ema_step_tiles_against_fp64():
    """The tile + segment ``_ema`` entry points over EMA_GRID on the TILE_MATS / TILE_SEGS layout: masters, state, mirror and
    every W^T copy carry the bits of the entry point without EMA; the average within _ema_bound of ema_ref over everything the
    tables cover; the 8 elements that belong to nothing keep their bits in the average too."""
    n, N = TILE_N + 8, TILE_N
    for kind, step, clip, rate in EMA_GRID:
        p0, g0, m0, v0, sumsq, e0 = _start(n, step, clip, 77 + step)
        ss = torch.tensor([sumsq], device=DEV) if sumsq is not None else None
        outs = []
        for with_ema in (False, True):
            p, g, e = p0.to(DEV), g0.to(DEV), e0.to(DEV)
            state = [t.to(DEV) for t in _state_of(kind, step, p0, m0, v0)]
            p16, wts = _fresh_tiles(n)
            rc = _step(kind, "tiles", p, g, state, p16, ss, step, e, rate, tables=_tile_tables(p16, wts), with_ema=with_ema)
            assert rc == 0, _lib()[0].ce_last_error()
            outs.append((p, *state, p16, *wts, g, e))
        tag = f"ema tiles {kind} step={step} clip={clip} rate={rate}"
        for a, b in zip(outs[0][:-1], outs[1][:-1]):
            assert _same_bits(a, b), tag
        p, e = outs[1][0], outs[1][-1]
        assert _same_bits(outs[0][-1].cpu(), e0) and torch.equal(outs[1][-2].cpu(), g0)
        assert _same_bits(e[N:].cpu(), e0[N:]) and _same_bits(p[N:].cpu(), p0[N:])
        assert not _same_bits(p[:N].cpu(), p0[:N])
        _check_average(tag, e[:N], e0[:N].to(DEV), p[:N], rate)


# ---- 2. the forms agree ------------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_ema_forms_give_the_same_bits(kind):
    """Flat, tiles + segments, and the grouped form with one group over everything: bit-identical averages (and masters), at
    step 2 with the clip active for rates 0.1 and 1e-4."""
    n, N = TILE_N + 8, TILE_N
    step = 2
    p0, g0, m0, v0, sumsq = _adam_state(n, step, "active", 311)
    e0 = _ema_start(p0, 311)
    ss = torch.tensor([sumsq], device=DEV)
    for rate in RATES[1:]:
        outs = {}
        for form in ("flat", "tiles", "groups"):
            p, g, e = p0.to(DEV), g0.to(DEV), e0.to(DEV)
            state = [t.to(DEV) for t in _state_of(kind, step, p0, m0, v0)]
            p16, wts = _fresh_tiles(n)
            rc = _step(kind, form, p, g, state, p16, ss, step, e, rate, n=N, tables=_tile_tables(p16, wts), groups=_groups([(LR, WD, 0)]))
            assert rc == 0, _lib()[0].ce_last_error()
            outs[form] = (e, p, *state, p16)
        assert not _same_bits(outs["flat"][0][:N], e0[:N].to(DEV))
        for form in ("tiles", "groups"):
            for i, (a, b) in enumerate(zip(outs[form], outs["flat"])):
                assert _same_bits(a, b), (kind, rate, form, i)


# ---- 3. frozen ranges --------------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_ema_leaves_frozen_ranges_alone(kind):
    """The grouped form with tests/test_partial_ops.py's tables, which leave out the 8 x 8 matrix and one segment: there (and in
    the 8 guard elements) the average keeps its poisoned prior content -- NaN -- bit for bit, the gradient there is NaN and is
    never read; everywhere else the average moved (it starts 1 away from the masters) and follows ema_ref."""
    n = TILE_N + 8
    step, rate = 2, RATES[1]
    rows = _group_rows(WD, kind == "adam")
    _, _, _, live = _element_scalars(n, rows)
    p0, g0, m0, v0, sumsq = _adam_state(n, step, "active", 419)
    g0 = g0.clone()
    g0[~live] = float("nan")
    e0 = p0 + 1.0
    e0[~live] = float("nan")
    p, g, e = p0.to(DEV), g0.to(DEV), e0.to(DEV)
    state = [t.to(DEV) for t in _state_of(kind, step, p0, m0, v0)]
    p16, wts = _fresh_tiles(n)
    jobs, tiles = _job_table_groups([mat for mat, _ in LIVE_MATS], p16, [wts[0], wts[2]], [gr for _, gr in LIVE_MATS])
    seg_tab = torch.tensor([s for s, _ in LIVE_SEGS], dtype=torch.int64).to(DEV)
    seg_group = torch.tensor([gr for _, gr in LIVE_SEGS], dtype=torch.int32).to(DEV)
    rc = _step(kind, "groups", p, g, state, p16, torch.tensor([sumsq], device=DEV), step, e, rate,
               tables=(jobs, len(LIVE_MATS), tiles, seg_tab, seg_group), groups=_groups(rows))
    assert rc == 0, _lib()[0].ce_last_error()
    e_h, p_h = e.cpu(), p.cpu()
    assert _same_bits(e_h[~live], e0[~live]) and _same_bits(p_h[~live], p0[~live])
    assert bool(torch.isfinite(e_h[live]).all()) and bool((e_h[live] != e0[live]).all())
    _check_average(f"ema frozen ranges {kind}", e_h[live], e0[live], p_h[live], rate)


# ---- 4. ce_swap_cast_bf16 ----------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("n", [5, 7171, 1000003])
def test_swap_cast_exchanges_and_mirrors(n):
    """``ce_swap_cast_bf16``: a and b change places bit for bit, the mirror equals ``ce_cast_bf16`` of the new a bit for bit, a
    second call restores both buffers (and the mirror of the first a), and the guard elements behind all three are intact."""
    cl, ptr, stream = _lib()
    gen = torch.Generator().manual_seed(n)
    a0, b0 = torch.randn(n, generator=gen), torch.randn(n, generator=gen) * 0.02
    a0[0], b0[n - 1] = float("inf"), -0.0
    a, b = _guarded(a0), _guarded(b0)
    a16 = torch.full((n + 6,), 4.0, device=DEV, dtype=torch.bfloat16)
    want16 = torch.empty(n, device=DEV, dtype=torch.bfloat16)
    for new_a, new_b in ((b0, a0), (a0, b0)):
        assert cl.ce_swap_cast_bf16(ptr(a), ptr(b), ptr(a16), c_long(n), stream()) == 0, cl.ce_last_error()
        assert cl.ce_cast_bf16(ptr(a), ptr(want16), c_long(n), stream()) == 0, cl.ce_last_error()
        torch.cuda.synchronize()
        assert _same_bits(a[:n].cpu(), new_a) and _same_bits(b[:n].cpu(), new_b)
        assert _same_bits(a16[:n], want16)
        assert bool((a[n:] == 4.0).all()) and bool((b[n:] == 4.0).all()) and bool((a16[n:] == 4.0).all())
    assert cl.ce_swap_cast_bf16(ptr(a), ptr(a), ptr(a16), c_long(n), stream()) == EINVAL
    assert cl.ce_swap_cast_bf16(ptr(a), ptr(b), ptr(a16), c_long(0), stream()) == EINVAL


# ---- 5. argument checks ------------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("kind", ["adam", "sgd"])
@pytest.mark.parametrize("form", ["flat", "tiles", "groups"])
def test_ema_argument_checks(kind, form):
    """NULL ``ema``, rate 0 and rate 1.5 (and a negative rate, and NaN) return -EINVAL from every ``_ema`` entry point, and
    nothing was launched: every buffer keeps its bits."""
    n, N = TILE_N + 8, TILE_N
    step = 2
    p0, g0, m0, v0, sumsq = _adam_state(n, step, "active", 523)
    e0 = _ema_start(p0, 523)
    p, g, e = p0.to(DEV), g0.to(DEV), e0.to(DEV)
    state0 = _state_of(kind, step, p0, m0, v0)
    state = [t.to(DEV) for t in state0]
    p16, wts = _fresh_tiles(n)
    tables = _tile_tables(p16, wts)
    ss = torch.tensor([sumsq], device=DEV)
    for ema, rate in ((None, 0.1), (e, 0.0), (e, 1.5), (e, -0.1), (e, float("nan"))):
        rc = _step(kind, form, p, g, state, p16, ss, step, ema, rate, n=N, tables=tables, groups=_groups([(LR, WD, 0)]))
        assert rc == EINVAL, (ema is None, rate, rc)
        assert b"ema" in _lib()[0].ce_last_error()
    assert _same_bits(p.cpu(), p0) and _same_bits(e.cpu(), e0) and all(_same_bits(t.cpu(), t0) for t, t0 in zip(state, state0))
    assert bool((p16 == 4.0).all()) and all(bool((wt == -4.0).all()) for wt in wts)
    assert _step(kind, form, p, g, state, p16, ss, step, e, 1.0, n=N, tables=tables, groups=_groups([(LR, WD, 0)])) == 0
    assert _same_bits(e[:N], p[:N])
