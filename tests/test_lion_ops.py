"""Op-level checks of clip + Lion (csrc/optim.hip: ``ce_lion_step`` and its tiles / groups / ``_ema`` forms) against an fp64
restatement of the kernel's element function, in the style of tests/test_sgd_ops.py (whose helpers, and those of
tests/test_embed_optim_ops.py, tests/test_partial_ops.py and tests/test_ema_ops.py, are imported): element-wise bounds from the
count of fp32 roundings, bit-equality where a kernel only rounds or moves or must not differ, sentinels behind every buffer.

The sign.  A master moves by exactly ``lr``, so a wrong sign is an error of ``2 lr`` and no rounding bound covers it.  The sign
of ``c = b1 m + (1 - b1) gc`` is decided in fp32, where c carries about four roundings of terms of size
``c_mag = b1 |m| + (1 - b1) |gc|``; an element is AMBIGUOUS when the fp64 ``|c| <= 2^-20 c_mag``: there fp32 may land on the other
side of zero (or on it) and the master may differ by up to ``2 lr`` more.  Everywhere else the sign must agree.  Every case first
asserts, on the fp64 reference alone, that it has at most 4 ambiguous elements (this generator has none)."""
import math
from ctypes import c_float, c_int, c_long, c_void_p

import numpy as np
import pytest
import torch

from tests.test_embed_optim_ops import (DEV, LR, MAX_NORM, TILE_MATS, TILE_N, TILE_SEGS, U, _adam_state, _dev, _lib, _same_bits,
                                        _within)
from tests.test_ema_ops import RATES, _check_average, _ema_start
from tests.test_partial_ops import FROZEN_MAT, FROZEN_SEG, _groups, _job_table_groups
from tests.test_sgd_ops import WD, _job_table

gpu = pytest.mark.gpu

# betas as the kernel receives them (fp32); the references use the same fp32-rounded values (1 - beta is exact in fp32 for both)
B1, B2 = (float(np.float32(x)) for x in (0.9, 0.99))
MAX_AMBIGUOUS = 4
LION_GRID = [(clip, wd, step) for clip in ("active", "inactive", "none") for wd in (0.0, WD) for step in (1, 2)]


def lion_ref(p, g, m, sumsq, wd, lr=LR, b1=B1, b2=B2, max_norm=MAX_NORM):
    """fp64 restatement of optim.hip's lion_elem: gc = g coef with coef = min(1, max_norm / (sqrt(sumsq) + 1e-6)) (1 without
    sumsq); c = b1 m + (1 - b1) gc; u = sign(c) (0 at 0); p -= (lr wd) p; p -= lr u; m = b2 m + (1 - b2) gc from the old m.
    ``wd`` / ``lr`` may be per-element tensors.  Returns (p, m, m_mag, c, c_mag): m_mag / c_mag are the sizes of the terms that
    make up the new momentum and c."""
    p, g, m = (t.double() for t in (p, g, m))
    coef = 1.0 if sumsq is None else min(1.0, max_norm / (math.sqrt(sumsq) + 1e-6))
    gc = g * coef
    c = b1 * m + (1 - b1) * gc
    c_mag = b1 * m.abs() + (1 - b1) * gc.abs()
    u = (c > 0).double() - (c < 0).double()
    p = p - (lr * wd) * p
    p = p - lr * u
    m_mag = b2 * m.abs() + (1 - b2) * gc.abs()
    return p, b2 * m + (1 - b2) * gc, m_mag, c, c_mag


def ambiguous(ref):
    """Mask of the elements whose sign fp32 may decide differently: |c| <= 2^-20 c_mag in fp64 (c == 0 = c_mag -- a zero
    gradient on a zero momentum -- is NOT ambiguous: every product and the sum are exactly 0 in fp32 too)."""
    _, _, _, c, c_mag = ref
    return (c.abs() <= 2.0 ** -20 * c_mag) & (c_mag > 0)


def _lion_bounds(ref, wd, lr=LR):
    """Element bounds on (p, m) of the fp32 kernel against lion_ref.  m is a handful of fp32 roundings (clip coefficient, scaling,
    two products, one sum) of terms of size m_mag: 2^-20 of it, as for Adam's and SGD's state.  p with the right sign is two
    subtractions, each rounded to within U = 2^-24 of a value no larger than |p| + lr: 2 U |p| + 2 U lr; the decay term lr wd p
    is two more roundings of its own size: 2^-20 of it.  An ambiguous element may have taken the other sign (or none): 2 lr more."""
    p, _, m_mag, _, _ = ref
    bound = 2 * U * p.abs() + 2 * U * lr + 2.0 ** -20 * lr * wd * p.abs()
    return bound + ambiguous(ref).double() * 2 * lr, 2.0 ** -20 * m_mag


def _lion_state(n, step, clip, seed):
    """(p, g, m, sumsq or None) from the Adam tests' generator: gradient norm 10 x / 0.5 x max_norm; zero momentum at step 1 (the
    initial state; c is then (1 - b1) gc and the sign is the gradient's), an earlier step's momentum at step 2."""
    p, g, m, _, sumsq = _adam_state(n, step, clip, seed)
    return p, g, m, sumsq


def _checked_ref(tag, p0, g0, m0, sumsq, wd, lr=LR):
    """lion_ref, after the condition on the case itself: at most MAX_AMBIGUOUS ambiguous elements (asserted before any kernel
    result is looked at)."""
    ref = lion_ref(p0, g0, m0, sumsq, wd, lr=lr)
    count = int(ambiguous(ref).sum())
    assert count <= MAX_AMBIGUOUS, f"{tag}: {count} ambiguous elements; the case does not pin the sign"
    return ref


def _check_lion(tag, ref, wd, p, m, lr=LR, sel=None):
    bp, bm = _lion_bounds(ref, wd, lr)
    pick = (lambda t: t[sel]) if sel is not None else (lambda t: t)
    _within(pick(m.cpu()), pick(ref[1]), pick(bm), f"{tag} exp_avg")
    _within(pick(p.cpu()), pick(ref[0]), pick(bp), f"{tag} master")


class StockLion:
    """The stock loop the model-level tests compare with (tests/test_lion_gpu.py, tests/lion_ddp_child.py):
    ``clip_grad_norm_`` plus the three lines of the published algorithm in fp32 torch over detached twins of the parameters, fed
    the gradients it is handed, on whatever device they live on.  It also evaluates c in fp64 from its own tensors and counts,
    per element, the steps at which the sign was ambiguous (|c| <= 2^-20 (b1 |m| + (1 - b1) |gc|)).

    ``check`` is the comparison rule: first the share of elements that were ever ambiguous must be at most 1e-4 of the parameters
    (a condition on the case, asserted on this side alone); then every element must agree with the model's master within
    2 U |p| + 2 U lr (+ 2^-20 lr wd |p|) per step taken -- which forces every sign to agree -- plus 2 lr for every step at which
    it was ambiguous.  ``wd``: one value, or a dict by parameter name."""

    def __init__(self, start, lr, betas, wd=0.0, max_norm=1.0):
        self.twins = {n: torch.nn.Parameter(t.detach().clone()) for n, t in start.items()}
        self.m = {n: torch.zeros_like(t) for n, t in self.twins.items()}
        self.m_mag = {n: torch.zeros_like(t) for n, t in self.twins.items()}       # b2 m_mag + (1 - b2) |gc|: the momentum's terms
        self.flagged = {n: torch.zeros(t.shape, dtype=torch.int32, device=t.device) for n, t in self.twins.items()}
        self.lr, (self.b1, self.b2), self.max_norm = lr, betas, max_norm
        self.wd = wd if isinstance(wd, dict) else {n: wd for n in self.twins}
        self.steps, self.lr_sum, self.lr_max = 0, 0.0, 0.0

    @torch.no_grad()
    def step(self, grads, lr=None):
        """One step from ``grads`` (by name; copied); returns the gradient norm before the clip (None without a clip)."""
        lr = self.lr if lr is None else lr
        for n, t in self.twins.items():
            t.grad = grads[n].detach().clone()
        norm = None
        if self.max_norm is not None:
            norm = float(torch.nn.utils.clip_grad_norm_(list(self.twins.values()), self.max_norm))
        b1, b2 = self.b1, self.b2
        for n, t in self.twins.items():
            g, m = t.grad, self.m[n]
            c = m.double() * b1 + g.double() * (1 - b1)
            c_mag = m.double().abs() * b1 + g.double().abs() * (1 - b1)
            self.flagged[n] += ((c.abs() <= 2.0 ** -20 * c_mag) & (c_mag > 0)).int()
            t.data.mul_(1 - lr * self.wd[n])
            t.data.add_(torch.sign(m * b1 + g * (1 - b1)), alpha=-lr)
            m.lerp_(g, 1 - b2)
            self.m_mag[n].mul_(b2).add_(g.abs(), alpha=1 - b2)
        self.steps += 1
        self.lr_sum += lr
        self.lr_max = max(self.lr_max, lr)
        return norm

    def ambiguous_share(self):
        total = sum(t.numel() for t in self.twins.values())
        return sum(int((f > 0).sum()) for f in self.flagged.values()) / total

    def check(self, tag, masters):
        """``masters``: name -> the model's master of every parameter this loop follows."""
        share = self.ambiguous_share()
        assert share <= 1e-4, f"{tag}: {share:.2e} of the parameters had an ambiguous sign; the case does not pin the update"
        worst, wrong = 0.0, 0
        for n, t in self.twins.items():
            ref = t.detach().double()
            bound = 2 * U * (self.steps * ref.abs() + self.lr_sum) + 2.0 ** -20 * self.lr_sum * self.wd[n] * ref.abs() + \
                self.flagged[n].double() * 2 * self.lr_max
            err = (masters[n].detach().double() - ref).abs()
            worst = max(worst, float((err / bound).max()))
            wrong += int((err > bound).sum())
        print(f"[{tag}] {self.steps} steps, ambiguous share {share:.2e}; worst |fused - stock| / bound {worst:.3f}")
        assert wrong == 0, f"{tag}: {wrong} elements over the bound (worst ratio {worst:.3g}; a wrong sign is about lr / (2 U |p|))"


def _null(t):
    return c_void_p(t.data_ptr()) if t is not None else c_void_p(0)


def lion_call(form, p, g, m, p16, ss, wd=0.0, n=None, tables=None, groups=None, ema=None, rate=None, lr=LR, b1=B1, b2=B2):
    """One launch of the ``form`` ("flat" / "tiles" / "groups") entry point, its ``_ema`` twin when ``rate`` is given.
    ``tables`` = (jobs, njobs, tiles, seg_tab, seg_group); ``groups`` = a ce_optim_group array."""
    cl, ptr, stream = _lib()
    stem = "ce_lion_step" + {"flat": "", "tiles": "_tiles", "groups": "_groups"}[form]
    args = [ptr(p), ptr(g), _null(m), ptr(p16)]
    if form == "flat":
        args.append(c_long(n))
    else:
        jobs, njobs, tiles, seg_tab, seg_group = tables
        args += [_null(jobs), c_int(njobs), c_int(tiles), _null(seg_tab), c_int(seg_tab.shape[0] if seg_tab is not None else 0)]
        if form == "groups":
            args.append(_null(seg_group))
    args += [_null(ss), c_float(MAX_NORM)]
    if form == "groups":
        args += [groups, c_int(len(groups)), c_float(b1), c_float(b2)]
    else:
        args += [c_float(lr), c_float(b1), c_float(b2), c_float(wd)]
    if rate is not None:
        args += [_null(ema), c_float(rate)]
        stem += "_ema"
    rc = getattr(cl, stem)(*args, stream())
    torch.cuda.synchronize()
    assert rc == 0, cl.ce_last_error()


def _ss(sumsq):
    return torch.tensor([sumsq], device=DEV) if sumsq is not None else None


def _guarded(t, guard=6):
    return torch.cat([t, torch.full((guard,), 4.0)]).to(DEV)


# ---- 1. flat ----------------------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("n", [5, 7171, 1000003])
def test_lion_step_against_fp64(n):
    """``ce_lion_step`` (flat) over the grid clip active / inactive / off (sumsq NULL) x weight decay 0 / 0.1 x step 1 (zero
    momentum) / step 2, n with n % 4 != 0 and n % 2048 != 0: the momentum within 2^-20 of b2 |m| + (1 - b2) |gc| of lion_ref, the
    masters within 2 U |p| + 2 U lr (+ 2^-20 lr wd |p|) wherever the sign is not ambiguous -- which forces the sign -- the bf16
    mirror bit-equal to the masters' RNE cast, the gradient not written, six sentinels behind every buffer intact."""
    for clip, wd, step in LION_GRID:
        tag = f"lion n={n} clip={clip} wd={wd} step={step}"
        p0, g0, m0, sumsq = _lion_state(n, step, clip, n + step)
        ref = _checked_ref(tag, p0, g0, m0, sumsq, wd)
        p, g, m = _guarded(p0), _guarded(g0), _guarded(m0)
        p16 = torch.full((n + 6,), 4.0, device=DEV, dtype=torch.bfloat16)
        lion_call("flat", p, g, m, p16, _ss(sumsq), wd, n=n)
        _check_lion(tag, ref, wd, p[:n], m[:n])
        moved = (p[:n].cpu().double() - p0.double()).abs()
        assert bool((moved >= 0.5 * LR).all()), f"{tag}: a master with a non-zero c did not move by lr"
        assert _same_bits(p16[:n], p[:n].to(torch.bfloat16))
        assert torch.equal(g[:n].cpu(), g0)
        for t in (p, g, m):
            assert bool((t[n:] == 4.0).all())
        assert bool((p16[n:] == 4.0).all())


@gpu
@pytest.mark.parametrize("wd", [0.0, WD])
def test_lion_zero_gradient_on_zero_momentum_moves_by_the_decay_alone(wd):
    """Eight planted elements with g = m = 0 (one of them at the ragged end, one with p = -0.0): c is exactly 0, the sign is 0,
    so those masters change by the decay alone -- p - fl(fl(lr wd) p), the kernel's own two roundings, bit for bit -- and with
    weight decay 0 not at all, bit for bit; their momentum stays +0.  Everything else is within the bounds as usual."""
    n = 7171
    p0, g0, m0, sumsq = _lion_state(n, 2, "active", 41)
    planted = torch.tensor([0, 1, 2, 3, 1024, 4099, n - 2, n - 1])
    g0[planted], m0[planted] = 0.0, 0.0
    p0[1] = -0.0
    tag = f"lion planted zeros wd={wd}"
    ref = _checked_ref(tag, p0, g0, m0, sumsq, wd)
    p, g, m = _guarded(p0), _guarded(g0), _guarded(m0)
    p16 = torch.full((n + 6,), 4.0, device=DEV, dtype=torch.bfloat16)
    lion_call("flat", p, g, m, p16, _ss(sumsq), wd, n=n)
    _check_lion(tag, ref, wd, p[:n], m[:n])
    decay = torch.tensor(LR, dtype=torch.float32) * torch.tensor(wd, dtype=torch.float32)
    want = p0[planted] - decay * p0[planted] if wd != 0 else p0[planted]
    assert _same_bits(p[:n].cpu()[planted], want)
    assert _same_bits(m[:n].cpu()[planted], torch.zeros(8))
    assert _same_bits(p16[:n], p[:n].to(torch.bfloat16))


# ---- 2. tiles + segments ----------------------------------------------------------------------------------------------------------

def _fresh_tiles(n):
    p16 = torch.full((n,), 4.0, device=DEV, dtype=torch.bfloat16)
    wts = [torch.full((c, r), -4.0, device=DEV, dtype=torch.bfloat16) for _, r, c in TILE_MATS]
    return p16, wts


def _tile_tables(p16, wts):
    jobs, tiles = _job_table(TILE_MATS, p16, wts)
    return jobs, len(TILE_MATS), tiles, torch.tensor(TILE_SEGS, dtype=torch.int64).to(DEV), None


@gpu
def test_lion_step_tiles_against_fp64():
    """``ce_lion_step_tiles`` over the matrix / segment layout of test_adam_step_tiles_against_fp64 for the same grid: the same
    bounds, the mirror bit-equal to the masters' cast, every W^T copy bit-equal to the mirror's transpose, the 8 elements outside
    every matrix and segment untouched in p / m / mirror, the gradient not written."""
    n, N = TILE_N + 8, TILE_N
    for clip, wd, step in LION_GRID:
        tag = f"lion tiles clip={clip} wd={wd} step={step}"
        p0, g0, m0, sumsq = _lion_state(n, step, clip, 77 + step)
        ref = _checked_ref(tag, p0, g0, m0, sumsq, wd)
        p, g, m = _dev(p0, g0, m0)
        p16, wts = _fresh_tiles(n)
        lion_call("tiles", p, g, m, p16, _ss(sumsq), wd, tables=_tile_tables(p16, wts))
        _check_lion(tag, ref, wd, p, m, sel=slice(0, N))
        assert _same_bits(p16[:N], p[:N].to(torch.bfloat16))
        for t, t0 in ((p, p0), (m, m0)):
            assert _same_bits(t[N:].cpu(), t0[N:])
        assert torch.equal(g.cpu(), g0)
        assert bool((p16[N:] == 4.0).all())
        for (off, r, c), wt in zip(TILE_MATS, wts):
            assert _same_bits(wt, p16[off:off + r * c].view(r, c).t()), (r, c)


# ---- 3. the three forms -----------------------------------------------------------------------------------------------------------

@gpu
def test_lion_tiled_flat_and_segment_forms_are_bit_identical():
    """tests/test_optim_shared.py's check for the third rule: the flat kernel (over TILE_N + 3 elements, so its length is no
    multiple of 4), the tile + segment launch and a launch of segments only (the whole range cut into chunks of at most 2048)
    leave the same bits in the masters, the momentum and the bf16 mirror over LION_GRID; the table forms cover TILE_N and leave
    the three elements behind it alone."""
    N, n = TILE_N, TILE_N + 3
    all_segs = torch.tensor([(lo, min(lo + 2048, N)) for lo in range(0, N, 2048)], dtype=torch.int64).to(DEV)
    for clip, wd, step in LION_GRID:
        p0, g0, m0, sumsq = _lion_state(n, step, clip, 300 + step)
        out = {}
        for form in ("flat", "tiles", "segments"):
            p, g, m = _dev(p0, g0, m0)
            p16, wts = _fresh_tiles(n)
            if form == "flat":
                lion_call("flat", p, g, m, p16, _ss(sumsq), wd, n=n)
            elif form == "tiles":
                lion_call("tiles", p, g, m, p16, _ss(sumsq), wd, tables=_tile_tables(p16, wts))
            else:
                lion_call("tiles", p, g, m, p16, _ss(sumsq), wd, tables=(None, 0, 0, all_segs, None))
            out[form] = (p, m, p16)
        start = (p0, m0, torch.full((n,), 4.0, dtype=torch.bfloat16))
        for form in ("tiles", "segments"):
            for i, what in enumerate(("masters", "exp_avg", "bf16 mirror")):
                a, b = out[form][i], out["flat"][i]
                assert _same_bits(a[:N], b[:N]), (clip, wd, step, form, what, int((a[:N] != b[:N]).sum()))
                assert _same_bits(a[N:].cpu(), start[i][N:]), (clip, wd, step, form, what)
        assert bool((out["flat"][2][N:] != 4.0).all()), (clip, wd, step)          # the flat form did reach its ragged end
        assert not _same_bits(out["flat"][0][:N].cpu(), p0[:N])


# ---- 4. groups --------------------------------------------------------------------------------------------------------------------

# Two groups over the TILE_* layout, the 8 x 8 matrix and the segment (16452, 16500) frozen (in no table), as in
# tests/test_partial_ops.py: group 0 = LR with the grid's weight decay, group 1 = twice the rate with decay 0.05.
LR_B, WD_B = (float(np.float32(x)) for x in (LR * 2, 0.05))
G_MATS = [(mat, gr) for i, (mat, gr) in enumerate(zip(TILE_MATS, (1, 0, 0))) if i != FROZEN_MAT]
G_SEGS = [(seg, gr) for i, (seg, gr) in enumerate(zip(TILE_SEGS, (0, 1, 0, 1, 0))) if i != FROZEN_SEG]
SENTINEL_P, SENTINEL_M = 7.0, -7.0


def _two_group_scalars(n, rows):
    lr, wd, live = torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.bool)
    for (lo, hi), gr in [((off, off + r * c), gr) for (off, r, c), gr in G_MATS] + G_SEGS:
        assert not bool(live[lo:hi].any())
        lr[lo:hi], wd[lo:hi], live[lo:hi] = rows[gr][0], rows[gr][1], True
    return lr, wd, live


def _two_group_tables(p16, wts):
    jobs, tiles = _job_table_groups([mat for mat, _ in G_MATS], p16, [wt for i, wt in enumerate(wts) if i != FROZEN_MAT],
                                    [gr for _, gr in G_MATS])
    seg_tab = torch.tensor([s for s, _ in G_SEGS], dtype=torch.int64).to(DEV)
    seg_group = torch.tensor([gr for _, gr in G_SEGS], dtype=torch.int32).to(DEV)
    return jobs, len(G_MATS), tiles, seg_tab, seg_group


@gpu
def test_two_group_lion_against_fp64_and_frozen_ranges_untouched():
    """``ce_lion_step_groups`` with two groups (distinct lr and weight decay) over LION_GRID; the 8 x 8 matrix, one segment and the
    8 guard elements are in no table and hold NaN in the gradient and sentinels in p (7), m (-7), the mirror (4) and the frozen
    matrix's W^T copy (-4): they come back bit for bit.  Every updated element is within the bounds of lion_ref with ITS group's
    lr and weight decay; the mirror is the cast, W^T the transpose; ``decoupled`` set on both groups gives the same bits."""
    n = TILE_N + 8
    for clip, wd, step in LION_GRID:
        tag = f"lion groups clip={clip} wd={wd} step={step}"
        rows = [(LR, wd, 0), (LR_B, WD_B, 0)]
        lr_e, wd_e, live = _two_group_scalars(n, rows)
        dead = ~live
        p0, g0, m0, sumsq = _lion_state(n, step, clip, 177 + step)
        p0[dead], m0[dead] = SENTINEL_P, SENTINEL_M
        g_dev = g0.clone()
        g_dev[dead] = float("nan")
        ref = lion_ref(p0, g0, m0, sumsq, wd_e, lr=lr_e)
        assert int(ambiguous(ref)[live].sum()) <= MAX_AMBIGUOUS, tag
        outs = []
        for decoupled in (0, 1):
            p, g, m = _dev(p0, g_dev, m0)
            p16, wts = _fresh_tiles(n)
            lion_call("groups", p, g, m, p16, _ss(sumsq), tables=_two_group_tables(p16, wts),
                      groups=_groups([(lr, w, decoupled) for lr, w, _ in rows]))
            outs.append((p, m, p16, *wts))
        for a, b in zip(*outs):
            assert _same_bits(a, b), f"{tag}: the decoupled flag changed bits"
        p, m, p16, *wts = outs[0]
        for name, t, t0 in (("p", p, p0), ("m", m, m0)):
            assert _same_bits(t.cpu()[dead], t0[dead]), (tag, name)
        assert bool((p16.cpu()[dead] == 4.0).all()) and bool((wts[FROZEN_MAT] == -4.0).all()), tag
        bp, bm = _lion_bounds(ref, wd_e, lr_e)
        _within(m.cpu()[live], ref[1][live], bm[live], f"{tag} exp_avg")
        _within(p.cpu()[live], ref[0][live], bp[live], f"{tag} master")
        assert _same_bits(p16.cpu()[live], p.cpu()[live].to(torch.bfloat16)), tag
        for i, ((off, r, c), wt) in enumerate(zip(TILE_MATS, wts)):
            if i != FROZEN_MAT:
                assert _same_bits(wt, p16[off:off + r * c].view(r, c).t()), (tag, r, c)


@gpu
def test_one_group_lion_leaves_the_bits_of_the_ungrouped_step():
    """``ce_lion_step_groups`` with one group against ``ce_lion_step_tiles`` over LION_GRID on the TILE_* layout: masters, momentum,
    mirror, every W^T copy and the 8 guard elements bit for bit -- segment_group NULL and a table of zeros alike, ``decoupled``
    set or not."""
    n = TILE_N + 8
    zeros = torch.zeros(len(TILE_SEGS), dtype=torch.int32, device=DEV)
    for clip, wd, step in LION_GRID:
        p0, g0, m0, sumsq = _lion_state(n, step, clip, 77 + step)
        outs = []
        for form, seg_group, decoupled in (("tiles", None, 0), ("groups", None, 0), ("groups", zeros, 0), ("groups", None, 1)):
            p, g, m = _dev(p0, g0, m0)
            p16, wts = _fresh_tiles(n)
            tables = _tile_tables(p16, wts)[:4] + (seg_group,)
            lion_call(form, p, g, m, p16, _ss(sumsq), wd, tables=tables, groups=_groups([(LR, wd, decoupled)]))
            outs.append((p, m, p16, *wts))
        for other in outs[1:]:
            for i, (a, b) in enumerate(zip(other, outs[0])):
                assert _same_bits(a, b), (clip, wd, step, i)
        assert _same_bits(outs[1][0][TILE_N:].cpu(), p0[TILE_N:]) and bool((outs[1][2][TILE_N:] == 4.0).all())
        assert not _same_bits(outs[1][0][:TILE_N].cpu(), p0[:TILE_N])


# ---- 5. the _ema forms ------------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("step,clip", [(1, "none"), (2, "active")])
def test_lion_ema_forms(step, clip):
    """``ce_lion_step_ema`` / ``_tiles_ema`` / ``_groups_ema`` (one group) on the TILE_* layout for rates 1, 0.1 and 1e-4 with weight
    decay 0.1: masters, momentum, mirror and W^T copies carry the bits of the same form without ``_ema`` (which leaves the average
    alone); the average is bit-equal across the three forms, within tests/test_ema_ops.py's bound of ema_ref on the kernel's own
    masters (rate 1: their bits), and keeps its bits in the 8 elements that belong to nothing; the gradient is not written."""
    n, N = TILE_N + 8, TILE_N
    p0, g0, m0, sumsq = _lion_state(n, step, clip, 311 + step)
    e0 = _ema_start(p0, 311)
    for rate in RATES:
        averages = {}
        for form in ("flat", "tiles", "groups"):
            outs = []
            for with_ema in (False, True):
                p, g, m, e = _dev(p0, g0, m0, e0)
                p16, wts = _fresh_tiles(n)
                lion_call(form, p, g, m, p16, _ss(sumsq), WD, n=N, tables=_tile_tables(p16, wts), groups=_groups([(LR, WD, 0)]),
                          ema=e, rate=rate if with_ema else None)
                outs.append((p, m, p16, *wts, g, e))
            tag = f"lion ema {form} step={step} clip={clip} rate={rate}"
            for a, b in zip(outs[0][:-1], outs[1][:-1]):
                assert _same_bits(a, b), tag
            p, e = outs[1][0], outs[1][-1]
            assert _same_bits(outs[0][-1].cpu(), e0) and torch.equal(outs[1][-2].cpu(), g0), tag
            assert _same_bits(e[N:].cpu(), e0[N:]) and _same_bits(p[N:].cpu(), p0[N:]), tag
            assert not _same_bits(p[:N].cpu(), p0[:N]), tag
            _check_average(tag, e[:N], e0[:N].to(DEV), p[:N], rate)
            averages[form] = e
        for form in ("tiles", "groups"):
            assert _same_bits(averages[form], averages["flat"]), (step, clip, rate, form)
