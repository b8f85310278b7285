"""GPU, op level: the fused distillation head (``functional.DistillHeadFn`` on ``ce_distill_head_fwd/bwd`` + ``ce_rowdot_sum``) and
the row kernels of the materialised path (``ce_soft_xent_fwd/bwd``) against the fp64 reference of tests/distill_ref.py.  Shapes
(tests/distill_ref.SHAPES) are the smallest at which each path runs: a padded tile with an 8-wave-eligible similarity over
128-wide values, splits with float atomics, queries through ``sel``, the real pair's widths, every gradient accumulator.  Every
case prints fp32 eager torch's own error against the fp64 reference beside the kernel's."""
import ctypes

import numpy as np
import pytest
import torch

from tests import distill_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAMES = ("loss", "dq", "dk", "dlogit_scale")
BOUNDS = (1e-5, 2e-5, 2e-5, 2e-5)           # test_sigmoid_ops.py's, relative (dq / dk: relative L2)
SENTINEL = -7.5


def _rel(got, want):
    got, want = got.double().cpu(), want.double().cpu()
    return float((got - want).norm() / (want.norm() + 1e-300))


def _run_fn(q, k, ls, tq, tk, tls, sel, grad=1.3):
    from clip_event_amd.functional import DistillHeadFn
    qd, kd, lsd = (t.clone().to(DEV).requires_grad_(True) for t in (q, k, ls))
    loss = DistillHeadFn.apply(qd, kd, lsd, tq.to(DEV), tk.to(DEV), tls.to(DEV), None if sel is None else sel.to(DEV))
    (loss * grad).backward()
    torch.cuda.synchronize()
    return loss.detach(), qd.grad, kd.grad, lsd.grad


@pytest.mark.parametrize("shape,A,pair", R.CASES)
def test_distill_head_against_fp64_reference(shape, A, pair):
    """Loss 1e-5 relative, dq / dk 2e-5 relative L2, dlogit_scale 2e-5 relative, upstream gradient 1.3; the fp64 loss and
    |dlogit_scale| are at least 0.1 first, so the relative bounds mean something.

    (33, 33, 128, 256) at A = 0.3 with both scales ln 100 is the case that caught the teacher's forward sweep running on eight
    waves and its gradient sweeps on four (loss 1.36e-5, dlogit_scale 1.48e-5 then; 1.1e-7 / 3.5e-7 with one wave count for all
    sweeps of a similarity -- DESIGN 4h, numerical point 1)."""
    (q, k, tq, tk, sel, ls, tls), want = R.case_and_reference(shape, A, pair)
    assert float(want[0]) >= 0.1 and abs(float(want[3])) >= 0.1
    eager = R.reference(q, k, ls, tq, tk, tls, sel, grad=1.3, dtype=torch.float32)
    got = _run_fn(q, k, ls, tq, tk, tls, sel)
    errs = []
    for name, g, w, e in zip(NAMES, got, want, eager):
        errs.append(_rel(g, w))
        print(f"[distill {shape[:4]} A {A:g} scales {pair}] {name}: kernel rel {errs[-1]:.3e}, fp32 eager torch rel {_rel(e, w):.3e}, "
              f"reference {float(w.norm()):.6e}")
    if sel is not None:                                           # rows that are no query get no gradient
        rest = torch.ones(q.shape[0], dtype=torch.bool)
        rest[sel] = False
        assert float(got[1].cpu()[rest].abs().max()) == 0.0
    for name, err, bound in zip(NAMES, errs, BOUNDS):
        assert err < bound, (name, err, bound)


def _entropy(tq, tk, tls, sel):
    T = R.logits(tq, tk, tls, sel)
    return float(-(T.softmax(dim=1) * T.log_softmax(dim=1)).sum(dim=1).mean())


def test_teacher_equal_to_student_gives_its_entropy_and_no_gradient():
    """Teacher == student at the same scale: the loss is the teacher's entropy (1e-5 relative) and |dq| is below 1e-4 of what an
    independent teacher of the same shape gives."""
    shape = (40, 97, 256, 256, None)
    q, k, tq, tk, sel = R.make_case(*shape, A=0.3)
    ls = torch.tensor(R.SCALE_PAIRS[1][0])
    same = _run_fn(q, k, ls, q, k, ls, sel)
    other = _run_fn(q, k, ls, tq, tk, ls, sel)
    H = _entropy(q, k, ls, sel)
    print(f"[distill self] loss {float(same[0]):.7f}, entropy {H:.7f}; |dq| {float(same[1].norm()):.3e} against {float(other[1].norm()):.3e}, "
          f"|dk| {float(same[2].norm()):.3e} against {float(other[2].norm()):.3e}")
    assert H > 0.1 and abs(float(same[0]) - H) < 1e-5 * H
    assert float(same[1].norm()) < 1e-4 * float(other[1].norm())
    assert float(same[2].norm()) < 1e-4 * float(other[2].norm())


def test_forward_loss_repeats_bit_for_bit():
    """The split shape: two forwards on the same inputs return the same bits.  v is accumulated by float atomics across the
    splits and may differ in its last bits from run to run; the loss is built on per-split row shares stored plainly and added
    in index order, and on row terms summed in index order."""
    shape = R.SHAPES[1]
    (q, k, tq, tk, sel, ls, tls), _ = R.case_and_reference(shape, 0.0, 0)
    a = _abi_fwd(*_normalised(q, k, tq, tk), ls, tls, None, shape[0], shape[1])
    b = _abi_fwd(*_normalised(q, k, tq, tk), ls, tls, None, shape[0], shape[1])
    assert torch.equal(a["loss"].view(torch.int32), b["loss"].view(torch.int32)), (float(a["loss"]), float(b["loss"]))


def _normalised(*ms):
    return tuple(torch.nn.functional.normalize(m.double(), dim=-1).float() for m in ms)


def _guarded(rows, cols, fill=0.0, guard=2):
    """A [rows, cols] device buffer with ``guard`` sentinel rows behind it: (whole, view)."""
    whole = torch.full((rows + guard, cols), SENTINEL, device=DEV)
    whole[:rows] = fill
    return whole, whole[:rows]


def _padded(m, ld, extra_rows=0):
    """``m`` in a NaN-filled [rows + extra_rows, ld] device buffer: NaN behind every row's width and behind the last row."""
    buf = torch.full((m.shape[0] + extra_rows, ld), float("nan"), device=DEV)
    buf[:m.shape[0], :m.shape[1]] = m.to(DEV)
    return buf


def _abi_fwd(qn, kn, tqn, tkn, ls, tls, sel, nq, nk, pad=0, grad=None):
    """``ce_distill_head_fwd`` (and ``_bwd`` + ``ce_rowdot_sum`` when ``grad`` is given) on normalised features as given, every
    output in a sentinel-guarded buffer; ``pad`` > 0: inputs in NaN-padded buffers with leading dimension E + pad and ``pad``
    NaN rows behind the keys."""
    from clip_event_amd._lib import check, lib, ptr, stream
    cl = lib()
    Es, Et = qn.shape[1], tqn.shape[1]
    bufs = [_padded(m, m.shape[1] + pad, extra) if pad else m.to(DEV).contiguous()
            for m, extra in ((qn, 0), (kn, pad), (tqn, 0), (tkn, pad))]
    qb, kb, tqb, tkb = bufs
    lsd, tlsd = ls.reshape(1).to(DEV), tls.reshape(1).to(DEV)
    seld = None if sel is None else sel.to(DEV)
    stats_w, stats = _guarded(2, 2 * nq, float("nan"))             # lse_s | lse_t, each [nq][2]
    v_w, v = _guarded(nq, Es)
    loss = torch.full((3,), SENTINEL, device=DEV)
    ws = torch.empty(cl.ce_distill_head_workspace_bytes(nq), dtype=torch.uint8, device=DEV)
    args = (ptr(qb), qb.stride(0), ptr(seld), nq, ptr(kb), kb.stride(0), nk, Es, ptr(lsd), ptr(tqb), tqb.stride(0), ptr(tkb),
            tkb.stride(0), Et, ptr(tlsd))
    check(cl.ce_distill_head_fwd(*args, ptr(stats[0]), ptr(stats[1]), ptr(v), ptr(loss[1:2]), ptr(ws), stream()), "ce_distill_head_fwd")
    out = {}
    if grad is not None:
        g = torch.tensor([grad], device=DEV)
        dq_w, dq = _guarded(qn.shape[0], Es)
        dk_w, dk = _guarded(nk, Es)
        dls = torch.zeros(1, device=DEV)
        check(cl.ce_distill_head_bwd(*args, ptr(stats[0]), ptr(stats[1]), ptr(v), ptr(g), ptr(dq), ptr(dk), stream()),
              "ce_distill_head_bwd")
        # the row-dot over the compact gradient and the (possibly padded) features
        check(cl.ce_rowdot_sum(ptr(qb), qb.stride(0), ptr(dq), Es, qn.shape[0], Es, ptr(dls), stream()), "ce_rowdot_sum")
        torch.cuda.synchronize()
        for w, rows in ((dq_w, qn.shape[0]), (dk_w, nk)):
            assert bool((w[rows:] == SENTINEL).all())
        out.update(dq=dq.cpu(), dk=dk.cpu(), dls=dls.cpu())
    torch.cuda.synchronize()
    assert bool((stats_w[2:] == SENTINEL).all()) and bool((v_w[nq:] == SENTINEL).all())
    assert float(loss[0]) == SENTINEL and float(loss[2]) == SENTINEL
    out.update(loss=loss[1:2].cpu(), v=v.cpu(), lse=stats.cpu())
    return out


@pytest.mark.parametrize("shape", [R.SHAPES[0], R.SHAPES[2]], ids=["33x33", "sel"])
def test_nothing_past_an_edge_is_read(shape):
    """Padded leading dimensions with NaN behind every row's width and NaN rows behind nk: the results are the fp64 reference's
    (on the normalised features) at the op bounds, and no NaN anywhere; every output's guard rows keep their sentinel."""
    nq, nk, Es, Et, rows_q = shape
    q, k, tq, tk, sel = R.make_case(nq, nk, Es, Et, rows_q, A=0.3, seed_extra=5)
    ls, tls = (torch.tensor(v) for v in R.SCALE_PAIRS[1])
    qn, kn, tqn, tkn = _normalised(q, k, tq, tk)
    got = _abi_fwd(qn, kn, tqn, tkn, ls, tls, sel, nq, nk, pad=4, grad=1.3)
    # reference w.r.t. the NORMALISED features: unit rows pass through the reference's normalisation as x - x <x, g> ...
    leaves = [t.double().requires_grad_(True) for t in (qn, kn, ls)]
    qs, tqs = (leaves[0] if sel is None else leaves[0][sel]), (tqn if sel is None else tqn[sel]).double()
    S = leaves[2].exp() * qs @ leaves[1].t()
    T = tls.double().exp() * tqs @ tkn.double().t()
    loss = R.distill_loss_from_logits(S, T)
    (loss * 1.3).backward()
    want = (loss.detach(), leaves[0].grad, leaves[1].grad, leaves[2].grad)
    for name, g, w, bound in zip(NAMES, (got["loss"], got["dq"], got["dk"], got["dls"]), want, BOUNDS):
        assert bool(torch.isfinite(g).all()), name
        err = _rel(g.reshape(w.shape), w)
        print(f"[distill padded {shape[:4]}] {name}: rel {err:.3e}")
        assert err < bound, (name, err, bound)


@pytest.mark.parametrize("shape,A,pair", [(R.SHAPES[0], 0.3, 0), (R.SHAPES[2], 0.3, 1), (R.SHAPES[1], 0.0, 2)], ids=["33x33", "sel", "97"])
def test_soft_cross_entropy_rows_against_fp64_reference(shape, A, pair):
    """``ce_soft_xent_fwd/bwd`` on materialised logits: loss 1e-5 relative, dlogits 2e-5 relative L2 against fp64 autograd on the
    same (fp32-rounded) logits, rows through ``sel`` where the case has it; rows not selected get no gradient."""
    from clip_event_amd.losses import soft_cross_entropy
    (q, k, tq, tk, sel, ls, tls), _ = R.case_and_reference(shape, A, pair)
    S = R.logits(q, k, ls).float()                      # every row of q: sel picks among them
    T = R.logits(tq, tk, tls).float()
    Sd = S.double().requires_grad_(True)
    rows = slice(None) if sel is None else sel
    want = R.distill_loss_from_logits(Sd[rows], T.double()[rows])
    (want * 1.3).backward()
    x = S.to(DEV).requires_grad_(True)
    loss = soft_cross_entropy(x, T.to(DEV), None if sel is None else sel.to(DEV))
    (loss * 1.3).backward()
    torch.cuda.synchronize()
    e_loss, e_grad = _rel(loss.detach(), want.detach()), _rel(x.grad, Sd.grad)
    print(f"[soft xent {shape[:4]}] loss rel {e_loss:.3e}, dlogits rel-L2 {e_grad:.3e}")
    assert float(want) >= 0.1 and e_loss < 1e-5 and e_grad < 2e-5
    if sel is not None:
        rest = torch.ones(S.shape[0], dtype=torch.bool)
        rest[sel] = False
        assert float(x.grad.cpu()[rest].abs().max()) == 0.0


def test_arguments_are_checked_before_any_launch():
    from clip_event_amd._lib import lib
    cl = lib()
    one = torch.zeros(1024, device=DEV)
    p = ctypes.c_void_p(one.data_ptr())
    tail = (p, p, p, p, p, None)
    rc = cl.ce_distill_head_fwd(p, 96, None, 2, p, 96, 2, 96, p, p, 128, p, 128, 128, p, *tail)
    assert rc != 0 and b"multiple of 128" in cl.ce_last_error()
    rc = cl.ce_distill_head_fwd(p, 128, None, 2, p, 128, 2, 128, p, p, 128, p, 128, 1152, p, *tail)
    assert rc != 0 and b"Et must be" in cl.ce_last_error()
    rc = cl.ce_distill_head_fwd(p, 128, None, 2, p, 128, 2, 128, p, p, 128, p, 128, 256, p, *tail)
    assert rc != 0 and b"leading dimensions" in cl.ce_last_error()
    rc = cl.ce_distill_head_fwd(p, 128, None, 2, p, 128, 2, 128, p, None, 128, p, 128, 128, p, *tail)
    assert rc != 0 and b"null" in cl.ce_last_error()
    rc = cl.ce_distill_head_bwd(p, 128, None, 2, p, 128, 2, 128, p, p, 128, p, 128, 128, p, p, p, p, p, p, None, None)
    assert rc != 0 and b"null" in cl.ce_last_error()
    rc = cl.ce_rowdot_sum(p, 64, p, 128, 2, 128, p, None)
    assert rc != 0 and b"bad shape" in cl.ce_last_error()
    rc = cl.ce_soft_xent_fwd(p, 8, None, 8, None, p, p, p, 2, 8, None)
    assert rc != 0 and b"null" in cl.ce_last_error()
