"""GPU, op level: the fused sigmoid pairwise head (``functional.SigmoidHeadFn`` on ``ce_sigmoid_head_fwd/bwd``) against the fp64
reference of tests/sigmoid_ref.py.  Shapes are the smallest at which each path of the kernel runs: one ragged block each way, a
second block of one row, many splits (float atomics across them), the 8-wave form, the 4-wave form at the LDS limit.  Every case
also prints fp32 eager torch's own error against the fp64 reference, the yardstick for "summation order only"."""
import ctypes

import numpy as np
import pytest
import torch

from tests.sigmoid_ref import reference

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LOGIT_SCALE = float(np.log(1 / 0.07))
SHAPES = [(5, 7, 128, False), (33, 70, 128, True), (70, 333, 128, True), (40, 96, 256, False), (37, 65, 768, True),
          (9, 130, 1024, False)]


def _case(nq, nk, E, use_sel, seed_extra=0):
    """Raw features, distinct labels, and for half of the queries a key next to the query (k[label] = q + 0.1 noise): positives
    reach x ~ +14 + bias, the other positives and all negatives stay near the bias, so both saturated regimes occur."""
    rng = np.random.default_rng(nq * 31 + nk + E + seed_extra)
    rows_q = nq + 9 if use_sel else nq
    q = torch.from_numpy(rng.standard_normal((rows_q, E)).astype(np.float32))
    k = torch.from_numpy(rng.standard_normal((nk, E)).astype(np.float32))
    sel = torch.from_numpy(rng.permutation(rows_q)[:nq].astype(np.int64)) if use_sel else None
    labels = torch.from_numpy(rng.permutation(nk)[:rows_q].astype(np.int64))
    rows = (sel if sel is not None else torch.arange(nq))[::2]
    k[labels[rows]] = q[rows] + 0.1 * torch.from_numpy(rng.standard_normal((len(rows), E)).astype(np.float32))
    return q, k, labels, sel


def _rel(got, want):
    got, want = got.double().cpu(), want.double().cpu()
    return float((got - want).norm() / (want.norm() + 1e-300))


@pytest.mark.parametrize("bias", [-10.0, 0.0])
@pytest.mark.parametrize("nq,nk,E,use_sel", SHAPES)
def test_sigmoid_head_against_fp64_reference(nq, nk, E, use_sel, bias):
    """Loss 1e-5 relative, dq / dk 2e-5 relative L2, dlogit_scale / dlogit_bias 2e-5 relative (the bounds of
    test_fused_infonce_against_pytorch for this sweep), upstream gradient 1.3."""
    from clip_event_amd.functional import SigmoidHeadFn
    q, k, labels, sel = _case(nq, nk, E, use_sel)
    ls, lb = torch.tensor(LOGIT_SCALE), torch.tensor(bias)
    want = reference(q, k, ls, lb, labels, sel, grad=1.3)
    eager = reference(q, k, ls, lb, labels, sel, grad=1.3, dtype=torch.float32)
    qd, kd, lsd, lbd = (t.clone().to(DEV).requires_grad_(True) for t in (q, k, ls, lb))
    loss = SigmoidHeadFn.apply(qd, kd, lsd, lbd, labels.to(DEV), None if sel is None else sel.to(DEV))
    (loss * 1.3).backward()
    torch.cuda.synchronize()
    got = (loss.detach(), qd.grad, kd.grad, lsd.grad, lbd.grad)
    names = ("loss", "dq", "dk", "dlogit_scale", "dlogit_bias")
    bounds = (1e-5, 2e-5, 2e-5, 2e-5, 2e-5)
    errs = []
    for name, g, w, e in zip(names, got, want, eager):
        errs.append(_rel(g, w))
        print(f"[sigmoid {nq}x{nk}x{E} bias {bias:g}] {name}: kernel rel {errs[-1]:.3e}, fp32 eager torch rel {_rel(e, w):.3e}, "
              f"reference {float(w.norm()):.6e}")
    if use_sel:                                                   # rows that are no query get no gradient
        rest = torch.ones(q.shape[0], dtype=torch.bool)
        rest[sel] = False
        assert float(qd.grad.cpu()[rest].abs().max()) == 0.0
    for name, err, bound in zip(names, errs, bounds):
        assert err < bound, (name, err, bound)


def test_forward_loss_repeats_bit_for_bit():
    """The 11-split shape: two forwards on the same inputs return the same bits (partials per workgroup, summed in a fixed
    order; no float atomics on the loss)."""
    from clip_event_amd.functional import SigmoidHeadFn
    q, k, labels, sel = _case(70, 333, 128, True)
    args = (q.to(DEV), k.to(DEV), torch.tensor(LOGIT_SCALE, device=DEV), torch.tensor(-10.0, device=DEV), labels.to(DEV), sel.to(DEV))
    losses = [SigmoidHeadFn.apply(*args) for _ in range(2)]
    torch.cuda.synchronize()
    a, b = (t.cpu().view(torch.int32) for t in losses)
    assert torch.equal(a, b), (float(losses[0]), float(losses[1]))


def _abi_run(qn, kn_buf, nk, labels, bias):
    """``ce_sigmoid_head_fwd/bwd`` on normalised features as given, ``nk`` rows of ``kn_buf`` declared."""
    from clip_event_amd._lib import check, lib, ptr, stream
    cl = lib()
    nq, E = qn.shape
    ls, lb = torch.tensor([LOGIT_SCALE], device=DEV), torch.tensor([bias], device=DEV)
    g = torch.tensor([1.3], device=DEV)
    loss = torch.full((1,), float("nan"), device=DEV)
    ws = torch.empty(cl.ce_sigmoid_head_workspace_bytes(nq, nk), dtype=torch.uint8, device=DEV)
    check(cl.ce_sigmoid_head_fwd(ptr(qn), E, None, nq, ptr(kn_buf), E, nk, E, ptr(ls), ptr(lb), ptr(labels), ptr(loss), ptr(ws),
                                 stream()), "ce_sigmoid_head_fwd")
    dq, dk, ds = torch.zeros_like(qn), torch.zeros_like(kn_buf), torch.zeros(2, device=DEV)
    check(cl.ce_sigmoid_head_bwd(ptr(qn), E, None, nq, ptr(kn_buf), E, nk, E, ptr(ls), ptr(lb), ptr(labels), ptr(g), ptr(dq), ptr(dk),
                                 ptr(ds[0:1]), ptr(ds[1:2]), stream()), "ce_sigmoid_head_bwd")
    torch.cuda.synchronize()
    return loss.cpu(), dq.cpu(), dk.cpu(), ds.cpu()


@pytest.mark.parametrize("bias", [-10.0, 0.0])
def test_rows_behind_nk_are_not_read_into_the_result(bias):
    """nk = 33 (a second key block with ONE live row): the same problem with a 34th key row appended to the buffer -- a large
    finite row -- and nk still passed as 33 gives the same loss bits and the same gradients, the appended row gets no gradient,
    and the loss is the fp64 reference's: neither the padded tile rows (zeros, softplus(0) = log 2 each) nor memory behind the
    declared rows enters the loss, dlogit_bias or dlogit_scale."""
    nq, nk, E = 20, 33, 128
    q, k, labels, _ = _case(nq, nk, E, False, seed_extra=7)
    qn = torch.nn.functional.normalize(q, dim=-1).to(DEV).contiguous()
    kn = torch.nn.functional.normalize(k, dim=-1).to(DEV).contiguous()
    kn34 = torch.cat([kn, torch.full((1, E), 3.0, device=DEV)], dim=0).contiguous()
    a = _abi_run(qn, kn, nk, labels.to(DEV), bias)
    b = _abi_run(qn, kn34, nk, labels.to(DEV), bias)
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)), (float(a[0]), float(b[0]))
    assert float(b[2][nk].abs().max()) == 0.0
    # gradients: plain stores when unsplit, float atomics across splits -- equal to summation order
    for name, x, y in (("dq", a[1], b[1]), ("dk", a[2], b[2][:nk]), ("dscale, dbias", a[3], b[3])):
        assert _rel(y, x) < 1e-6, name
    want = reference(q, k, torch.tensor(LOGIT_SCALE), torch.tensor(bias), labels, None, grad=1.3)
    print(f"[sigmoid padding bias {bias:g}] loss {float(a[0]):.7f}, fp64 reference {float(want[0]):.7f}, "
          f"a padded tile would add {(64 - nk) * np.log(2.0):.3f} per query row")
    assert abs(float(a[0]) - float(want[0])) < 1e-5 * abs(float(want[0]))
    assert abs(float(a[3][1]) - float(want[4])) < 2e-5 * abs(float(want[4]))
    assert abs(float(a[3][0]) - float(want[3])) < 2e-5 * abs(float(want[3]))


def test_arguments_are_checked_before_any_launch():
    from clip_event_amd._lib import lib
    cl = lib()
    one = torch.zeros(256, device=DEV)
    idx = torch.zeros(4, dtype=torch.int64, device=DEV)
    p = ctypes.c_void_p(one.data_ptr())
    rc = cl.ce_sigmoid_head_fwd(p, 96, None, 2, p, 96, 2, 96, p, p, ctypes.c_void_p(idx.data_ptr()), p, p, None)
    assert rc != 0 and b"multiple of 128" in cl.ce_last_error()
    rc = cl.ce_sigmoid_head_fwd(p, 128, None, 2, p, 128, 2, 128, p, None, ctypes.c_void_p(idx.data_ptr()), p, p, None)
    assert rc != 0 and b"null" in cl.ce_last_error()
