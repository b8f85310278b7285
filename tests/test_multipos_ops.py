"""GPU, op level: group-id targets on the fused head (``functional.MultiPosHeadFn`` on ``ce_multipos_head_fwd/bwd``, the group
form of ``SigmoidHeadFn`` on ``ce_sigmoid_head_group_fwd/bwd``) and on materialised logits (``ce_multipos_xent_fwd/bwd``) against
the fp64 reference of tests/multipos_ref.py.  Shapes are tests/test_sigmoid_ops.py's: one ragged block each way, a second block
of one row, many splits, the 8-wave form, the 4-wave form at the LDS limit.  Every case prints fp32 eager torch's own error
against the fp64 reference next to the kernel's before it asserts."""
import ctypes

import numpy as np
import pytest
import torch

from tests.multipos_ref import multipos_loss_from_logits, positives, reference, sigmoid_reference

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LOGIT_SCALE = float(np.log(1 / 0.07))
SHAPES = [(5, 7, 128, False), (33, 70, 128, True), (70, 333, 128, True), (40, 96, 256, False), (37, 65, 768, True),
          (9, 130, 1024, False)]
PATTERNS = ["one", "layout22", "scattered", "allkeys", "negative_and_unmatched", "highbits"]
HIGH = 1 << 32


def _rel(got, want):
    got, want = got.double().cpu(), want.double().cpu()
    return float((got - want).norm() / (want.norm() + 1e-300))


def _groups(pattern, rng, rows_q, nk, first, second):
    """(gq [rows_q], gk [nk]) int64.  ``first`` / ``second`` are the source rows of queries 0 and 1.  The base is one positive per row: query row s has
    id 100 + s, one key (a random distinct one) carries it, every other key -1."""
    labels = rng.permutation(nk)[:rows_q]
    gq = np.arange(rows_q, dtype=np.int64) + 100
    gk = np.full(nk, -1, dtype=np.int64)
    gk[labels] = gq
    if pattern == "layout22":                                   # texts 4i .. 4i+3 belong to image i, the first two are positives
        gq = np.arange(rows_q, dtype=np.int64)
        c = np.arange(nk, dtype=np.int64)
        gk = np.where(c % 4 < 2, c // 4, -1)
    elif pattern == "scattered":                                # first block, a middle block and the last key: other splits at 333 keys
        gk[[1, nk // 2, nk - 1]] = gq[first]
    elif pattern == "allkeys":                                  # every key is a positive of query 0, of nobody else
        gk[:] = 777
        gq[first] = 777
    elif pattern == "negative_and_unmatched":                   # -1 queries while -1 keys exist; ids no key carries
        gq[0::3] = -1
        gq[1::3] = 10_000 + np.arange(len(gq[1::3]))
        assert (gk == -1).any()
    elif pattern == "highbits":                                 # equal in the low 32 bits
        gk[labels[first]], gk[labels[second]] = 5, 5 + HIGH
        gq[first], gq[second] = 5, 5 + HIGH
        spare = np.flatnonzero(gk == -1)[0]
        gk[spare] = 5 + 2 * HIGH
    return torch.from_numpy(gq), torch.from_numpy(gk)


def _case(nq, nk, E, use_sel, pattern, seed_extra=0):
    """Raw features and group ids; for every second query (the odd ones) that has positives these lie next to it (k = q + 0.3
    noise): peaked and flat rows both occur, and no pattern is left with peaked rows only -- there the loss is a difference of
    two numbers near 14 that agree to five digits, which no fp32 arithmetic resolves to 1e-5 of itself."""
    rng = np.random.default_rng(nq * 31 + nk + E + seed_extra + 7 * PATTERNS.index(pattern))
    rows_q = nq + 9 if use_sel else nq
    q = torch.from_numpy(rng.standard_normal((rows_q, E)).astype(np.float32))
    k = torch.from_numpy(rng.standard_normal((nk, E)).astype(np.float32))
    sel = torch.from_numpy(rng.permutation(rows_q)[:nq].astype(np.int64)) if use_sel else None
    first, second = (int(sel[0]), int(sel[1])) if use_sel else (0, 1)
    gq, gk = _groups(pattern, rng, rows_q, nk, first, second)
    if pattern != "allkeys":
        for s in (sel if sel is not None else torch.arange(nq))[1::2].tolist():
            cols = torch.nonzero((gk == gq[s]) & (gq[s] >= 0)).flatten()
            if len(cols):
                k[cols] = q[s] + 0.3 * torch.from_numpy(rng.standard_normal((len(cols), E)).astype(np.float32))
    return q, k, gq, gk, sel


def _abi_forward(qn, k_buf, nk, gq, gk_buf, sel):
    """``ce_multipos_head_fwd`` on normalised features as given, ``nk`` rows of ``k_buf`` declared: (loss, lse, invpos)."""
    from clip_event_amd._lib import check, lib, ptr, stream
    cl = lib()
    E = qn.shape[1]
    nq = qn.shape[0] if sel is None else sel.shape[0]
    ls = torch.tensor([LOGIT_SCALE], device=DEV)
    loss = torch.zeros(1, device=DEV)
    lse, invpos = torch.full((nq,), float("nan"), device=DEV), torch.full((nq,), float("nan"), device=DEV)
    ws = torch.empty(cl.ce_multipos_head_workspace_bytes(nq), dtype=torch.uint8, device=DEV)
    check(cl.ce_multipos_head_fwd(ptr(qn), E, ptr(sel), nq, ptr(k_buf), E, nk, E, ptr(ls), ptr(gq), ptr(gk_buf), ptr(lse), ptr(invpos),
                                  ptr(loss), ptr(ws), stream()), "ce_multipos_head_fwd")
    return loss, lse, invpos


def _abi_backward(qn, k_buf, nk, gq, gk_buf, sel, lse, invpos, grad=1.3):
    from clip_event_amd._lib import check, lib, ptr, stream
    E = qn.shape[1]
    nq = qn.shape[0] if sel is None else sel.shape[0]
    ls, g = torch.tensor([LOGIT_SCALE], device=DEV), torch.tensor([grad], device=DEV)
    dq, dk, ds = torch.zeros_like(qn), torch.zeros_like(k_buf), torch.zeros(1, device=DEV)
    check(lib().ce_multipos_head_bwd(ptr(qn), E, ptr(sel), nq, ptr(k_buf), E, nk, E, ptr(ls), ptr(gq), ptr(gk_buf), ptr(lse),
                                     ptr(invpos), ptr(g), ptr(dq), ptr(dk), ptr(ds), stream()), "ce_multipos_head_bwd")
    torch.cuda.synchronize()
    return dq, dk, ds


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("nq,nk,E,use_sel", SHAPES)
def test_multipos_head_against_fp64_reference(nq, nk, E, use_sel, pattern):
    """Loss, lse and invpos 1e-5 relative, dq / dk 2e-5 relative L2, dlogit_scale within 2e-5 sum |G x| (the sum cancels: with
    every row at its optimum it is zero), rows without a positive exactly zero in dq.  Upstream gradient 1.3."""
    from clip_event_amd.functional import MultiPosHeadFn, _l2norm
    q, k, gq, gk, sel = _case(nq, nk, E, use_sel, pattern)
    ls = torch.tensor(LOGIT_SCALE)
    want = reference(q, k, ls, gq, gk, sel, grad=1.3)
    eager = reference(q, k, ls, gq, gk, sel, grad=1.3, dtype=torch.float32)
    qd, kd, lsd = (t.clone().to(DEV).requires_grad_(True) for t in (q, k, ls))
    seld = None if sel is None else sel.to(DEV)
    loss = MultiPosHeadFn.apply(qd, kd, lsd, gq.to(DEV), gk.to(DEV), seld)
    (loss * 1.3).backward()
    with torch.no_grad():
        loss_abi, lse, invpos = _abi_forward(_l2norm(q.to(DEV))[0], _l2norm(k.to(DEV))[0], nk, gq.to(DEV), gk.to(DEV), seld)
    torch.cuda.synchronize()
    tag = f"[multipos {nq}x{nk}x{E} {pattern}]"
    names = ("loss", "dq", "dk")
    errs = {}
    for name, g, w, e in zip(names, (loss.detach(), qd.grad, kd.grad), want, eager):
        errs[name] = _rel(g, w)
        print(f"{tag} {name}: kernel rel {errs[name]:.3e}, fp32 eager torch rel {_rel(e, w):.3e}, reference {float(w.norm()):.6e}")
    errs["lse"], errs["invpos"] = _rel(lse, want[4]), _rel(invpos, want[5])
    print(f"{tag} lse rel {errs['lse']:.3e}, invpos rel {errs['invpos']:.3e}, live rows {int((want[5] > 0).sum())} of {nq}")
    dls_err, mag = abs(float(lsd.grad) - float(want[3])), float(want[6])
    print(f"{tag} dlogit_scale: kernel {float(lsd.grad):.6e}, reference {float(want[3]):.6e}, |err| / sum|G x| {dls_err / max(mag, 1e-300):.3e}, "
          f"fp32 eager torch {abs(float(eager[3]) - float(want[3])) / max(mag, 1e-300):.3e}")
    assert torch.equal(loss_abi.cpu().reshape(()).view(torch.int32), loss.detach().cpu().view(torch.int32))
    assert int((want[5] > 0).sum()) >= 1
    # rows that are no query, and queries without a positive, get exactly nothing
    src = sel if sel is not None else torch.arange(nq)
    dead = torch.ones(q.shape[0], dtype=torch.bool)
    dead[src[want[5] > 0]] = False
    if bool(dead.any()):
        assert float(qd.grad.cpu()[dead].abs().max()) == 0.0
    assert torch.equal(invpos.cpu() == 0, want[5] == 0)
    for name, bound in (("loss", 1e-5), ("lse", 1e-5), ("invpos", 1e-5), ("dq", 2e-5), ("dk", 2e-5)):
        assert errs[name] < bound, (name, errs[name], bound)
    assert dls_err <= 2e-5 * mag, (dls_err, mag)


def test_rows_behind_nk_are_neither_counted_nor_read():
    """nk = 33 (a second key block with ONE live row): the key buffer and the id buffer go on behind row 33 with NaN features
    and ids that MATCH queries.  Nothing changes: same loss bits, same lse / invpos bits, gradients equal to summation order and
    finite, no gradient behind row 33."""
    from clip_event_amd.functional import _l2norm
    nq, nk, E = 20, 33, 128
    q, k, gq, gk, _ = _case(nq, nk, E, False, "layout22", seed_extra=7)
    qn, kn = _l2norm(q.to(DEV))[0], _l2norm(k.to(DEV))[0]
    tail = 31
    kn_long = torch.cat([kn, torch.full((tail, E), float("nan"), device=DEV)], dim=0).contiguous()
    gk_long = torch.cat([gk, torch.arange(tail) % nq]).to(DEV)                # ids of live queries
    gqd, gkd = gq.to(DEV), gk.to(DEV)
    a = _abi_forward(qn, kn, nk, gqd, gkd, None)
    b = _abi_forward(qn, kn_long, nk, gqd, gk_long, None)
    for x, y in zip(a, b):
        assert torch.equal(x.cpu().view(torch.int32), y.cpu().view(torch.int32))
    ga = _abi_backward(qn, kn, nk, gqd, gkd, None, a[1], a[2])
    gb = _abi_backward(qn, kn_long, nk, gqd, gk_long, None, b[1], b[2])
    assert float(gb[1][nk:].abs().max()) == 0.0
    for name, x, y in (("dq", ga[0], gb[0]), ("dk", ga[1], gb[1][:nk]), ("dlogit_scale", ga[2], gb[2])):
        assert bool(torch.isfinite(y).all()), name
        assert _rel(y, x) < 1e-6, name
    want = reference(q, k, torch.tensor(LOGIT_SCALE), gq, gk, None, grad=1.3)
    print(f"[multipos padding] loss {float(a[0]):.7f}, fp64 reference {float(want[0]):.7f}")
    assert abs(float(a[0]) - float(want[0])) < 1e-5 * abs(float(want[0]))
    assert _rel(a[2], want[5]) < 1e-5


@pytest.mark.parametrize("nq,nk,E,use_sel", SHAPES)
def test_one_positive_per_row_agrees_with_the_infonce_head(nq, nk, E, use_sel):
    """The same inputs through ``InfoNCEFn`` (labels) and ``MultiPosHeadFn`` (ids with one key each): loss 1e-5, dq / dk 2e-5
    rel-L2, dlogit_scale within 2e-5 sum |G x|."""
    from clip_event_amd.functional import InfoNCEFn, MultiPosHeadFn
    q, k, gq, gk, sel = _case(nq, nk, E, use_sel, "one")
    labels = torch.tensor([int(torch.nonzero(gk == g).flatten()[0]) for g in gq])
    seld = None if sel is None else sel.to(DEV)
    out = []
    for fn, args in ((InfoNCEFn, (labels.to(DEV), seld)), (MultiPosHeadFn, (gq.to(DEV), gk.to(DEV), seld))):
        qd, kd, lsd = (t.clone().to(DEV).requires_grad_(True) for t in (q, k, torch.tensor(LOGIT_SCALE)))
        loss = fn.apply(qd, kd, lsd, *args)
        (loss * 1.3).backward()
        torch.cuda.synchronize()
        out.append((loss.detach(), qd.grad, kd.grad, lsd.grad))
    mag = float(reference(q, k, torch.tensor(LOGIT_SCALE), gq, gk, sel, grad=1.3)[6])
    (l0, dq0, dk0, ds0), (l1, dq1, dk1, ds1) = out
    print(f"[multipos vs infonce {nq}x{nk}x{E}] loss {float(l1):.7f} vs {float(l0):.7f}, dq rel {_rel(dq1, dq0):.3e}, "
          f"dk rel {_rel(dk1, dk0):.3e}, dlogit_scale {float(ds1):.6e} vs {float(ds0):.6e} (sum|G x| {mag:.3e})")
    assert abs(float(l1) - float(l0)) < 1e-5 * abs(float(l0))
    assert _rel(dq1, dq0) < 2e-5 and _rel(dk1, dk0) < 2e-5
    assert abs(float(ds1) - float(ds0)) <= 2e-5 * mag


# ---- the sigmoid form ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bias", [-10.0, 0.0])
@pytest.mark.parametrize("nq,nk,E,use_sel", SHAPES)
def test_sigmoid_group_form_with_one_positive_agrees_with_the_label_form(nq, nk, E, use_sel, bias):
    """``SigmoidHeadFn`` with labels and with ids that give every row that one positive: the same pairs get the same sign, so the
    two agree at the head's bounds (loss 1e-5, dq / dk 2e-5 rel-L2, scale and bias gradients 2e-5)."""
    from clip_event_amd.functional import SigmoidHeadFn
    q, k, gq, gk, sel = _case(nq, nk, E, use_sel, "one")
    labels = torch.tensor([int(torch.nonzero(gk == g).flatten()[0]) for g in gq])
    seld = None if sel is None else sel.to(DEV)
    out = []
    for groups in (None, (gq.to(DEV), gk.to(DEV))):
        qd, kd, lsd, lbd = (t.clone().to(DEV).requires_grad_(True) for t in (q, k, torch.tensor(LOGIT_SCALE), torch.tensor(bias)))
        if groups is None:
            loss = SigmoidHeadFn.apply(qd, kd, lsd, lbd, labels.to(DEV), seld)
        else:
            loss = SigmoidHeadFn.apply(qd, kd, lsd, lbd, None, seld, None, None, groups)
        (loss * 1.3).backward()
        torch.cuda.synchronize()
        out.append((loss.detach(), qd.grad, kd.grad, lsd.grad, lbd.grad))
    for name, x, y, bound in zip(("loss", "dq", "dk", "dlogit_scale", "dlogit_bias"), out[1], out[0], (1e-5, 2e-5, 2e-5, 2e-5, 2e-5)):
        err = _rel(x, y)
        print(f"[sigmoid groups vs labels {nq}x{nk}x{E} bias {bias:g}] {name}: rel {err:.3e}")
        assert err < bound, (name, err)


def test_sigmoid_group_forward_repeats_bit_for_bit():
    """The 11-split shape, several positives per row: two forwards on the same inputs return the same bits."""
    from clip_event_amd.functional import SigmoidHeadFn
    q, k, gq, gk, sel = _case(70, 333, 128, True, "layout22")
    args = (q.to(DEV), k.to(DEV), torch.tensor(LOGIT_SCALE, device=DEV), torch.tensor(-10.0, device=DEV), None, sel.to(DEV), None, None,
            (gq.to(DEV), gk.to(DEV)))
    losses = [SigmoidHeadFn.apply(*args) for _ in range(2)]
    torch.cuda.synchronize()
    a, b = (t.cpu().view(torch.int32) for t in losses)
    assert torch.equal(a, b), (float(losses[0]), float(losses[1]))


@pytest.mark.parametrize("pattern", ["layout22", "scattered", "negative_and_unmatched", "highbits"])
@pytest.mark.parametrize("nq,nk,E,use_sel", [(70, 333, 128, True), (40, 96, 256, False)])
def test_sigmoid_group_form_against_fp64_reference(nq, nk, E, use_sel, pattern):
    """Several positives per row, bias -10: loss 1e-5, dq / dk 2e-5 rel-L2; the scale and bias gradients are sums of terms of
    both signs (positives pull, negatives push), so each is held to 2e-5 of the sum of its terms' magnitudes."""
    from clip_event_amd.functional import SigmoidHeadFn
    q, k, gq, gk, sel = _case(nq, nk, E, use_sel, pattern)
    ls, lb = torch.tensor(LOGIT_SCALE), torch.tensor(-10.0)
    want = sigmoid_reference(q, k, ls, lb, gq, gk, sel, grad=1.3)
    qd, kd, lsd, lbd = (t.clone().to(DEV).requires_grad_(True) for t in (q, k, ls, lb))
    loss = SigmoidHeadFn.apply(qd, kd, lsd, lbd, None, None if sel is None else sel.to(DEV), None, None, (gq.to(DEV), gk.to(DEV)))
    (loss * 1.3).backward()
    torch.cuda.synchronize()
    # magnitudes of the terms of the two scalar gradients, in fp64
    qs = (q if sel is None else q[sel]).double()
    x = ls.double().exp() * torch.nn.functional.normalize(qs, dim=1) @ torch.nn.functional.normalize(k.double(), dim=1).t()
    pos = positives(gq if sel is None else gq[sel], gk)
    z = torch.where(pos, 1.0, -1.0).double()
    G = -(1.3 / nq) * z * torch.sigmoid(-z * (x - 10.0))
    mag_b, mag_s = float(G.abs().sum()), float((G * x).abs().sum())
    tag = f"[sigmoid groups {nq}x{nk}x{E} {pattern}]"
    for name, g, w, bound in zip(("loss", "dq", "dk"), (loss.detach(), qd.grad, kd.grad), want, (1e-5, 2e-5, 2e-5)):
        err = _rel(g, w)
        print(f"{tag} {name}: kernel rel {err:.3e}")
        assert err < bound, (name, err)
    es, eb = abs(float(lsd.grad) - float(want[3])), abs(float(lbd.grad) - float(want[4]))
    print(f"{tag} dlogit_scale err / sum|terms| {es / mag_s:.3e}, dlogit_bias err / sum|terms| {eb / mag_b:.3e}")
    assert es <= 2e-5 * mag_s and eb <= 2e-5 * mag_b


# ---- materialised logits ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pattern", ["one", "layout22", "scattered", "negative_and_unmatched", "highbits"])
@pytest.mark.parametrize("rows,C,use_sel", [(5, 7, False), (42, 70, True), (13, 333, True)])
def test_multipos_xent_against_fp64_reference(rows, C, use_sel, pattern):
    """``losses.multipos_cross_entropy`` (``ce_multipos_xent_fwd/bwd``, one wave per row) on given logits: loss 1e-5, dlogits 2e-5
    rel-L2, rows outside ``sel`` and rows without a positive exactly zero."""
    from clip_event_amd.losses import multipos_cross_entropy
    rng = np.random.default_rng(rows * 13 + C + PATTERNS.index(pattern))
    x = torch.from_numpy((rng.standard_normal((rows, C)) * 6).astype(np.float32))
    sel = torch.from_numpy(np.sort(rng.permutation(rows)[:max(2, rows * 2 // 3)]).astype(np.int64)) if use_sel else None
    gq, gk = _groups(pattern, rng, rows, C, *((int(sel[0]), int(sel[1])) if use_sel else (0, 1)))
    x64 = x.double().requires_grad_(True)
    xs, gs = (x64, gq) if sel is None else (x64[sel], gq[sel])
    pos = positives(gs, gk)
    want = multipos_loss_from_logits(xs, pos)
    (want * 1.3).backward()
    xd = x.clone().to(DEV).requires_grad_(True)
    loss = multipos_cross_entropy(xd, gq.to(DEV), gk.to(DEV), None if sel is None else sel.to(DEV))
    (loss * 1.3).backward()
    torch.cuda.synchronize()
    el, eg = _rel(loss.detach(), want.detach()), _rel(xd.grad, x64.grad)
    print(f"[multipos xent {rows}x{C} {pattern}] loss rel {el:.3e}, dlogits rel {eg:.3e}, live rows {int((pos.sum(1) > 0).sum())}")
    assert int((pos.sum(1) > 0).sum()) >= 1
    zero_rows = (x64.grad.abs().sum(1) == 0)
    if bool(zero_rows.any()):
        assert float(xd.grad.cpu()[zero_rows].abs().max()) == 0.0
    assert el < 1e-5 and eg < 2e-5


# ---- arguments -------------------------------------------------------------------------------------------------------------------

def test_arguments_are_checked_before_any_launch():
    """A refusal names its reason and writes nothing: the outputs keep their NaN fill."""
    from clip_event_amd._lib import lib
    cl = lib()
    one = torch.zeros(256, device=DEV)
    out = torch.full((64,), float("nan"), device=DEV)
    idx = torch.zeros(4, dtype=torch.int64, device=DEV)
    p, o, i = (ctypes.c_void_p(t.data_ptr()) for t in (one, out, idx))
    rc = cl.ce_multipos_head_fwd(p, 96, None, 2, p, 96, 2, 96, p, i, i, o, o, o, p, None)
    assert rc != 0 and b"multiple of 128" in cl.ce_last_error()
    rc = cl.ce_multipos_head_fwd(p, 128, None, 2, p, 128, 2, 128, p, i, None, o, o, o, p, None)
    assert rc != 0 and b"null" in cl.ce_last_error()
    rc = cl.ce_multipos_head_fwd(p, 128, None, 2, p, 128, 2, 128, p, i, i, o, None, o, p, None)
    assert rc != 0 and b"null" in cl.ce_last_error()
    rc = cl.ce_multipos_head_fwd(p, 128, None, 0, p, 128, 2, 128, p, i, i, o, o, o, p, None)
    assert rc != 0 and b"empty" in cl.ce_last_error()
    rc = cl.ce_multipos_head_bwd(p, 128, None, 2, p, 130, 2, 128, p, i, i, p, p, p, o, o, o, None)
    assert rc != 0 and b"leading dimensions" in cl.ce_last_error()
    rc = cl.ce_multipos_head_bwd(p, 128, None, 2, p, 128, 2, 128, p, i, i, p, None, p, o, o, o, None)
    assert rc != 0 and b"null" in cl.ce_last_error()
    rc = cl.ce_sigmoid_head_group_fwd(p, 96, None, 2, p, 96, 2, 96, p, p, i, i, o, p, None)
    assert rc != 0 and b"multiple of 128" in cl.ce_last_error()
    rc = cl.ce_sigmoid_head_group_fwd(p, 128, None, 2, p, 128, 2, 128, p, None, i, i, o, p, None)
    assert rc != 0 and b"null" in cl.ce_last_error()
    rc = cl.ce_sigmoid_head_group_bwd(p, 128, None, 2, p, 128, 2, 128, p, p, i, None, p, o, o, o, o, None)
    assert rc != 0 and b"null" in cl.ce_last_error()
    rc = cl.ce_multipos_xent_fwd(p, 2, i, None, None, o, o, o, 2, 4, None)
    assert rc != 0 and b"null" in cl.ce_last_error()
    rc = cl.ce_multipos_xent_fwd(p, 2, i, i, None, o, o, o, 2, 4, None)
    assert rc != 0 and b"bad shape" in cl.ce_last_error()
    rc = cl.ce_multipos_xent_bwd(p, 4, i, i, None, p, p, p, o, 2, 2, 4, None)
    assert rc != 0 and b"bad shape" in cl.ce_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
