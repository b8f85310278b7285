"""fp64 reference of the multi-positive (group-id) losses, written from the formulas, with no import of the product:

    x[r,c] = exp(logit_scale) <q^_r, k^_c>
    P(r)   = { c : gq[src(r)] >= 0 and gk[c] == gq[src(r)] },   n_r = |P(r)|
    loss   = (1/nq) sum_{r : n_r > 0} ( lse_r - (1/n_r) sum_{c in P(r)} x[r,c] )

and the sigmoid form, z[r,c] = +1 iff c in P(r), loss = -(1/nq) sum_r sum_c log sigma(z (x + logit_bias)).

``q`` / ``k`` are RAW features (normalised here), query r is row ``sel[r]`` of ``q`` (``sel`` None: row r), ``gq`` has one id
per row of ``q`` (read through ``sel``), ``gk`` one per row of ``k``.  A negative id belongs to no group."""
import torch
import torch.nn.functional as F


def positives(gq_rows: torch.Tensor, gk: torch.Tensor) -> torch.Tensor:
    """[nq, nk] bool: key c is a positive of query r.  ``gq_rows`` are the ids of the query rows themselves."""
    gq_rows, gk = gq_rows.to(torch.int64).reshape(-1, 1), gk.to(torch.int64).reshape(1, -1)
    return (gq_rows == gk) & (gq_rows >= 0)


def multipos_loss_from_logits(x: torch.Tensor, pos: torch.Tensor) -> torch.Tensor:
    """``x`` [nq, nk] scaled similarities, ``pos`` [nq, nk] bool.  Rows without a positive add nothing; the divisor stays nq."""
    n = pos.sum(dim=1)
    live = n > 0
    lse = torch.logsumexp(x, dim=1)
    mean_pos = (x * pos.to(x.dtype)).sum(dim=1) / n.clamp(min=1).to(x.dtype)
    return ((lse - mean_pos) * live.to(x.dtype)).sum() / x.shape[0]


def sigmoid_loss_from_logits(x: torch.Tensor, pos: torch.Tensor) -> torch.Tensor:
    """``x`` [nq, nk] already holds scale * similarity + bias."""
    z = torch.where(pos, torch.ones_like(x), -torch.ones_like(x))
    return -F.logsigmoid(z * x).sum() / x.shape[0]


def _logits(q, k, logit_scale, gq, sel, dtype):
    q, k = q.to(dtype), k.to(dtype)
    qs = q if sel is None else q[sel]
    gs = gq if sel is None else gq[sel]
    qn = qs / qs.norm(dim=1, keepdim=True)
    kn = k / k.norm(dim=1, keepdim=True)
    return logit_scale.to(dtype).exp() * qn @ kn.t(), gs


def multipos_loss(q, k, logit_scale, gq, gk, sel=None, dtype=torch.float64):
    x, gs = _logits(q, k, logit_scale, gq, sel, dtype)
    return multipos_loss_from_logits(x, positives(gs, gk))


def sigmoid_group_loss(q, k, logit_scale, logit_bias, gq, gk, sel=None, dtype=torch.float64):
    x, gs = _logits(q, k, logit_scale, gq, sel, dtype)
    return sigmoid_loss_from_logits(x + logit_bias.to(dtype), positives(gs, gk))


def reference(q, k, logit_scale, gq, gk, sel=None, grad=1.0, dtype=torch.float64):
    """(loss, dq, dk, dlogit_scale, lse [nq], invpos [nq], sum |G x|) in ``dtype`` on the CPU for the upstream gradient ``grad``.
    sum |G x| is the magnitude of the terms whose (cancelling) sum is dlogit_scale."""
    leaves = [t.detach().cpu().to(dtype).requires_grad_(True) for t in (q, k, logit_scale)]
    gq, gk = gq.cpu(), gk.cpu()
    sel = None if sel is None else sel.cpu()
    loss = multipos_loss(*leaves, gq, gk, sel, dtype=dtype)
    (loss * grad).backward()
    with torch.no_grad():
        x, gs = _logits(*leaves, gq, sel, dtype)
        pos = positives(gs, gk)
        n = pos.sum(dim=1)
        lse = torch.logsumexp(x, dim=1)
        invpos = torch.where(n > 0, 1.0 / n.clamp(min=1).to(dtype), torch.zeros((), dtype=dtype))
        G = grad / x.shape[0] * (torch.exp(x - lse[:, None]) - pos.to(dtype) * invpos[:, None]) * (n > 0).to(dtype)[:, None]
        mag = (G * x).abs().sum()
    return (loss.detach(),) + tuple(t.grad for t in leaves) + (lse, invpos, mag)


def sigmoid_reference(q, k, logit_scale, logit_bias, gq, gk, sel=None, grad=1.0, dtype=torch.float64):
    """(loss, dq, dk, dlogit_scale, dlogit_bias) in ``dtype`` on the CPU."""
    leaves = [t.detach().cpu().to(dtype).requires_grad_(True) for t in (q, k, logit_scale, logit_bias)]
    sel = None if sel is None else sel.cpu()
    loss = sigmoid_group_loss(*leaves, gq.cpu(), gk.cpu(), sel, dtype=dtype)
    (loss * grad).backward()
    return (loss.detach(),) + tuple(t.grad for t in leaves)
