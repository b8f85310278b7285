"""fp64 reference of the sigmoid pairwise loss (SigLIP) with a logit bias, written from the formula, independently of
``losses.CriterionSigmoid`` and of the kernels:

    x[r,c] = exp(logit_scale) <q^_r, k^_c> + logit_bias,   z[r,c] = +1 if c == labels[src(r)] else -1
    loss   = -(1/nq) sum_r sum_c log sigma(z x)

``q`` / ``k`` are RAW features (normalised here), query r is row ``sel[r]`` of ``q`` (``sel`` None: row r)."""
import torch
import torch.nn.functional as F


def sigmoid_loss_from_logits(x: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
    """``x`` [nq, nk] already holds scale * similarity + bias; ``labels`` [nq] the positive column of every row."""
    z = -torch.ones_like(x)
    z[torch.arange(x.shape[0]), labels] = 1.0
    return -F.logsigmoid(z * x).sum() / x.shape[0]


def sigmoid_loss(q, k, logit_scale, logit_bias, labels, sel=None, dtype=torch.float64):
    """Loss as a ``dtype`` scalar; the inputs may carry ``requires_grad`` (autograd gives the reference gradients)."""
    q, k = q.to(dtype), k.to(dtype)
    qs = q if sel is None else q[sel]
    ys = labels if sel is None else labels[sel]
    qn = qs / qs.norm(dim=1, keepdim=True)
    kn = k / k.norm(dim=1, keepdim=True)
    x = logit_scale.to(dtype).exp() * qn @ kn.t() + logit_bias.to(dtype)
    return sigmoid_loss_from_logits(x, ys)


def reference(q, k, logit_scale, logit_bias, labels, sel=None, grad=1.0, dtype=torch.float64):
    """(loss, dq, dk, dlogit_scale, dlogit_bias) in ``dtype`` on the CPU for the upstream gradient ``grad``."""
    leaves = [t.detach().cpu().to(dtype).requires_grad_(True) for t in (q, k, logit_scale, logit_bias)]
    labels = labels.cpu()
    sel = None if sel is None else sel.cpu()
    loss = sigmoid_loss(*leaves, labels, sel, dtype=dtype)
    (loss * grad).backward()
    return (loss.detach(),) + tuple(t.grad for t in leaves)
