"""fp64 reference of the distillation loss (open_clip's ``DistillClipLoss.dist_loss``), written from the formula with
``log_softmax`` and autograd, independently of ``losses.CriterionDistill`` and of the kernels:

    S[r,c] = exp(logit_scale) <q^_r, k^_c>          student
    T[r,c] = exp(teacher_logit_scale) <tq^_r, tk^_c>  teacher: a constant
    loss   = -(softmax_c(T) * log_softmax_c(S)).sum(1).mean()

``q`` / ``k`` / ``tq`` / ``tk`` are RAW features (normalised here), query r is row ``sel[r]`` of ``q`` and of ``tq`` (``sel`` None:
row r).  Also the inputs of tests/test_distill_ops.py, shared with the CPU test that checks their size."""
import numpy as np
import torch

LN = np.log
SCALE_PAIRS = [(float(LN(100.0)), float(LN(100.0))), (float(LN(14.0)), float(LN(100.0))), (float(LN(100.0)), float(LN(10.0)))]
# (nq, nk, Es, Et, rows of q when the queries go through sel or None)
SHAPES = [(33, 33, 128, 256, None),      # padded tile; 8-wave similarity with 128-wide values
          (40, 97, 256, 128, None),      # splits > 1: the atomic path; 4-wave similarity, 256-wide values
          (20, 70, 128, 128, 70),        # the text direction: 20 of 70 rows through sel
          (64, 320, 512, 768, None),     # the real pair's widths
          (40, 97, 1024, 128, None)]     # all GT accumulators


def pulls(Es, Et):
    """A = 0.3 only where both widths are at most 256: wider, with both scales at 100, both distributions collapse to one-hot."""
    return (0.0, 0.3) if max(Es, Et) <= 256 else (0.0,)


CASES = [(shape, A, pair) for shape in SHAPES for A in pulls(shape[2], shape[3]) for pair in range(len(SCALE_PAIRS))]


def distill_loss_from_logits(S: torch.Tensor, T: torch.Tensor) -> torch.Tensor:
    return -(T.softmax(dim=1) * S.log_softmax(dim=1)).sum(dim=1).mean()


def _unit(x):
    return x / x.norm(dim=1, keepdim=True)


def make_case(nq, nk, Es, Et, rows_q=None, A=0.0, seed_extra=0):
    """(q, k, tq, tk, sel): independent unit-norm random rows; the first nq keys are pulled towards their queries, student and
    teacher alike (k_r += A q_r, tk_r += A tq_r)."""
    rng = np.random.default_rng(1000 * nq + 10 * nk + Es + 3 * Et + seed_extra)
    rq = nq if rows_q is None else rows_q

    def rows(n, E):
        return _unit(torch.from_numpy(rng.standard_normal((n, E))).double())

    q, k, tq, tk = rows(rq, Es), rows(nk, Es), rows(rq, Et), rows(nk, Et)
    sel = None if rows_q is None else torch.from_numpy(rng.permutation(rq)[:nq].astype(np.int64))
    src = torch.arange(nq) if sel is None else sel
    m = min(nq, nk)
    k[:m] += A * q[src[:m]]
    tk[:m] += A * tq[src[:m]]
    return q.float(), k.float(), tq.float(), tk.float(), sel


def logits(q, k, logit_scale, sel=None, dtype=torch.float64):
    q, k = q.to(dtype), k.to(dtype)
    qs = q if sel is None else q[sel]
    return logit_scale.to(dtype).exp() * _unit(qs) @ _unit(k).t()


def distill_loss(q, k, logit_scale, tq, tk, teacher_logit_scale, sel=None, dtype=torch.float64):
    """Loss as a ``dtype`` scalar; q, k, logit_scale may carry ``requires_grad`` (autograd gives the reference gradients)."""
    T = logits(tq.detach(), tk.detach(), teacher_logit_scale.detach(), sel, dtype)
    return distill_loss_from_logits(logits(q, k, logit_scale, sel, dtype), T)


def reference(q, k, logit_scale, tq, tk, teacher_logit_scale, sel=None, grad=1.0, dtype=torch.float64):
    """(loss, dq, dk, dlogit_scale) in ``dtype`` on the CPU for the upstream gradient ``grad``."""
    leaves = [t.detach().cpu().to(dtype).requires_grad_(True) for t in (q, k, logit_scale)]
    sel = None if sel is None else sel.cpu()
    loss = distill_loss(*leaves, tq.detach().cpu(), tk.detach().cpu(), teacher_logit_scale.detach().cpu(), sel, dtype=dtype)
    (loss * grad).backward()
    return (loss.detach(),) + tuple(t.grad for t in leaves)


_CACHE = {}


def case_and_reference(shape, A, pair):
    """The inputs of a case and its fp64 reference at upstream gradient 1.3, computed once and shared (read-only)."""
    key = (shape, A, pair)
    if key not in _CACHE:
        nq, nk, Es, Et, rows_q = shape
        q, k, tq, tk, sel = make_case(nq, nk, Es, Et, rows_q, A)
        ls, tls = (torch.tensor(v) for v in SCALE_PAIRS[pair])
        _CACHE[key] = ((q, k, tq, tk, sel, ls, tls), reference(q, k, ls, tq, tk, tls, sel, grad=1.3))
    return _CACHE[key]
