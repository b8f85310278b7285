"""CPU (no GPU): the distillation loss's reference against open_clip's expression, the three identities the sweep
decomposition rests on in fp64, the size of the op test's cases, the C ABI's declarations, and ``Distillation``'s
argument checks."""
import pytest
import torch
import torch.nn.functional as F

from oracle import clip_oracle as O
from tests import distill_ref as R

CFG = O.ClipConfig(64, 64, 2, 128, 32, 20, 512, 128, 2, 3)


def _clip(seed=3):
    from clip_event_amd.model import build_model
    return build_model({k: v.clone() for k, v in O.init_params(CFG, seed).items()})


def _open_clip_dist_loss(teacher_logits, student_logits):
    """``DistillClipLoss.dist_loss`` of open_clip (src/open_clip/loss.py), verbatim in form."""
    return -(teacher_logits.softmax(dim=1) * student_logits.log_softmax(dim=1)).sum(dim=1).mean(dim=0)


@pytest.mark.parametrize("nq,nk", [(5, 7), (16, 48)])
def test_reference_is_open_clips_dist_loss(nq, nk):
    g = torch.Generator().manual_seed(nq * 100 + nk)
    S = torch.randn(nq, nk, generator=g, dtype=torch.float64) * 8
    T = torch.randn(nq, nk, generator=g, dtype=torch.float64) * 8
    a, b = R.distill_loss_from_logits(S, T), _open_clip_dist_loss(T, S)
    assert abs(float(a - b)) <= 1e-12 * abs(float(b))
    # and as soft-target cross entropy
    c = F.cross_entropy(S, T.softmax(dim=1))
    assert abs(float(a - c)) <= 1e-12 * abs(float(c))


@pytest.mark.parametrize("shape,A,pair", R.CASES)
def test_sweep_identities_hold_in_fp64_and_the_cases_are_not_degenerate(shape, A, pair):
    """With v_r = sum_c P_t[r,c] k^_c:  sum_c P_t S = s <q^_r, v_r>;  dq^_r = (g/nq) s (sum_c P_s k^_c - v_r);
    dlogit_scale = sum_r <q^_r, dq^_r> -- each to 1e-12 against autograd on the normalised features, on every case of the op
    test.  Every case has a loss and a |dlogit_scale| of at least 0.1 (a relative bound means something)."""
    (q, k, tq, tk, sel, ls, tls), want = R.case_and_reference(shape, A, pair)
    g = 1.3
    dt = torch.float64
    qs, tqs = (q if sel is None else q[sel]).to(dt), (tq if sel is None else tq[sel]).to(dt)
    qn = R._unit(qs).requires_grad_(True)
    kn = R._unit(k.to(dt)).requires_grad_(True)
    lsd = ls.to(dt).requires_grad_(True)
    s = lsd.exp()
    S = s * qn @ kn.t()
    T = tls.to(dt).exp() * R._unit(tqs) @ R._unit(tk.to(dt)).t()
    loss = R.distill_loss_from_logits(S, T)
    (loss * g).backward()
    nq = qn.shape[0]
    Pt, Ps = T.softmax(dim=1), S.detach().softmax(dim=1)
    v = Pt @ kn.detach()
    sd = s.detach()
    lse = S.detach().logsumexp(dim=1)
    loss_id = (lse - sd * (qn.detach() * v).sum(dim=1)).mean()
    dq_id = (g / nq) * sd * (Ps @ kn.detach() - v)
    dls_id = (qn.detach() * dq_id).sum()
    dk_id = (g / nq) * sd * ((Ps - Pt).t() @ qn.detach())
    assert abs(float(loss_id - loss)) <= 1e-12 * abs(float(loss))
    assert float((dq_id - qn.grad).norm()) <= 1e-12 * float(qn.grad.norm())
    assert float((dk_id - kn.grad).norm()) <= 1e-12 * float(kn.grad.norm())
    assert abs(float(dls_id - lsd.grad)) <= 1e-12 * abs(float(lsd.grad))
    assert abs(float((kn.detach() * dk_id).sum() - lsd.grad)) <= 1e-11 * abs(float(lsd.grad))     # and over the keys
    print(f"[distill {shape} A {A} scales {R.SCALE_PAIRS[pair]}] loss {float(want[0]):.4f}, dlogit_scale {float(want[3]):.4f}")
    assert abs(float(want[0] - loss)) <= 1e-12 * abs(float(loss))
    assert float(want[0]) >= 0.1 and abs(float(want[3])) >= 0.1


def test_header_declares_the_entry_points_and_the_binding_takes_them():
    from clip_event_amd import _lib
    with open(_lib.HEADER) as f:
        sig = _lib.signatures(f.read())
    for name, nargs in (("ce_distill_head_workspace_bytes", 1), ("ce_distill_head_fwd", 21), ("ce_distill_head_bwd", 22),
                        ("ce_rowdot_sum", 8), ("ce_soft_xent_fwd", 11), ("ce_soft_xent_bwd", 13)):
        assert name in sig and len(sig[name][1]) == nargs, name
    import ctypes
    assert sig["ce_distill_head_workspace_bytes"][0] is ctypes.c_size_t
    cl = _lib.lib()
    for name in ("ce_distill_head_fwd", "ce_distill_head_bwd", "ce_rowdot_sum", "ce_soft_xent_fwd", "ce_soft_xent_bwd"):
        assert getattr(cl, name).argtypes == sig[name][1], name
    assert cl.ce_distill_head_workspace_bytes(40) >= 40 * 4


def test_distillation_checks_its_arguments():
    from clip_event_amd.engine import Distillation
    from clip_event_amd.losses import CriterionDistill
    teacher = _clip()
    d = Distillation(teacher, weight=0.5)
    assert not teacher.training and not any(p.requires_grad for p in teacher.parameters()) and d.weight == 0.5
    assert float(d.logit_scale("cpu")) == float(teacher.logit_scale.detach())
    with pytest.raises(ValueError, match="optimiser"):
        d.check_optimizer(torch.optim.SGD(list(teacher.parameters()), lr=0.1))
    d.check_optimizer(torch.optim.SGD(list(_clip(4).parameters()), lr=0.1))            # another model's parameters: fine
    with pytest.raises(ValueError, match="logit_scale"):
        Distillation(None)
    assert float(Distillation(None, logit_scale=2.5).logit_scale("cpu")) == 2.5
    with pytest.raises(ValueError, match="weight"):
        Distillation(teacher, weight=-0.1)
    with pytest.raises(ValueError, match="weight"):
        CriterionDistill(weight=-1.0)
    with pytest.raises(TypeError, match="CLIP"):
        Distillation(torch.nn.Linear(2, 2))
    dropped = _clip()
    dropped.set_patch_dropout(0.5)
    with pytest.raises(ValueError, match="patch dropout"):
        Distillation(dropped)
    with pytest.raises(ValueError, match="teacher_features"):
        Distillation(None, logit_scale=2.5).encode(torch.zeros(1, 3, 64, 64), torch.zeros(1, 20, dtype=torch.long))
    with pytest.raises(ValueError, match="teacher_image"):
        d.encode(torch.zeros(1, 3, 32, 32), torch.zeros(1, 20, dtype=torch.long))
