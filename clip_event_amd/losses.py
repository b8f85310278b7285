"""Drop-ins for ``CriterionContrastive`` / ``CriterionAlignment`` (reference model_clip.py:620-715)
on the HIP kernels of head.hip / ot.hip."""
from __future__ import annotations

import torch
from torch import nn

from ._lib import check, lib, ptr, stream


class _CrossEntropyFn(torch.autograd.Function):
    """nn.CrossEntropyLoss() (mean) over the rows selected by ``sel`` (index_pos) or all rows."""

    @staticmethod
    def forward(ctx, logits, labels, sel):
        if not logits.is_cuda:
            raise RuntimeError("clip_event_amd losses run on the GPU only (no CPU fallback)")
        logits = logits if (logits.dtype == torch.float32 and logits.is_contiguous()) else logits.contiguous().float()
        labels = labels.to(device=logits.device, dtype=torch.int64).contiguous()
        if sel is not None:
            sel = sel.to(device=logits.device, dtype=torch.int64).contiguous()
        nrows = logits.shape[0] if sel is None else sel.shape[0]
        C = logits.shape[1]
        lse = torch.empty(nrows, dtype=torch.float32, device=logits.device)
        loss = torch.zeros((), dtype=torch.float32, device=logits.device)
        check(lib().ce_xent_fwd(ptr(logits), logits.stride(0), ptr(labels), ptr(sel), ptr(lse), ptr(loss),
                                nrows, C, stream()), "ce_xent_fwd")
        ctx.saved = (logits, labels, sel, lse)
        return loss

    @staticmethod
    def backward(ctx, g):
        logits, labels, sel, lse = ctx.saved
        nrows = logits.shape[0] if sel is None else sel.shape[0]
        d = torch.zeros_like(logits) if sel is not None else torch.empty_like(logits)
        g = g.contiguous().float()
        check(lib().ce_xent_bwd(ptr(logits), logits.stride(0), ptr(labels), ptr(sel), ptr(lse), ptr(g), ptr(d),
                                d.stride(0), nrows, logits.shape[1], stream()), "ce_xent_bwd")
        return d, None, None


def cross_entropy(logits, labels, sel=None):
    return _CrossEntropyFn.apply(logits, labels, sel)


class _MultiPosCrossEntropyFn(torch.autograd.Function):
    """mean over the rows ``sel`` (or all rows) of lse(x_r) - mean_{c in P(r)} x_r,c, P(r) the columns whose group id equals the
    row's (and is not negative); a row without positives adds nothing and the divisor stays the row count."""

    @staticmethod
    def forward(ctx, logits, row_groups, col_groups, sel):
        if not logits.is_cuda:
            raise RuntimeError("clip_event_amd losses run on the GPU only (no CPU fallback)")
        logits = logits if (logits.dtype == torch.float32 and logits.is_contiguous()) else logits.contiguous().float()
        dev = logits.device
        row_groups = row_groups.to(device=dev, dtype=torch.int64).contiguous()
        col_groups = col_groups.to(device=dev, dtype=torch.int64).contiguous()
        if row_groups.shape[0] != logits.shape[0] or col_groups.shape[0] != logits.shape[1]:
            raise RuntimeError(f"{row_groups.shape[0]} row / {col_groups.shape[0]} column group ids for logits {tuple(logits.shape)}")
        if sel is not None:
            sel = sel.to(device=dev, dtype=torch.int64).contiguous()
        nrows = logits.shape[0] if sel is None else sel.shape[0]
        stats = torch.empty(2, nrows, dtype=torch.float32, device=dev)                     # lse | 1 / positives
        loss = torch.zeros((), dtype=torch.float32, device=dev)
        check(lib().ce_multipos_xent_fwd(ptr(logits), logits.stride(0), ptr(row_groups), ptr(col_groups), ptr(sel), ptr(stats[0]),
                                         ptr(stats[1]), ptr(loss), nrows, logits.shape[1], stream()), "ce_multipos_xent_fwd")
        ctx.saved = (logits, row_groups, col_groups, sel, stats)
        return loss

    @staticmethod
    def backward(ctx, g):
        logits, row_groups, col_groups, sel, stats = ctx.saved
        nrows = logits.shape[0] if sel is None else sel.shape[0]
        d = torch.zeros_like(logits) if sel is not None else torch.empty_like(logits)
        g = g.contiguous().float()
        check(lib().ce_multipos_xent_bwd(ptr(logits), logits.stride(0), ptr(row_groups), ptr(col_groups), ptr(sel), ptr(stats[0]),
                                         ptr(stats[1]), ptr(g), ptr(d), d.stride(0), nrows, logits.shape[1], stream()),
              "ce_multipos_xent_bwd")
        return d, None, None, None


def multipos_cross_entropy(logits, row_groups, col_groups, sel=None):
    return _MultiPosCrossEntropyFn.apply(logits, row_groups, col_groups, sel)


class _ElemLossFn(torch.autograd.Function):
    """nn.BCEWithLogitsLoss() (mode 0) / nn.KLDivLoss() (mode 1), default 'mean' reduction."""

    @staticmethod
    def forward(ctx, x, y, mode):
        x = x.contiguous().float()
        y = y.to(x.device).contiguous().float()
        if x.shape != y.shape:
            raise RuntimeError(f"target size {tuple(y.shape)} must match input size {tuple(x.shape)}")
        loss = torch.zeros((), dtype=torch.float32, device=x.device)
        check(lib().ce_elem_loss_fwd(ptr(x), ptr(y), x.numel(), mode, ptr(loss), stream()), "ce_elem_loss_fwd")
        ctx.saved, ctx.mode = (x, y), mode
        return loss

    @staticmethod
    def backward(ctx, g):
        x, y = ctx.saved
        dx = torch.empty_like(x)
        g = g.contiguous().float()
        check(lib().ce_elem_loss_bwd(ptr(x), ptr(y), x.numel(), ctx.mode, ptr(g), ptr(dx), stream()),
              "ce_elem_loss_bwd")
        return dx, None, None


class CriterionContrastive(nn.Module):
    """model_clip.py:620-662.  ``forward`` keeps the reference signature; ``index_pos`` is
    effectively required there (``index_select(index=None)`` fails) and is required here too."""

    def __init__(self, constrastive_loss):
        super().__init__()
        if constrastive_loss not in ("ce", "bce", "kl"):
            raise RuntimeError("Invalid constrastive_loss '{}'. ".format(constrastive_loss))
        self.kind = constrastive_loss

    def forward(self, logits_per_image, logits_per_text, labels_per_image=None, labels_per_text=None,
                index_pos=None, constrastive_overbatch=True):
        n = logits_per_image.shape[0]
        dev = logits_per_image.device
        if labels_per_image is None:
            labels_per_image = torch.arange(n, device=dev)
        if labels_per_text is None:
            labels_per_text = torch.arange(n, device=dev)
        if index_pos is None:
            raise TypeError("index_select(): argument 'index' must be Tensor, not NoneType")
        if self.kind == "ce":
            loss_i = cross_entropy(logits_per_image, labels_per_image)
        elif self.kind == "bce":
            loss_i = _ElemLossFn.apply(logits_per_image, labels_per_image, 0)
        else:
            loss_i = _ElemLossFn.apply(logits_per_image, labels_per_image, 1)
        loss_t = cross_entropy(logits_per_text, labels_per_text, index_pos)
        return {"loss_i": loss_i, "loss_t": loss_t}


class CriterionMultiPositive(nn.Module):
    """Several positive texts per image (and several images per text): each row's target is uniform over the SET of columns
    that carry the row's group id -- UniCL's bidirectional supervised contrastive loss; with one positive per row it is
    ``CriterionContrastive('ce')``.  ``labels_per_image`` [B] holds the images' group ids, ``labels_per_text`` [N] the texts'; a
    negative id belongs to no group (a text that is nobody's positive).  ``index_pos`` selects the text-direction query rows.
    When the logits' columns were gathered across ranks, ``all_groups=(groups_per_image_all, groups_per_text_all)`` gives the
    ids of the columns; without it the rows' ids are the columns' ids.  This is the logits path (``ce_multipos_xent_*``);
    ``engine`` runs the fused head (``functional.MultiPosHeadFn``) where the kernels take the width."""

    kind = "multipos"

    def forward(self, logits_per_image, logits_per_text, labels_per_image=None, labels_per_text=None,
                index_pos=None, constrastive_overbatch=True, all_groups=None):
        if not constrastive_overbatch:
            raise RuntimeError("CriterionMultiPositive needs constrastive_overbatch=True: the per-instance layout scores an image "
                               "against its own descriptions only, so it has no negatives from other images")
        if labels_per_image is None or labels_per_text is None:
            raise RuntimeError("CriterionMultiPositive needs the group ids of the images (labels_per_image) and of the texts "
                               "(labels_per_text): distributed.global_groups lays them out")
        gi_all, gt_all = (labels_per_image, labels_per_text) if all_groups is None else all_groups
        return {"loss_i": multipos_cross_entropy(logits_per_image, labels_per_image, gt_all),
                "loss_t": multipos_cross_entropy(logits_per_text, labels_per_text, gi_all, index_pos)}


class CriterionSigmoid(nn.Module):
    """The sigmoid pairwise loss of SigLIP (open_clip's ``SigLipLoss``) on a materialised ``logits_per_image`` [nq, nk]: every
    (image, text) pair is its own binary term, positive where the column is the image's label,
    loss = -(1/nq) sum_r sum_c log sigma(z (logits + logit_bias)).  One direction: ``logits_per_text`` and its labels are
    accepted for the common call and not used.  This is the general path, for embed dims the fused head
    (``functional.SigmoidHeadFn``) does not take; ``engine`` picks between them.

    ``multi_positive=True`` reads ``labels_per_image`` / ``labels_per_text`` as the group ids of the images and of the texts (as
    ``CriterionMultiPositive`` does): a pair is positive wherever the ids are equal and not negative.  ``all_groups`` as there."""

    kind = "sigmoid"

    def __init__(self, multi_positive: bool = False):
        super().__init__()
        self.multi_positive = bool(multi_positive)

    def forward(self, logits_per_image, logits_per_text, labels_per_image=None, labels_per_text=None,
                index_pos=None, constrastive_overbatch=True, logit_bias=None, all_groups=None):
        if not constrastive_overbatch:
            raise RuntimeError("CriterionSigmoid needs constrastive_overbatch=True: the per-instance layout scores an image against "
                               "its own descriptions only, so it has no negatives from other images")
        if logit_bias is None:
            raise RuntimeError("CriterionSigmoid needs logit_bias (model.enable_logit_bias())")
        nq, nk = logits_per_image.shape
        dev = logits_per_image.device
        if self.multi_positive:
            if labels_per_image is None or labels_per_text is None:
                raise RuntimeError("CriterionSigmoid(multi_positive=True) needs the group ids of the images and of the texts")
            gq = labels_per_image.to(device=dev, dtype=torch.int64).reshape(nq, 1)
            gk = (labels_per_text if all_groups is None else all_groups[1]).to(device=dev, dtype=torch.int64).reshape(1, nk)
            multihot = ((gq == gk) & (gq >= 0)).float()
            return {"loss_sig": _ElemLossFn.apply(logits_per_image + logit_bias, multihot, 0) * nk}
        if labels_per_image is None:
            labels_per_image = torch.arange(nq, device=dev)
        onehot = torch.zeros(nq, nk, dtype=torch.float32, device=dev)
        onehot.scatter_(1, labels_per_image.to(device=dev, dtype=torch.int64).reshape(nq, 1), 1.0)
        # BCE-with-logits is the mean over nq * nk elements; times nk it is the sum over pairs divided by nq
        return {"loss_sig": _ElemLossFn.apply(logits_per_image + logit_bias, onehot, 0) * nk}


class _SoftCrossEntropyFn(torch.autograd.Function):
    """mean over the rows ``sel`` (or all rows) of lse(x_r) - sum_c softmax(t_r)_c x_r,c; ``teacher_logits`` is a constant."""

    @staticmethod
    def forward(ctx, logits, teacher_logits, sel):
        if not logits.is_cuda:
            raise RuntimeError("clip_event_amd losses run on the GPU only (no CPU fallback)")
        if teacher_logits.shape != logits.shape:
            raise RuntimeError(f"teacher logits {tuple(teacher_logits.shape)} must match the student's {tuple(logits.shape)}")
        logits = logits if (logits.dtype == torch.float32 and logits.is_contiguous()) else logits.contiguous().float()
        teacher = teacher_logits.detach().to(logits.device).contiguous().float()
        if sel is not None:
            sel = sel.to(device=logits.device, dtype=torch.int64).contiguous()
        nrows = logits.shape[0] if sel is None else sel.shape[0]
        lse = torch.empty(2, nrows, dtype=torch.float32, device=logits.device)
        loss = torch.zeros((), dtype=torch.float32, device=logits.device)
        check(lib().ce_soft_xent_fwd(ptr(logits), logits.stride(0), ptr(teacher), teacher.stride(0), ptr(sel), ptr(lse[0]),
                                     ptr(lse[1]), ptr(loss), nrows, logits.shape[1], stream()), "ce_soft_xent_fwd")
        ctx.saved = (logits, teacher, sel, lse)
        return loss

    @staticmethod
    def backward(ctx, g):
        logits, teacher, sel, lse = ctx.saved
        nrows = logits.shape[0] if sel is None else sel.shape[0]
        d = torch.zeros_like(logits) if sel is not None else torch.empty_like(logits)
        g = g.contiguous().float()
        check(lib().ce_soft_xent_bwd(ptr(logits), logits.stride(0), ptr(teacher), teacher.stride(0), ptr(sel), ptr(lse[0]),
                                     ptr(lse[1]), ptr(g), ptr(d), d.stride(0), nrows, logits.shape[1], stream()), "ce_soft_xent_bwd")
        return d, None, None


def soft_cross_entropy(logits, teacher_logits, sel=None):
    return _SoftCrossEntropyFn.apply(logits, teacher_logits, sel)


class CriterionDistill(nn.Module):
    """The distillation terms of open_clip's ``DistillClipLoss`` on materialised logits: for each direction
    -(softmax(teacher logits) * log_softmax(logits)).sum(1).mean(), the text direction over the ``index_pos`` rows, times
    ``weight``.  The teacher's matrices are constants.  This is the general path, for embed dims the fused head
    (``functional.DistillHeadFn``) does not take, and its cross-check on the device; ``engine`` picks between them."""

    kind = "distill"

    def __init__(self, weight: float = 1.0):
        super().__init__()
        if not weight >= 0:
            raise ValueError(f"distillation weight must be >= 0 (got {weight})")
        self.weight = float(weight)

    def forward(self, logits_per_image, logits_per_text, teacher_logits_per_image, teacher_logits_per_text, index_pos=None):
        li = soft_cross_entropy(logits_per_image, teacher_logits_per_image)
        lt = soft_cross_entropy(logits_per_text, teacher_logits_per_text, index_pos)
        if self.weight != 1.0:
            li, lt = li * self.weight, lt * self.weight
        return {"loss_dist_i": li, "loss_dist_t": lt}


class CriterionAlignment(nn.Module):
    """model_clip.py:664-715: IPOT optimal-transport distance between entity-text and object
    features (object slot 0 = whole image is dropped), summed over the batch, times 0.01."""

    def forward(self, entitytxt_vec, object_vec, entitytxt_num, object_num):
        from .ot import optimal_transport_dist
        img = object_vec[:, 1:]
        txt_pad = entitytxt_num == 0
        img_pad = object_num[:, 1:] == 0
        ot_dist = optimal_transport_dist(entitytxt_vec, img, txt_pad, img_pad).to(entitytxt_vec.dtype)
        return {"loss_ot": ot_dist.sum() * 0.01}
