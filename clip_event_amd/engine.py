"""The per-iteration body of the reference's ``train_one_epoch`` (engine.py:48-95) on the HIP path:
forward, contrastive criterion (+ optional OT alignment), loss SUM (engine.py:67), backward,
global-norm clip to 1 and Adam (fused, optim.py).  With more than one rank the features are
all-gathered for a global-batch InfoNCE and parameter gradients are averaged (distributed.py)."""
from __future__ import annotations

import contextlib
import functools
import logging
import math
import operator
import os
import sys
from typing import Dict, Optional

import numpy as np
import torch

from . import distributed as D
from .functional import (attach_lengths, distill_losses, fused_contrastive_losses, fused_head_ok, logits_from_features,
                         multipos_contrastive_losses, sigmoid_contrastive_losses, small_contrastive_losses, small_head_ok, tokens_to_device)
from .losses import CriterionAlignment, CriterionContrastive, CriterionDistill


def _unwrap(model):
    """``DistributedDataParallel(model)`` (ours, train.py:222-225) -> the CLIP module (engine.py:52,57-61)."""
    return model.module if isinstance(model, D.DistributedDataParallel) else model


class Distillation:
    """Knowledge distillation from a frozen teacher (open_clip's ``--distill-model`` / ``DistillClipLoss``): ``train_step(...,
    distill=Distillation(teacher))`` adds ``weight`` times the cross entropy of the student's softmax against the teacher's, in
    both directions, as ``loss_dist_i`` / ``loss_dist_t``.

    ``teacher`` is this package's ``CLIP`` on the student's device; it is put in ``eval()`` with ``requires_grad_(False)`` and
    encodes under ``torch.no_grad()`` (the stash-free towers), every patch of every image.  ``logit_scale`` (the LOG of the scale,
    as ``CLIP.logit_scale`` holds it) replaces the teacher's own; with ``teacher=None`` it is required and every step needs
    ``teacher_features=`` (precomputed features)."""

    def __init__(self, teacher, weight: float = 1.0, logit_scale=None):
        from .model import CLIP
        if not float(weight) >= 0:
            raise ValueError(f"Distillation: weight must be >= 0 (got {weight})")
        if teacher is None:
            if logit_scale is None:
                raise ValueError("Distillation(teacher=None) is for precomputed teacher features and needs the teacher's logit_scale")
        else:
            if not isinstance(teacher, CLIP):
                raise TypeError(f"Distillation: the teacher must be clip_event_amd's CLIP (got {type(teacher).__name__})")
            if float(getattr(teacher.visual, "patch_dropout", 0.0)) > 0.0:
                raise ValueError("Distillation: the teacher has patch dropout switched on (set_patch_dropout(0.0)): it must see "
                                 "every patch")
            teacher.eval()
            teacher.requires_grad_(False)
        self.teacher = teacher
        self.weight = float(weight)
        self._logit_scale = None if logit_scale is None else torch.as_tensor(float(logit_scale), dtype=torch.float32)

    def logit_scale(self, device) -> torch.Tensor:
        ls = self.teacher.logit_scale.detach() if self._logit_scale is None else self._logit_scale
        return ls.to(device=device, dtype=torch.float32)

    def check_optimizer(self, optimizer):
        """A teacher the optimiser would update is no teacher: raises when any of its parameters is in ``optimizer``."""
        if self.teacher is None:
            return
        if getattr(optimizer, "model", None) is self.teacher:
            raise ValueError("Distillation: the optimiser was built on the teacher")
        mine = {id(p) for p in self.teacher.parameters()}
        for group in getattr(optimizer, "param_groups", []):
            if any(id(p) in mine for p in group["params"] if isinstance(p, torch.Tensor)):
                raise ValueError("Distillation: a parameter of the teacher is in the optimiser's parameter list")

    def check_student(self, model):
        if self.teacher is None:
            return
        if self.teacher is model:
            raise ValueError("Distillation: the teacher is the student")
        dev, tdev = next(model.parameters()).device, next(self.teacher.parameters()).device
        if dev != tdev:
            raise ValueError(f"Distillation: the teacher is on {tdev}, the student on {dev}")

    def encode(self, image, text, teacher_image=None):
        """The teacher's (image, text) features of a batch, no gradient, no stash."""
        t = self.teacher
        if t is None:
            raise ValueError("Distillation(teacher=None) holds no teacher: pass teacher_features=(image features, text features)")
        img = image if teacher_image is None else teacher_image
        res = int(t.visual.input_resolution)
        if tuple(img.shape[-2:]) != (res, res):
            which = "teacher_image" if teacher_image is not None else "image"
            raise ValueError(f"Distillation: the teacher takes {res} x {res} images and {which} is {tuple(img.shape[-2:])}; "
                             f"pass teacher_image= at the teacher's resolution")
        if img.shape[0] != image.shape[0]:
            raise ValueError(f"Distillation: teacher_image has {img.shape[0]} images, the batch {image.shape[0]}")
        if t.training:
            t.eval()
        with torch.no_grad():
            tfi, tft = t.encode_both(img, text)
        return tfi, tft


# Logits per direction from which the 'ce' criterion over the batch runs on the fused head, SURVEY 8(a) a6.  The fused head
# exists to keep a big logits matrix out of HBM (config 3 per rank: 512 x 20,480); at B = 256, K = 1 the matrix is 256 KB and the
# plain path's kernels are the faster ones (same-box A/B: 12.75 / 12.53 vs 12.79 / 12.67 ms/step), so the fused head takes over
# from 2^17 logits per direction (256 x 1280 and 512 x 512: fused ahead by 0.1-0.2 ms).  CE_FUSED_HEAD=1 / 0 forces either.
CE_FUSED_MIN_LOGITS = 1 << 17

# Logits per direction from which distillation runs on the fused head.  Measured (DESIGN 4h "Numbers"), the fused head is the
# slower one at every size up to 4096 x 20480 (1.1-1.9 x logits + CriterionDistill): there is no crossover in speed, so the switch
# is by memory.  At 2^28 logits one fp32 matrix is 1 GiB and the materialised path holds four of them and two gradients of that
# size, 6 GiB on the stretch where both towers' stashes are alive; from there the fused head, which holds none, takes over.
# CE_FUSED_HEAD=1 / 0 forces either.
DISTILL_FUSED_MIN_LOGITS = 1 << 28


def head_route(kind, *, rows, keys, width, teacher_width=None, dist_global=False, overbatch=True, has_index_pos=True,
               small_ok=False, fused_env="", small_env="1") -> str:
    """Which head a loss runs on: "small" (the three-launch head), "fused" (no logits matrix) or "logits" (logits + criterion).
    Pure: everything it looks at is an argument.  ``kind``: the criterion's ("ce", "sigmoid", "multipos", "bce", "kl", ...) or "distill";
    ``rows`` x ``keys``: local query rows and all key rows of one direction (the logits the direction would materialise);
    ``width`` / ``teacher_width``: the feature widths; ``dist_global``: the keys are gathered across ranks; ``small_ok``:
    ``small_head_ok`` of the shapes; ``fused_env`` / ``small_env``: the values of CE_FUSED_HEAD ("" unset) and CE_SMALL_HEAD."""
    logits = rows * keys
    if kind in ("sigmoid", "multipos"):    # the fused head at every size the kernels take: the three-launch small head is 'ce'-only
        return "fused" if fused_env != "0" and fused_head_ok(width) else "logits"
    if kind == "distill":
        fused = (fused_env != "0" and (fused_env == "1" or logits >= DISTILL_FUSED_MIN_LOGITS) and fused_head_ok(width)
                 and fused_head_ok(teacher_width))
        return "fused" if fused else "logits"
    if kind != "ce" or not overbatch:
        return "logits"
    if fused_env != "0" and (fused_env == "1" or logits >= CE_FUSED_MIN_LOGITS) and fused_head_ok(width):
        return "fused"
    # below that size, in one process: the three-launch head (CE_SMALL_HEAD=0 or CE_FUSED_HEAD=0: the general logits + criterion path)
    if not dist_global and fused_env == "" and small_env != "0" and has_index_pos and small_ok:
        return "small"
    return "logits"


def _distill_from_features(model, distill, fi, ft, tfi, tft, index_pos, pair):
    """``weight`` x the two distillation terms from the student's and the teacher's raw features.  ``pair``: the student's
    gathered (image, text) features when a process group is live (the queries are the local rows; the teacher's features are
    gathered here, without grad, in one collective), else None.  Logits + ``CriterionDistill`` below ``DISTILL_FUSED_MIN_LOGITS``
    logits per direction or where the fused head does not take a width, the fused head above; CE_FUSED_HEAD=1 / 0 forces either."""
    if not model.constrastive_overbatch:
        raise RuntimeError("distillation needs constrastive_overbatch=True: the per-instance layout has no distribution over the batch")
    tls = distill.logit_scale(fi.device)
    if pair is None:
        fi_all, ft_all, tfi_all, tft_all = fi, ft, tfi, tft
    else:
        fi_all, ft_all = pair
        with torch.no_grad():
            tfi_all, tft_all = D.gather_feature_pair(tfi.float().contiguous(), tft.float().contiguous())
    if head_route("distill", rows=int(fi.shape[0]), keys=int(ft_all.shape[0]), width=int(fi.shape[1]),
                  teacher_width=int(tfi.shape[1]), fused_env=os.environ.get("CE_FUSED_HEAD", "")) == "fused":
        out = distill_losses(fi, ft, fi_all, ft_all, model.logit_scale, tfi, tft, tfi_all, tft_all, tls, index_pos)
    else:
        with torch.no_grad():                                                     # the teacher's side is a constant
            tlpi, _ = logits_from_features(tfi, tft_all, tls, True, want="image")
            _, tlpt = logits_from_features(tfi_all, tft, tls, True, want="text")
        lpi, _ = logits_from_features(fi, ft_all, model.logit_scale, True, want="image")
        _, lpt = logits_from_features(fi_all, ft, model.logit_scale, True, want="text")
        out = CriterionDistill()(lpi, lpt, tlpi, tlpt, index_pos=index_pos)
    return {k: v * distill.weight for k, v in out.items()}


def _contrastive_from_features(model, criterion, fi, ft, labels_per_image, labels_per_text, index_pos, global_batch, teacher=None):
    """Loss dict of the contrastive criterion from the two towers' (raw) features: all-gather over the ranks when a
    process group is live, then the fused head (no logits matrix in HBM) or logits + criterion.  ``teacher`` =
    (``Distillation``, teacher image features, teacher text features) adds the distillation terms, computed from the features
    alone; None leaves every launch what it is without it."""
    if teacher is not None:
        distill, tfi, tft = teacher
        pair = D.gather_feature_pair(fi, ft) if (D.active() and global_batch) else None
        loss_dict = _criterion_from_features(model, criterion, fi, ft, labels_per_image, labels_per_text, index_pos, global_batch, pair)
        loss_dict.update(_distill_from_features(model, distill, fi, ft, tfi, tft, index_pos, pair))
        return loss_dict
    return _criterion_from_features(model, criterion, fi, ft, labels_per_image, labels_per_text, index_pos, global_batch, None)


def _criterion_from_features(model, criterion, fi, ft, labels_per_image, labels_per_text, index_pos, global_batch, pair):
    """``pair``: the gathered (image, text) features when the caller has them already, else None."""
    dist_global = D.active() and global_batch
    if getattr(criterion, "kind", None) == "sigmoid":
        return _sigmoid_from_features(model, criterion, fi, ft, labels_per_image, dist_global, None if pair is None else pair[1],
                                      labels_per_text)
    if getattr(criterion, "kind", None) == "multipos":
        return _multipos_from_features(model, criterion, fi, ft, labels_per_image, labels_per_text, index_pos, dist_global, pair)
    route = head_route(getattr(criterion, "kind", None), rows=int(fi.shape[0]),
                       keys=int(ft.shape[0]) * (D.world_size() if dist_global else 1), width=model.embed_dim,
                       dist_global=dist_global, overbatch=model.constrastive_overbatch, has_index_pos=index_pos is not None,
                       small_ok=small_head_ok(fi, ft, index_pos), fused_env=os.environ.get("CE_FUSED_HEAD", ""),
                       small_env=os.environ.get("CE_SMALL_HEAD", "1"))
    if route == "small":
        return small_contrastive_losses(fi, ft, model.logit_scale, labels_per_image, labels_per_text, index_pos)
    fi_all, ft_all = pair if pair is not None else (D.gather_feature_pair(fi, ft) if dist_global else (fi, ft))
    if route == "fused":
        return fused_contrastive_losses(fi, ft, fi_all, ft_all, model.logit_scale, labels_per_image, labels_per_text, index_pos)
    overbatch = model.constrastive_overbatch
    if dist_global:
        lpi, _ = logits_from_features(fi, ft_all if overbatch else ft, model.logit_scale, overbatch, want="image")
        _, lpt = logits_from_features(fi_all, ft, model.logit_scale, True, want="text")
    else:
        lpi, lpt = logits_from_features(fi, ft, model.logit_scale, overbatch)
    return criterion(lpi, lpt, labels_per_image, labels_per_text, index_pos=index_pos, constrastive_overbatch=overbatch)


def _multipos_from_features(model, criterion, fi, ft, groups_per_image, groups_per_text, index_pos, dist_global, pair):
    """``CriterionMultiPositive``: the local images against all texts and the ``index_pos`` rows of the local texts against all
    images, each row's target uniform over the keys that carry its group id.  Across ranks the features are gathered as for
    'ce' and the two id vectors in one more collective, without grad.  The fused head at every size the kernels take, else
    logits + criterion; CE_FUSED_HEAD=0 forces the latter."""
    if not model.constrastive_overbatch:
        raise RuntimeError("the multi-positive loss needs constrastive_overbatch=True: the per-instance layout has no negatives "
                           "from other images")
    if groups_per_image is None or groups_per_text is None:
        raise RuntimeError("the multi-positive loss needs the group ids of the images and of the texts (distributed.global_groups)")
    fi_all, ft_all = pair if pair is not None else (D.gather_feature_pair(fi, ft) if dist_global else (fi, ft))
    gi_all, gt_all = groups_per_image, groups_per_text
    if dist_global:
        with torch.no_grad():
            gi_all, gt_all = D.gather_group_ids(groups_per_image.to(fi.device), groups_per_text.to(fi.device))
    if head_route("multipos", rows=int(fi.shape[0]), keys=int(ft_all.shape[0]), width=model.embed_dim,
                  fused_env=os.environ.get("CE_FUSED_HEAD", "")) == "fused":
        return multipos_contrastive_losses(fi, ft, fi_all, ft_all, model.logit_scale, groups_per_image, groups_per_text, gi_all,
                                           gt_all, index_pos)
    if dist_global:
        lpi, _ = logits_from_features(fi, ft_all, model.logit_scale, True, want="image")
        _, lpt = logits_from_features(fi_all, ft, model.logit_scale, True, want="text")
    else:
        lpi, lpt = logits_from_features(fi, ft, model.logit_scale, True)
    return criterion(lpi, lpt, groups_per_image, groups_per_text, index_pos=index_pos, constrastive_overbatch=True,
                     all_groups=(gi_all, gt_all))


def _sigmoid_from_features(model, criterion, fi, ft, labels_per_image, dist_global, ft_all=None, labels_per_text=None):
    """``CriterionSigmoid``: the local images against all texts, one direction.  Across ranks only the TEXT features are gathered
    (half of ``gather_feature_pair``'s bytes): the rank's loss is over its own rows, DDP's mean over the ranks makes it the global
    loss, and the reduce-scatter in the gather's backward brings the other ranks' text gradients home.  The fused head (three
    sweeps, no logits matrix) at every size the kernels take -- the three-launch small head is 'ce'-only -- else logits +
    criterion.  CE_FUSED_HEAD=0 forces the latter."""
    if not model.constrastive_overbatch:
        raise RuntimeError("the sigmoid loss needs constrastive_overbatch=True: the per-instance layout has no negatives from other "
                           "images")
    bias = getattr(model, "logit_bias", None)
    if bias is None:
        raise RuntimeError("the sigmoid loss needs a logit bias: call model.enable_logit_bias() before building the optimiser")
    if ft_all is None:
        ft_all = D.gather_features(ft) if dist_global else ft
    if getattr(criterion, "multi_positive", False):
        # the labels are group ids: a pair is positive wherever the ids match.  Across ranks the ids travel in one more collective
        if labels_per_image is None or labels_per_text is None:
            raise RuntimeError("CriterionSigmoid(multi_positive=True) needs the group ids of the images and of the texts")
        groups = (labels_per_image, labels_per_text)
        if dist_global:
            with torch.no_grad():
                groups = (labels_per_image, D.gather_group_ids(labels_per_image.to(fi.device), labels_per_text.to(fi.device))[1])
        if head_route("sigmoid", rows=int(fi.shape[0]), keys=int(ft_all.shape[0]), width=model.embed_dim,
                      fused_env=os.environ.get("CE_FUSED_HEAD", "")) == "fused":
            return sigmoid_contrastive_losses(fi, ft_all, model.logit_scale, bias, None, groups)
        lpi, _ = logits_from_features(fi, ft_all, model.logit_scale, True, want="image")
        return criterion(lpi, None, labels_per_image, labels_per_text, constrastive_overbatch=True, logit_bias=bias,
                         all_groups=(None, groups[1]))
    if head_route("sigmoid", rows=int(fi.shape[0]), keys=int(ft_all.shape[0]), width=model.embed_dim,
                  fused_env=os.environ.get("CE_FUSED_HEAD", "")) == "fused":
        return sigmoid_contrastive_losses(fi, ft_all, model.logit_scale, bias, labels_per_image)
    lpi, _ = logits_from_features(fi, ft_all, model.logit_scale, True, want="image")
    return criterion(lpi, None, labels_per_image, constrastive_overbatch=True, logit_bias=bias)


def contrastive_step_losses(model, criterion: CriterionContrastive, image, text, labels_per_image, labels_per_text,
                            index_pos, global_batch: bool = True, train_arg=None, bboxs=None, bbox_desc_vec=None,
                            bbox_label_vec=None, teacher=None) -> Dict[str, torch.Tensor]:
    """Forward + criterion.  ``global_batch`` (W > 1): logits_per_image = s * I_local @ T_all^T,
    logits_per_text = s * T_local @ I_all^T with labels from ``distributed.global_labels``.  With ``train_arg``
    (model_clip.py:419-488) the two region / argument losses join the dict as ``loss_bbox`` / ``loss_arg``; they
    are per-image sums over the local batch, no exchange."""
    model = _unwrap(model)
    extra = {}
    if train_arg is None:
        fi, ft = model.encode_both(image, text)
    else:
        fi, ft, loss_bbox, loss_arg = model.encode_with_regions(image, text, train_arg, bboxs, bbox_desc_vec, bbox_label_vec)
        extra = {"loss_bbox": loss_bbox, "loss_arg": loss_arg}
    loss_dict = _contrastive_from_features(model, criterion, fi, ft, labels_per_image, labels_per_text, index_pos, global_batch,
                                           teacher=teacher)
    loss_dict.update(extra)
    return loss_dict


# How far the host may run ahead of the GPU.  Nothing in a step needs the host to wait (with host-side caption lengths the text
# tower no longer reads anything back), but an unthrottled host queues the whole run and that measured SLOWER: 12.93-12.94
# ms/step against 12.48-12.56 with the per-step read-back (which happened to hold the host about a step behind), same box.
# CE_STEPS_AHEAD = n (default 2; 0 = unlimited) makes the distance explicit: before enqueueing a step the host waits for the
# end of the step n before it.  Same-box A/B: n = 1 12.76-13.0 (the GPU drains at every step boundary), n = 2 / 3 / 4 12.50-12.56
# (second box 12.28-12.34, all three equal).
_STEPS_AHEAD = int(os.environ.get("CE_STEPS_AHEAD", "2"))


def _throttle(model):
    if _STEPS_AHEAD <= 0 or not torch.cuda.is_available():
        return
    evs = model.__dict__.setdefault("_step_events", [])
    while len(evs) >= _STEPS_AHEAD:
        evs.pop(0).synchronize()


def _mark_step_end(model):
    if _STEPS_AHEAD <= 0 or not torch.cuda.is_available():
        return
    ev = torch.cuda.Event()
    ev.record()
    model.__dict__.setdefault("_step_events", []).append(ev)


def _cat_tokens(parts):
    """One [n, T] token matrix for one text-tower pass; the host-side lengths travel along when every part has them."""
    if len(parts) == 1:
        return parts[0]
    out = torch.cat(parts, dim=0)
    lens = [getattr(p, "_ce_lengths", None) for p in parts]
    if all(l is not None for l in lens):
        attach_lengths(out, np.concatenate([np.asarray(l).reshape(-1) for l in lens]))
    return out


def merged_step_losses(model, criterion, criterion_ot, image, text, labels_per_image, labels_per_text, index_pos,
                       train_arg=None, bboxs=None, bbox_desc_vec=None, bbox_label_vec=None, object_vec=None,
                       entitytxt_vec=None, object_num=None, entitytxt_num=None, global_batch: bool = True, teacher=None):
    """BASELINE config 4's forward with ONE pass per tower.  The reference (and ``CLIP.forward`` / ``sim_entity`` here) runs
    the image tower twice (batch, object crops: engine.py:57-63) and the text tower up to four times (captions, entity
    mentions, role descriptions, role labels: model_clip.py:430-455, :531-552).  Tower rows are independent of each other,
    so the same values come out of one image pass over [images | crops] and one text pass over [captions | mentions | roles |
    labels]: a 64-image pass fills a quarter of the GPU and a 100-caption pass is ~200 launches of a few microseconds each,
    while the merged passes fill their tiles, and each tower's weight gradients are written once instead of accumulated.
    With ``train_arg`` the image pass keeps every token (the region branch pools the grid of the batch images; the crops'
    CLS features are row 0 of theirs).  ``teacher`` (as in ``_contrastive_from_features``) holds the teacher's features of the
    image and caption rows only: the region and alignment branches are not distilled."""
    from .region import region_losses_from_features, region_plan
    dev = image.device
    B = image.shape[0]
    want_align = criterion_ot is not None and model.alignment
    images, texts = [image], [text]
    n_obj = n_ent = 0
    if want_align:
        n_obj, n_ent = object_vec.size(1), entitytxt_vec.size(1)
        images.append(object_vec.reshape(B * n_obj, *object_vec.shape[2:]))
        ent = entitytxt_vec.reshape(B * n_ent, entitytxt_vec.size(2))
        if getattr(entitytxt_vec, "_ce_lengths", None) is not None:
            attach_lengths(ent, entitytxt_vec._ce_lengths)
        texts.append(ent)
    plan = region_plan(model, bboxs, bbox_desc_vec, bbox_label_vec, train_arg, dev) if train_arg is not None else None
    if plan is not None:
        texts.append(plan.descs)
        if plan.use_label:
            texts.append(plan.labs)
    img_all = torch.cat([_f for _f in images], dim=0) if len(images) > 1 else image
    txt_all = _cat_tokens(texts)
    fi_all, ft_all = model.encode_both(img_all, txt_all, use_grid=train_arg is not None)
    loss_dict = {}
    # split the features back (views: autograd sums their gradients into one tensor per tower)
    n_cap = text.shape[0]
    ft = ft_all[:n_cap]
    pos = n_cap
    if train_arg is not None:
        pn = model.visual.patch_num
        fi = fi_all[:B, 0, :]
        grid = fi_all[:B, 1:, :].reshape(B, pn, pn, -1)
        obj_f = fi_all[B:, 0, :]
    else:
        fi, grid, obj_f = fi_all[:B], None, fi_all[B:]
    loss_dict.update(_contrastive_from_features(model, criterion, fi, ft, labels_per_image, labels_per_text, index_pos, global_batch,
                                                teacher=teacher))
    ent_f = None
    if want_align:
        ent_f = ft_all[pos:pos + B * n_ent].view(B, n_ent, -1)
        pos += B * n_ent
    if train_arg is not None:
        if plan is None:
            zero = torch.zeros((), dtype=torch.float32, device=dev)
            loss_dict.update(loss_bbox=zero, loss_arg=zero)
        else:
            nd = plan.descs.shape[0]
            desc_f = ft_all[pos:pos + nd]
            lab_f = ft_all[pos + nd:pos + 2 * nd] if plan.use_label else None
            lb, la = region_losses_from_features(model, grid, plan, desc_f, lab_f)
            loss_dict.update(loss_bbox=lb, loss_arg=la)
    if want_align:
        loss_dict.update(criterion_ot(ent_f, obj_f.reshape(B, n_obj, -1), entitytxt_num, object_num))      # engine.py:57-63
    return loss_dict


def _sum_losses(loss_dict, check_finite: bool):
    """engine.py:67-82: the loss SUM, and with ``check_finite`` the all-rank mean of the losses, ``.item()``, stop on a
    non-finite value."""
    losses = functools.reduce(operator.add, loss_dict.values())                            # engine.py:67 (sum() would add an int 0 first: one more launch)
    if check_finite:
        reduced = D.reduce_dict({k: v.detach() for k, v in loss_dict.items()})
        loss_value = float(sum(v for v in reduced.values()))
        if not math.isfinite(loss_value):
            logging.error("Loss is {}, stopping training".format(loss_value))
            logging.error(reduced)
            sys.exit(1)
    return losses


def micro_batched_backward(model, criterion, image, text, labels_per_image, labels_per_text, index_pos, micro_batch: int,
                           grad_sync: Optional[D.GradSync] = None, check_finite: bool = False,
                           global_batch: bool = True, distill=None, teacher_image=None,
                           teacher_features=None) -> Dict[str, torch.Tensor]:
    """Forward + backward of the plain contrastive step for a batch whose activation stash does not fit: the stash is
    32-36 x width bytes per row AND block (0.45 GB per ViT-L/14@336 image), and the contrastive loss needs the features of
    the WHOLE batch, so accumulating the gradients of small steps would be a different loss.  Instead:

      1. features of every chunk of ``micro_batch`` images (and their ``micro_batch * K`` captions) without grad -- the
         forward-only tower, which keeps no stash (``ce_tower_forward_infer``);
      2. the head ONCE over all of them, and its backward: the gradients of the loss w.r.t. every feature row (and the
         ``logit_scale`` gradient);
      3. per chunk a second forward, now with the stash, and its backward with those feature gradients injected.  One
         stash per tower lives at a time; the parameter gradients of the chunks accumulate in the flat buffer (the first
         chunk's backward writes the block weights, ``zero_grad_first_touch``).

    The towers treat rows independently, so the cut needs no knowledge of the label layout, and the loss dict is the
    unchunked step's up to what a different tile choice at a smaller M does to the bf16 roundings.  Costs one extra tower
    forward: 4/3 of the unchunked step's tower FLOPs.  The caller has zeroed the gradients and runs the optimiser.

    With ``distill`` the teacher encodes each chunk in pass 1 (``teacher_features`` given: no teacher pass); the head, the
    distillation terms included, still runs once over the whole batch."""
    B, n = int(image.shape[0]), int(text.shape[0])
    mb = int(micro_batch)
    if mb < 1:
        raise ValueError(f"micro_batch must be at least 1 (got {micro_batch})")
    if n % B != 0:
        raise RuntimeError(f"micro_batch needs the same number of captions per image ({n} captions, {B} images)")
    K = n // B
    lens = getattr(text, "_ce_lengths", None)
    if lens is None:                       # tokens on the device without host lengths: ONE read-back for the whole batch
        lens = (text.reshape(n, -1).argmax(dim=-1) + 1).cpu().numpy()
    lens = np.asarray(lens).reshape(-1)
    if text.dtype != torch.int64:          # the text tower would convert every view anew, and the copy carries no lengths
        text = text.long()
    chunks = []
    for lo in range(0, B, mb):
        hi = min(lo + mb, B)
        chunks.append((lo, hi, image[lo:hi], attach_lengths(text[lo * K:hi * K], lens[lo * K:hi * K])))
    gs = grad_sync if grad_sync is not None else getattr(model, "grad_sync", None)
    # a locked tower (model.trainable_plan: nothing in it trains) is encoded once, in pass 1, and has no backward
    locked = model.trainable_plan().locked
    live = [t for t in ("visual", "text") if not locked[t]]
    if gs is not None and hasattr(gs, "expect_passes") and live:
        gs.expect_passes({t: len(chunks) for t in live})
    # every chunk, the shorter last one included, runs in buffers leased for a full chunk (the pool is keyed by byte count)
    model._lease_batch = {"vision": mb, "text": mb * K}
    # ... and on the attention kernels the step's longest caption selects (functional.text_tower_tokens), not the chunk's own: a chunk
    # of short captions would otherwise take the one-workgroup kernels where the unchunked step takes the tiled ones, and the
    # chunked step would differ from it by more than a tile choice
    model._route_longest = int(lens.max()) if len(lens) else None
    # patch dropout: ONE draw for the step; both passes of the chunk [lo, hi) run pinned to it with their samples counted from
    # lo, so the chunked step drops exactly the patches the unchunked step drops
    draw = model.next_patch_draw() if model.drops_patches() else None

    def pinned(lo):
        return contextlib.nullcontext() if draw is None else model.pinned_patch_draw(draw[0], sample0=draw[1] + lo)

    try:
        with torch.no_grad():
            feats = []
            for lo, _, img_c, txt_c in chunks:
                with pinned(lo):
                    feats.append(model.encode_both(img_c, txt_c))
            teacher = None
            if distill is not None:
                if teacher_features is None:
                    tf = [distill.encode(img_c, txt_c, None if teacher_image is None else teacher_image[lo:hi])
                          for lo, hi, img_c, txt_c in chunks]
                    teacher_features = (torch.cat([f[0] for f in tf], dim=0), torch.cat([f[1] for f in tf], dim=0))
                teacher = (distill, teacher_features[0], teacher_features[1])
        fi = torch.cat([f[0] for f in feats], dim=0).requires_grad_(not locked["visual"])
        ft = torch.cat([f[1] for f in feats], dim=0).requires_grad_(not locked["text"])
        del feats
        loss_dict = _contrastive_from_features(model, criterion, fi, ft, labels_per_image, labels_per_text, index_pos, global_batch,
                                               teacher=teacher)
        _sum_losses(loss_dict, check_finite).backward()        # fi.grad, ft.grad, logit_scale.grad; no tower node, no exchange
        for lo, hi, img_c, txt_c in (chunks if live else []):
            if len(live) == 2:
                with pinned(lo):
                    outs = model.encode_both(img_c, txt_c)
                grads = [fi.grad[lo:hi], ft.grad[lo * K:hi * K]]
            elif live[0] == "visual":
                with pinned(lo):
                    outs = [model.encode_image(img_c)]
                grads = [fi.grad[lo:hi]]
            else:
                outs, grads = [model.encode_text(txt_c)], [ft.grad[lo * K:hi * K]]
            torch.autograd.backward(list(outs), grads)
            del outs
    finally:
        model._lease_batch = None
        model._route_longest = None
    return loss_dict


def train_step(model, criterion, optimizer, image, text, labels_per_image, labels_per_text, index_pos,
               grad_sync: Optional[D.GradSync] = None, criterion_ot: Optional[CriterionAlignment] = None,
               object_vec=None, entitytxt_vec=None, object_num=None, entitytxt_num=None,
               check_finite: bool = False, train_arg=None, bboxs=None, bbox_desc_vec=None,
               bbox_label_vec=None, text_lengths=None, micro_batch: Optional[int] = None, distill: Optional[Distillation] = None,
               teacher_image=None, teacher_features=None) -> Dict[str, torch.Tensor]:
    """One iteration of engine.py:48-95.  BASELINE config 4 is this call with ``criterion_ot`` + the object / entity
    tensors (``model.alignment``) and ``train_arg`` + boxes in ONE step, as the reference's forward takes them
    (model_clip.py:419-528, engine.py:57-63).  ``check_finite`` reproduces engine.py:70-81 (all-rank mean of the
    losses, ``.item()``, stop on a non-finite value); it costs the host synchronisation the reference pays every
    step, so it is off by default.

    Token tensors may arrive on the HOST, as the reference's data loader yields them (engine.py:52 copies them): their
    caption lengths are then taken on the host and travel with the asynchronous copy, so the text tower never reads
    anything back from the device.  For tokens already on the GPU pass ``text_lengths`` (host integers, tokens up to and
    including the EOT) or tag the tensor with ``functional.attach_lengths``; without either the lengths are read back
    (one small synchronous copy per new tensor).

    ``micro_batch`` (images per chunk; None or >= the number of images: the step above, untouched) runs the plain contrastive
    step for a batch whose activation stash does not fit the card: see ``micro_batched_backward``.  Same loss over the whole
    batch, one extra tower forward.  Not available with ``train_arg`` / ``criterion_ot``.

    ``distill`` (a ``Distillation``) adds ``loss_dist_i`` / ``loss_dist_t``: the teacher encodes ``teacher_image`` (None: ``image``,
    which must then have the teacher's resolution) and the captions without grad, or ``teacher_features=(image features, text
    features)`` are taken as given and no teacher pass runs.  With ``distill=None`` the step is what it is without the argument."""
    wrapped = model
    model = _unwrap(model)
    chunked = micro_batch is not None and int(micro_batch) < int(image.shape[0])
    if chunked and (train_arg is not None or criterion_ot is not None):
        raise NotImplementedError("train_step(micro_batch=...) covers the plain contrastive step only: the region / alignment "
                                  "losses of train_arg / criterion_ot couple rows inside the towers' outputs; run that "
                                  "configuration without micro_batch")
    dev = next(model.parameters()).device
    _throttle(model)
    if text_lengths is not None:
        attach_lengths(text, text_lengths)
    text = tokens_to_device(text, dev)
    if entitytxt_vec is not None:
        entitytxt_vec = tokens_to_device(entitytxt_vec, dev)
    if grad_sync is None and wrapped is not model:
        grad_sync = wrapped.grad_sync
    teacher = None                         # checked, and the teacher run, before anything of the step is touched
    if distill is not None:
        distill.check_student(model)
        distill.check_optimizer(optimizer)
        if teacher_features is not None:
            teacher = (distill, teacher_features[0], teacher_features[1])
        elif not chunked:
            teacher = (distill,) + tuple(distill.encode(image, text, teacher_image))
    elif teacher_image is not None or teacher_features is not None:
        raise ValueError("teacher_image / teacher_features need distill=Distillation(...)")
    if hasattr(optimizer, "zero_grad_first_touch"):
        optimizer.zero_grad_first_touch()      # nothing reads .grad between here and backward(): block weights are overwritten
    else:
        optimizer.zero_grad()
    want_align = model.alignment and criterion_ot is not None
    if chunked:
        loss_dict = micro_batched_backward(model, criterion, image, text, labels_per_image, labels_per_text, index_pos,
                                           int(micro_batch), grad_sync=grad_sync, check_finite=check_finite, distill=distill,
                                           teacher_image=teacher_image, teacher_features=teacher_features)
    elif (want_align or train_arg is not None) and os.environ.get("CE_MERGE_PASSES", "1") != "0":
        # config 4: one pass per tower over [images | object crops] and [captions | entity mentions | role texts]
        loss_dict = merged_step_losses(model, criterion, criterion_ot if want_align else None, image, text, labels_per_image,
                                       labels_per_text, index_pos, train_arg=train_arg, bboxs=bboxs, bbox_desc_vec=bbox_desc_vec,
                                       bbox_label_vec=bbox_label_vec, object_vec=object_vec, entitytxt_vec=entitytxt_vec,
                                       object_num=object_num, entitytxt_num=entitytxt_num, teacher=teacher)
    else:
        loss_dict = contrastive_step_losses(model, criterion, image, text, labels_per_image, labels_per_text, index_pos,
                                            train_arg=train_arg, bboxs=bboxs, bbox_desc_vec=bbox_desc_vec,
                                            bbox_label_vec=bbox_label_vec, teacher=teacher)
        if want_align:
            image_features, text_features = model.sim_entity(object_vec, entitytxt_vec)       # engine.py:57-63
            loss_dict.update(criterion_ot(text_features, image_features, entitytxt_num, object_num))
    if not chunked:
        _sum_losses(loss_dict, check_finite).backward()
    if check_finite and getattr(model, "stream16", False):
        # the fp16 streams clamp instead of overflowing, so a clipped activation / gradient never shows up as a non-finite
        # loss: read the device-side clamp counters on the synchronisation this mode pays anyway, before the update is applied
        sat_f, sat_g = model.stream16_saturation()
        if sat_f or sat_g:
            logging.error("fp16 stream saturated ({} forward, {} gradient slots), stopping training".format(sat_f, sat_g))
            sys.exit(1)
    if hasattr(model, "_settle_first_touch"):
        model._settle_first_touch()    # a tower without a backward pass in this step: its weight gradients are zero
    if grad_sync is not None:
        grad_sync.finish()             # no-op when the autograd final callback has already run it
    optimizer.step()                                                                       # clip + Adam
    _mark_step_end(model)
    return loss_dict
