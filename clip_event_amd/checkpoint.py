"""Checkpoint interchange with the reference.

Same file layout as ``save_model_on_master`` (engine.py:202-218): ``{'epoch', 'model', 'state_dict', 'perf',
'optimizer'}`` written with ``torch.save`` as ``<task>_<epoch>.pth``; the ``state_dict`` has the reference's keys
and shapes, ``optimizer`` is ``torch.optim.Adam``'s format (optim.FusedAdam speaks it) or ``torch.optim.SGD``'s
(optim.FusedSGD: per-parameter ``momentum_buffer``, an empty state before the first step), so files move both ways; with
optim.FusedLion it is the layout of the common Lion implementations (timm, lion-pytorch): per-parameter ``exp_avg``, group keys
``lr`` / ``betas`` / ``weight_decay``, an empty state before the first step.
Loading follows train.py:101-124 (resume) and also accepts a bare state dict such as the OpenAI ViT-B/32 weights
(fp16 tensors are widened to the fp32 masters by ``build_model``).  Files are read with ``weights_only=True``:
nothing in a checkpoint is executed.

An optimiser with a weight average (``optimizer.enable_ema``) adds one entry, ``'ema'``: ``optimizer.ema_state_dict()`` with
its tensors on the CPU, read back by ``load_ema``.  Without one the file has exactly the reference's five keys.  A checkpoint
OF the averaged weights in the reference's layout is ``with optimizer.averaged(): save_model_on_master(...)``.

A model with low-rank adapters (``CLIP.enable_lora``) adds one entry, ``'lora'``: ``model.lora_config()``; its ``state_dict``
then holds the adapters beside the base weights, and ``load_checkpoint`` rebuilds base model, adapters and their values from
the two.  ``model.lora_state_dict()`` alone is the few-MB per-task file; ``model.merge_lora()`` gives a plain model again.
"""
from __future__ import annotations

import logging
import os
from typing import Any, Dict, Optional, Tuple

import torch

from . import distributed as D
from .model import build_model

CKPT_KEYS = ("epoch", "model", "state_dict", "perf", "optimizer")


def checkpoint_dict(model, optimizer, task: str, epoch: int, best_perf: float) -> Dict[str, Any]:
    states = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    opt = optimizer.state_dict() if optimizer is not None else None
    if opt is not None:
        opt = {"state": {i: {k: (v.detach().cpu() if torch.is_tensor(v) else v) for k, v in st.items()}
                         for i, st in opt["state"].items()},
               "param_groups": opt["param_groups"]}
    ckpt = {"epoch": epoch, "model": task, "state_dict": states, "perf": best_perf, "optimizer": opt}
    if getattr(optimizer, "ema_enabled", False):
        ema = optimizer.ema_state_dict()
        ckpt["ema"] = {**ema, "shadow": {k: v.detach().cpu() for k, v in ema["shadow"].items()}}
    lora = model.lora_config() if hasattr(model, "lora_config") else None
    if lora is not None:
        ckpt["lora"] = lora
    return ckpt


def save_model_on_master(model, ckpt_dir: str, task: str, epoch: int, best_perf: float, optimizer=None) -> Optional[str]:
    """engine.py:202-218: rank 0 writes ``<ckpt_dir>/<task>_<epoch>.pth``; other ranks return None."""
    if D.rank() != 0:
        return None
    path = os.path.join(ckpt_dir, "%s_%s.pth" % (task, epoch))
    logging.info("=> saving checkpoint to {}".format(ckpt_dir))
    try:
        torch.save(checkpoint_dict(model, optimizer, task, epoch, best_perf), path)
    except Exception:
        logging.error("=> error when saving checkpoint!")
        return None
    return path


def load_checkpoint(path: str, device=None, is_train: bool = True) -> Tuple[Any, Optional[dict], int, float]:
    """train.py:101-124: returns ``(model, optimizer_state, begin_epoch, best_perf)``.  ``path`` holds either the
    reference's checkpoint dictionary or a bare CLIP state dict (then optimizer_state is None, epoch 0, perf 0)."""
    if not os.path.exists(path):
        raise FileNotFoundError("=> error when loading checkpoint (cannot find checkpoint): {}".format(path))
    blob = torch.load(path, map_location="cpu", weights_only=True)
    if isinstance(blob, dict) and "state_dict" in blob:
        state_dict = blob["state_dict"]
        opt_state = blob.get("optimizer")
        begin_epoch = blob.get("epoch" if is_train else "step", 0)
        best_perf = blob.get("perf", 0.0)
    else:
        state_dict, opt_state, begin_epoch, best_perf = blob, None, 0, 0.0
    # low-rank adapters: the base model from the other keys, enable_lora(**config), then the adapters (model.build_model)
    model = build_model(dict(state_dict), lora=blob.get("lora") if isinstance(blob, dict) else None)
    if device is not None:
        model = model.to(device)
    return model, opt_state, begin_epoch, best_perf


def load_ema(path: str) -> Optional[dict]:
    """The ``'ema'`` entry of a checkpoint (``optimizer.load_ema_state_dict`` takes it), or None when the file has none."""
    if not os.path.exists(path):
        raise FileNotFoundError("=> error when loading checkpoint (cannot find checkpoint): {}".format(path))
    blob = torch.load(path, map_location="cpu", weights_only=True)
    return blob.get("ema") if isinstance(blob, dict) else None
