"""The optimiser side of the step: fused clip_grad_norm_(.,1) + Adam, or + SGD with momentum, or + Lion, over the
model's flat buffers (reference engine.py:87-95, build_optimizer engine.py:129-151) -- two HIP launches per step, no host
synchronisation -- and the learning-rate schedules of utils.py:310-416 / build_lr_scheduler engine.py:154-176
(host arithmetic: one float per step)."""
from __future__ import annotations

import contextlib
import math
import os
from bisect import bisect_right
import ctypes
from ctypes import c_float, c_int
from typing import List, Sequence

import torch

from ._lib import check, lib, ptr, stream

MAX_GROUPS = 8


class OptimGroup(ctypes.Structure):
    """``ce_optim_group`` of include/clip_event_hip.h."""
    _fields_ = [("lr", c_float), ("weight_decay", c_float), ("decoupled", c_int), ("pad_", c_int)]


def ema_rate(decay: float, warmup: bool, updates: int) -> float:
    """The weight of the new masters in the ``updates + 1``-th update of the weight average: ``1 - decay``, or with ``warmup``
    ``1 - min(decay, (1 + updates) / (10 + updates))`` (the TF / timm rule: 0.9, 9/11, ... until the cap, so that a young
    average is not dominated by its start).  Python floats; the kernels take it rounded once to fp32."""
    d = float(decay)
    if warmup:
        d = min(d, (1.0 + updates) / (10.0 + updates))
    return 1.0 - d


class _FusedFlatOptimizer(torch.optim.Optimizer):
    """What the fused optimisers share: one param group over the model's flat buffers, the gradient zero-fill, the device
    scalar of the gradient norm, the whole of ``step()`` and the frames of ``state_dict()`` / ``load_state_dict()``.

    A model that can describe its trainable ranges (``trainable_plan``, model.CLIP) may have frozen parameters and parameter
    ``groups`` (a list of dicts: ``"params"`` = parameter names or Parameters, plus ``lr`` / ``weight_decay`` / -- Adam --
    ``decoupled``; at most 8; what is named nowhere forms the first group with the constructor's values).  ``step()`` then takes
    the grouped path: the gradient norm over the plan's chunk table, the update over its tile and segment tables with each
    group's scalars; a frozen range is in no table.  With nothing frozen, one group and no decoupled decay it is the plain path,
    launch for launch what it was before groups existed.  Every group is an entry of ``param_groups`` that holds the group's
    TRAINABLE parameters; a parameter frozen or unfrozen between steps leaves or joins its group at the next ``step()`` (an
    unfrozen one starts with zero moments, under the one shared step count).

    A subclass names its rule (``_rule``: the entry points are ``ce_<rule>_step(p, g, *state, p16, n, *args, stream)`` on a range of the
    flat buffers, ``ce_<rule>_step_tiles(p, g, *state, p16, jobs, njobs, tiles, segments, nsegments, *args, stream)`` and
    ``ce_<rule>_step_groups``: the same with ``segment_group`` behind ``nsegments`` and ``groups, ngroups`` in place of lr / weight
    decay), its flat state buffers (``_STATE``: attribute names, in the kernels' order; ``_state()`` allocates them and ``sumsq``) and
    its torch counterpart (``_stock``), and provides ``_rule_args(sumsq, grouped)`` (the rule's arguments behind the form's, without
    clip and lr / weight decay in the grouped form), ``_after_step(sharded)`` (what to note once the step is launched) and, where a
    fresh state buffer means something, ``_new_state()``.

    Weight EMA (``enable_ema``; off by default, and then every launch is what it is without it): one more flat fp32 buffer,
    ``ema <- ema + rate (p - ema)`` with ``rate = ema_rate(decay, warmup, ema_updates)``, carried by the SAME kernels as the
    update (the ``_ema`` twin of whichever entry point the step takes) from the fp32 masters as the update wrote them.  It is
    not one of ``state_buffers()``: the average of a frozen parameter is the parameter, and stays that when the parameter
    wakes (a woken parameter's moments restart from zero, its average does not).  The average belongs to the model's flat
    buffer: if that buffer is re-created (the model moved to another device, a new layout), the average starts again from the
    new masters and ``ema_updates`` from 0.  ``averaged()`` swaps the average into the model for evaluation or a checkpoint
    and swaps the training weights back on exit."""

    _GROUP_KEYS = ("lr", "weight_decay")       # what a group may set for itself; everything else is shared
    _STATE = ()                                # the flat fp32 state buffers: attribute names, in the order the kernels take them

    def __init__(self, model, max_norm, defaults, groups=None):
        name = type(self).__name__
        named = list(model.named_parameters())
        frozen = [n for n, p in named if not p.requires_grad]
        if (frozen or groups) and not hasattr(model, "trainable_plan"):
            what = f"frozen parameters ({frozen[:3]}...)" if frozen else "parameter groups"
            raise NotImplementedError(f"{name} updates the whole flat parameter buffer; {what} need a model that describes its "
                                      f"trainable ranges (trainable_plan), or {self._stock} over the trainable ones instead")
        if (frozen or groups) and getattr(getattr(model, "grad_sync", None), "plan", None) is not None:
            raise NotImplementedError(f"{name}: the sharded optimiser step (CE_SHARDED_ADAM) does not take frozen parameters or "
                                      "parameter groups")
        self.model = model
        self.max_norm = max_norm
        self.step_count = 0                # steps taken by THIS object (Adam's bias correction; the telemetry cadence)
        self.sat_poll_every = int(os.environ.get("CE_SAT_POLL_EVERY", "16"))     # 0 = never
        self.sumsq = None
        self.ema = None                    # the weight average (flat fp32, the layout of model._flat), or None: EMA off
        self.ema_decay, self.ema_warmup, self.ema_updates = None, False, 0
        self._ema_of = None                # the flat master buffer the average was started from
        self._averaging = False            # inside averaged(): the average sits in model._flat, the masters in self.ema
        # group specs: (own hyper-parameters, names); names None = whatever no group lists, with the constructor's values
        by_id, known = {id(p): n for n, p in named}, {n for n, _ in named}
        if len(groups or ()) > MAX_GROUPS:
            raise ValueError(f"{name}: at most {MAX_GROUPS} parameter groups (got {len(groups)})")
        specs, owner = [], {}
        for gi, g in enumerate(groups or ()):
            if not isinstance(g, dict) or "params" not in g:
                raise ValueError(f"{name}: group {gi} must be a dict with a 'params' list")
            extra = sorted(set(g) - {"params"} - set(self._GROUP_KEYS))
            if extra:
                raise ValueError(f"{name}: group {gi} sets {extra}; a group may set {sorted(self._GROUP_KEYS)} only "
                                 "(everything else is shared by all groups)")
            for q in g["params"]:
                n = q if isinstance(q, str) else by_id.get(id(q))
                if n not in known:
                    raise ValueError(f"{name}: group {gi} names {q if isinstance(q, str) else 'a tensor'!r}, which is no parameter of the model")
                if n in owner:
                    raise ValueError(f"{name}: parameter {n} is in groups {owner[n]} and {gi}")
                if n in frozen:
                    raise ValueError(f"{name}: group {gi} names the frozen parameter {n}; unfreeze it first")
                owner[n] = gi
            specs.append((self._group_hyper(g), {n for n, at in owner.items() if at == gi}))
        if not specs or any(p.requires_grad and n not in owner for n, p in named):
            specs.insert(0, ({}, None))
        if len(specs) > MAX_GROUPS:
            raise ValueError(f"{name}: at most {MAX_GROUPS} parameter groups (got {len(specs)} with the unnamed parameters' group)")
        self._specs = specs
        self._flags_seen = tuple(p.requires_grad for _, p in named)
        if groups or frozen:
            params = [{"params": [p for n, p in named if p.requires_grad and (n in names if names is not None else n not in owner)],
                       **hyper} for hyper, names in specs]
        else:
            params = [p for _, p in named]
        super().__init__(params, defaults)

    def _group_hyper(self, g):
        """The param-group entries a user group sets for itself."""
        return {k: g[k] for k in ("lr", "weight_decay") if k in g}

    # ---- groups and frozen parameters ----
    def _follow_flags(self):
        """Make ``param_groups`` hold the trainable parameters of every group again after a ``requires_grad`` flag changed
        (cheap when none did).  A parameter that became trainable and is named in no group joins the unnamed parameters' group,
        which is appended behind the others if there was none; its state starts from zero."""
        m = self.model
        if not hasattr(m, "_flags"):
            return
        flags = m._flags()
        if flags == self._flags_seen:
            return
        named = list(m.named_parameters())
        owner = {n: gi for gi, (_, names) in enumerate(self._specs) for n in names or ()}
        woken = [n for (n, p), was in zip(named, self._flags_seen) if p.requires_grad and not was]
        if all(names is not None for _, names in self._specs) and any(p.requires_grad and n not in owner for n, p in named):
            if len(self._specs) >= MAX_GROUPS:
                raise ValueError(f"{type(self).__name__}: a parameter unfrozen outside every group needs the unnamed parameters' "
                                 f"group, and there are {MAX_GROUPS} groups already")
            self._specs.append(({}, None))
            self.add_param_group({"params": [p for n, p in named if p.requires_grad and n not in owner]})
        for g, (_, names) in zip(self.param_groups, self._specs):
            g["params"] = [p for n, p in named if p.requires_grad and (n in names if names is not None else n not in owner)]
        self._flags_seen = flags
        if woken and self.step_count > 0 and getattr(m, "_flat", None) is not None:
            for buf in self.state_buffers():
                for n in woken:
                    o = m._offsets[n]
                    buf[o:o + (m._pmap[n].numel() + 63) // 64 * 64].zero_()

    def _group_of(self):
        """name -> index of its group, for every trainable parameter."""
        owner = {n: gi for gi, (_, names) in enumerate(self._specs) for n in names or ()}
        default = next((gi for gi, (_, names) in enumerate(self._specs) if names is None), None)
        return {n: owner.get(n, default) for n, p in self.model.named_parameters() if p.requires_grad}

    def _plain(self) -> bool:
        """Nothing frozen (as of the last ``_follow_flags``), one group, no decoupled decay: the launches of the step before groups
        existed."""
        return len(self.param_groups) == 1 and not self.param_groups[0].get("decoupled_weight_decay") and all(self._flags_seen)

    def _grouped_step(self, sumsq, s):
        m = self.model
        if getattr(getattr(m, "grad_sync", None), "plan", None) is not None:
            raise NotImplementedError(f"{type(self).__name__}: the sharded optimiser step (CE_SHARDED_ADAM) does not take frozen "
                                      "parameters or parameter groups")
        group_of = self._group_of()
        if not group_of:
            raise RuntimeError(f"{type(self).__name__}.step: every parameter is frozen")
        tiles = bool(getattr(m, "_adam_tiles_ok", False)) and os.environ.get("CE_ADAM_TILES", "1") != "0"
        plan = m.trainable_plan(group_of, tiles=tiles)
        garr = (OptimGroup * len(self.param_groups))()
        for i, g in enumerate(self.param_groups):
            garr[i].lr, garr[i].weight_decay, garr[i].decoupled = float(g["lr"]), float(g["weight_decay"]), int(bool(g.get("decoupled_weight_decay")))
        if sumsq is not None:
            sumsq.zero_()
            check(lib().ce_sumsq_segments(ptr(m._flat_grad), ptr(plan.chunks), plan.chunks.shape[0], ptr(sumsq), s),
                  "ce_sumsq_segments")
        tj, tn_, tt = plan.tjobs
        self._launch("groups", (ptr(tj), tn_, tt, ptr(plan.segments), plan.segments.shape[0], ptr(plan.segment_group), ptr(sumsq),
                                self.max_norm or 0.0, garr, len(garr)), self._rule_args(sumsq, True), s)
        # a frozen range was not touched: its mirror and W^T copy were current before the step and its master did not move
        m.mark_operands_stale(mirror_fresh=True, wt_fresh=tiles)

    # ---- weight EMA ----
    @property
    def ema_enabled(self) -> bool:
        return self.ema_decay is not None

    def _refuse_while_averaged(self, what):
        if self._averaging:
            raise RuntimeError(f"{type(self).__name__}.{what} inside averaged(): the model holds the averaged weights; leave the "
                               "context first")

    def enable_ema(self, decay: float = 0.9999, warmup: bool = False):
        """Start a weight average at the current weights: one flat fp32 buffer, a copy of the model's flat master buffer
        (alignment padding included), updated by every ``step()`` from here on; ``ema_updates`` = 0.  ``warmup``: see
        ``ema_rate``.  Enabling again starts again."""
        self._refuse_while_averaged("enable_ema")
        decay = float(decay)
        if not 0.0 <= decay < 1.0:
            raise ValueError(f"{type(self).__name__}.enable_ema: decay must lie in [0, 1) (got {decay})")
        self.ema_decay, self.ema_warmup = decay, bool(warmup)
        self.ema = self._ema_of = None
        self._state()
        self._ema_ready()

    def disable_ema(self):
        """Stop averaging and free the buffer."""
        self._refuse_while_averaged("disable_ema")
        self.ema = self._ema_of = None
        self.ema_decay, self.ema_warmup, self.ema_updates = None, False, 0

    def _ema_ready(self):
        """(Re-)start the average from the masters when there is none for the model's present flat buffer (after ``_state()``)."""
        flat = self.model._flat
        if self.ema_enabled and (self.ema is None or self._ema_of is not flat):
            self.ema = flat.detach().clone()
            self._ema_of = flat
            self.ema_updates = 0

    def _swap_average(self):
        m = self.model
        m.wait_transposes()           # an asynchronous W^T rebuild may still be reading the mirror the swap rewrites
        check(lib().ce_swap_cast_bf16(ptr(m._flat), ptr(self.ema), ptr(m._flat16), m._flat.numel(), stream()), "ce_swap_cast_bf16")
        # the mirror is that of the new content; the W^T copies (and the fp8 operands) are rebuilt from it by the next _ready()
        m.mark_operands_stale(mirror_fresh=True, wt_fresh=False)

    @contextlib.contextmanager
    def averaged(self):
        """Inside, the model holds the averaged weights (``encode_*``, ``inference.*``, ``model.state_dict()``, a checkpoint
        written here) and this object holds the training weights: one pass exchanges the two flat buffers and writes the bf16
        mirror.  On exit -- also when the body raises -- the same pass puts everything back, bit for bit.  ``step()``,
        ``enable_ema`` and ``disable_ema`` raise inside; not re-entrant."""
        if not self.ema_enabled:
            raise RuntimeError(f"{type(self).__name__}.averaged: enable_ema() first")
        self._refuse_while_averaged("averaged")
        self._state()
        self._ema_ready()
        self._swap_average()
        self._averaging = True
        try:
            yield self.model
        finally:
            self._averaging = False
            self._swap_average()

    def _named_offsets(self):
        m = self.model
        return [(n, p, m._offsets[n]) for n, p in m.named_parameters()]

    def ema_state_dict(self):
        """``{"decay", "warmup", "updates", "shadow": {parameter name: the average, in the parameter's shape}}`` (copies; every
        parameter, frozen ones too)."""
        if not self.ema_enabled:
            raise RuntimeError(f"{type(self).__name__}.ema_state_dict: EMA is off")
        if not self._averaging:
            self._state()
            self._ema_ready()
        src = self.model._flat if self._averaging else self.ema
        shadow = {n: src[o:o + p.numel()].view(p.shape).clone() for n, p, o in self._named_offsets()}
        return {"decay": self.ema_decay, "warmup": self.ema_warmup, "updates": self.ema_updates, "shadow": shadow}

    def load_ema_state_dict(self, sd):
        """Take the average, its decay / warm-up and its update count from ``ema_state_dict()``'s format (enables EMA if it is
        off); names and shapes must be the model's."""
        self._refuse_while_averaged("load_ema_state_dict")
        shadow = sd["shadow"]
        named = {n: p for n, p in self.model.named_parameters()}
        missing, extra = sorted(set(named) - set(shadow)), sorted(set(shadow) - set(named))
        if missing or extra:
            raise ValueError(f"EMA state does not match the model: missing {missing[:3]}, unexpected {extra[:3]}")
        for n, p in named.items():
            if tuple(shadow[n].shape) != tuple(p.shape):
                raise ValueError(f"EMA state does not match the model: {n} is {tuple(shadow[n].shape)}, expected {tuple(p.shape)}")
        self.enable_ema(sd["decay"], sd.get("warmup", False))
        with torch.no_grad():
            for n, p, o in self._named_offsets():
                self.ema[o:o + p.numel()].view(p.shape).copy_(shadow[n])
        self.ema_updates = int(sd.get("updates", 0))

    # kept as attributes of the first (only) group so that schedulers and user code see one source of truth
    @property
    def lr(self):
        return self.param_groups[0]["lr"]

    @property
    def weight_decay(self):
        return self.param_groups[0]["weight_decay"]

    def zero_grad(self, set_to_none: bool = False):
        self._state()
        self.model._flat_grad.zero_()
        self.model._attach_grads_fast()

    def zero_grad_first_touch(self):
        """``zero_grad`` for a caller that owns the whole step (engine.train_step): the block weight gradients are left
        to be overwritten by the step's first backward pass (model.zero_grad_first_touch)."""
        self._state()
        self.model.zero_grad_first_touch()

    def grad_norm(self) -> torch.Tensor:
        """Device scalar: total L2 norm of the gradients as of the last ``step``."""
        return self.sumsq.sqrt()

    @torch.no_grad()
    def step(self, closure=None):
        """clip + update (engine.py:87-95): sum of squares of the whole gradient buffer, then the update with the clip coefficient
        applied on the fly -- by default in tiles that also leave the blocks' W^T operand copies behind (``_tiles_op``).  With
        frozen parameters, several groups or decoupled decay: the same over the tables of ``model.trainable_plan`` (``_grouped_step``)."""
        if closure is not None:
            raise RuntimeError(f"{type(self).__name__}.step takes no closure")
        self._refuse_while_averaged("step")
        self._state()
        self._ema_ready()
        m = self.model
        self._follow_flags()            # a parameter frozen or unfrozen since the last step
        m._settle_first_touch()         # a tower that saw no backward since zero_grad_first_touch
        if hasattr(m, "finish_lora_grads"):
            m.finish_lora_grads()       # adapters: their gradients from the weight gradients of the frozen matrices (no-op without)
        m.wait_transposes()            # the update rewrites the bf16 mirror an asynchronous W^T rebuild may still be reading
        n = m._flat.numel()
        s = stream()
        self.step_count += 1
        from . import distributed as D
        plan = getattr(getattr(m, "grad_sync", None), "plan", None)
        sharded = plan is not None and D.active()
        if sharded and self.ema_enabled:
            raise NotImplementedError(f"{type(self).__name__}: the sharded optimiser step (CE_SHARDED_ADAM) does not carry the weight "
                                      "EMA; use the replicated step (every rank then computes the same average)")
        sumsq = self.sumsq if self.max_norm is not None else None
        if not self._plain():
            self._grouped_step(sumsq, s)
        else:
            args = self._rule_args(sumsq, False)

            def sum_squares(lo, hi):
                check(lib().ce_sumsq(ptr(m._flat_grad[lo:hi]), hi - lo, ptr(self.sumsq), s), "ce_sumsq")

            def update(lo, hi):
                self._launch("", (hi - lo,), args, s, lo, hi)

            if sharded:
                # sharded step (distributed.ShardPlan; DESIGN 5 lever 2): the gradient pieces arrived reduce-SCATTERED, this rank updates
                # its shard of every piece (+ the replicated head range), the fp32 masters are completed by an all-gather in place and
                # the bf16 operand mirror is re-cast from them by the next refresh_operands; the optimiser state stays sharded
                D.sharded_update(plan, m._flat, sumsq, sum_squares, update)
                m.mark_operands_stale(mirror_fresh=False)
            else:
                if sumsq is not None:
                    sumsq.zero_()
                    sum_squares(0, n)
                if getattr(m, "_adam_tiles_ok", False) and os.environ.get("CE_ADAM_TILES", "1") != "0":
                    # the block weights tile by tile, which also writes their W^T operand copies (no transpose pass at the start of the
                    # next step); everything else by the chunk table of the first-touch zero-fill (= the complement of the block weights)
                    tj, tn_, tt = m._tjobs_bwd
                    seg = m._adam_segment_table()
                    self._launch("tiles", (ptr(tj), tn_, tt, ptr(seg), seg.shape[0]), args, s)
                    m.mark_operands_stale(mirror_fresh=True, wt_fresh=True)
                else:
                    update(0, n)
                    m.mark_operands_stale(mirror_fresh=True)
        # every path ends here, the grouped and the sharded one included
        self._after_step(sharded)
        self.ema_updates += int(self.ema_enabled)
        # fp16 streams: look at the clamp counters every few steps, without a synchronisation (the copy started by one poll is
        # examined by the next); raises model.Stream16Saturation
        if self.sat_poll_every and self.step_count % self.sat_poll_every == 0 and hasattr(m, "poll_stream16_saturation"):
            m.poll_stream16_saturation()

    def _launch(self, form, operands, args, s, lo=None, hi=None):
        """One update launch: ``ce_<rule>_step`` (``form`` ""; on ``[lo, hi)`` of the flat buffers), ``..._tiles`` or ``..._groups``
        (on the whole buffers), its ``_ema`` twin while the average is on -- the one place where an entry point gets its name.
        ``operands``: the form's between ``p_bf16`` and the rule's ``args``."""
        m = self.model
        name = f"ce_{self._rule}_step" + (form and "_" + form) + ("_ema" if self.ema_enabled else "")
        state = (getattr(self, b) if b in self._state_names() else None for b in self._STATE)      # (None: SGD without momentum)

        def at(b):
            return ptr(b if b is None or lo is None else b[lo:hi])

        ema = (at(self.ema), ema_rate(self.ema_decay, self.ema_warmup, self.ema_updates)) if self.ema_enabled else ()
        check(getattr(lib(), name)(at(m._flat), at(m._flat_grad), *map(at, state), at(m._flat16), *operands, *args, *ema, s), name)

    # ---- the flat state buffers ----
    def _state_names(self):
        """The buffers of ``_STATE`` this optimiser keeps (SGD: none at momentum 0; the kernels then get NULL)."""
        return self._STATE

    def _state(self):
        """Make ``sumsq`` and the flat state buffers exist for the model's present flat buffer (its size, its device); a buffer
        that had to be created starts at zero, and the subclass is told (``_new_state``)."""
        m = self.model
        m._ready()
        flat = m._flat
        if self.sumsq is None or self.sumsq.device != flat.device:
            self.sumsq = torch.zeros(1, dtype=torch.float32, device=flat.device)
        for name in self._state_names():
            buf = getattr(self, name)
            if buf is None or buf.numel() != flat.numel() or buf.device != flat.device:
                setattr(self, name, torch.zeros_like(flat))
                self._new_state()

    def _new_state(self):
        pass

    def state_buffers(self):
        """The flat optimiser state tensors (what ``distributed.consolidate`` gathers after sharded steps): Adam ``(m, v)``, SGD
        ``(buf,)`` or ``()`` without momentum, Lion ``(exp_avg,)``."""
        self._state()
        return tuple(getattr(self, name) for name in self._state_names())

    def _params(self):
        """Every parameter of every group, in group order: torch's state indices run consecutively over them."""
        self._follow_flags()
        return [p for g in self.param_groups for p in g["params"]]

    def _offset_of(self):
        """Flat offset of every parameter of the groups, in group order."""
        names = {id(p): n for n, p in self.model.named_parameters()}
        return [self.model._offsets[names[id(p)]] for p in self._params()]

    def _pieces(self, buf):
        """The piece of the flat buffer ``buf`` that belongs to each parameter of the groups, in group order, in its shape."""
        return [buf[o:o + p.numel()].view(p.shape) for p, o in zip(self._params(), self._offset_of())]

    # ---- torch-format state (checkpoint interop): the frames; a subclass fills in the per-parameter state ----
    def _state_dict_of(self, state):
        self._params()
        groups, at = [], 0
        for g in self.param_groups:
            group = {k: v for k, v in g.items() if k != "params"}
            group["params"] = list(range(at, at + len(g["params"])))
            at += len(g["params"])
            groups.append(group)
        return {"state": state, "param_groups": groups}

    def _refuse_sharded_state(self, what):
        if getattr(self, "_moments_stale", False):
            raise RuntimeError(f"the {what} sharded over the ranks (sharded optimiser step): call "
                               "clip_event_amd.distributed.consolidate(model, optimizer) on EVERY rank before state_dict()")

    def _matching_group(self, sd):
        """The param groups of ``sd`` (the one group itself when there is one), after checking that they are ours."""
        self._params()
        groups = sd["param_groups"]
        if len(self.param_groups) == 1:
            params = self.param_groups[0]["params"]
            if len(groups) != 1 or len(groups[0]["params"]) != len(params):
                raise ValueError("optimizer state does not match: expected one group of %d parameters" % len(params))
            return groups[0]
        if len(groups) != len(self.param_groups) or any(len(a["params"]) != len(b["params"]) for a, b in zip(groups, self.param_groups)):
            raise ValueError("optimizer state does not match: expected %d groups of %s parameters"
                             % (len(self.param_groups), [len(g["params"]) for g in self.param_groups]))
        def norm(v):
            return tuple(v) if isinstance(v, (list, tuple)) else v

        for k in groups[0]:
            if k not in ("params", "lr", "weight_decay", "decoupled_weight_decay", "initial_lr") and \
                    any(norm(g.get(k)) != norm(groups[0][k]) for g in groups):
                raise ValueError(f"optimizer state sets {k!r} per group; the fused step shares it")
        return groups

    def _adopt_group(self, group):
        for mine, theirs in zip(self.param_groups, group if isinstance(group, list) else [group]):
            for k, v in theirs.items():
                if k != "params":
                    mine[k] = tuple(v) if k == "betas" else v


class FusedAdam(_FusedFlatOptimizer):
    """``torch.optim.Adam(params, lr, weight_decay)`` semantics (L2 decay added to the gradient)
    preceded by the global-norm clip of ``clip_grad_norm_(params, max_norm)``.  ``max_norm=None``
    disables clipping.

    A real ``torch.optim.Optimizer`` (one param group over ``model.parameters()``), so the stock and the
    reference's LR schedulers drive it through ``param_groups[0]['lr']``, and ``state_dict()`` /
    ``load_state_dict()`` speak ``torch.optim.Adam``'s format (per-parameter ``step`` / ``exp_avg`` /
    ``exp_avg_sq``): the ``'optimizer'`` entry of a reference checkpoint (engine.py:202-218) loads here and vice
    versa.  The moments themselves live in two flat buffers next to the flat parameters."""

    _rule, _STATE, _stock = "adam", ("m", "v"), "torch.optim.Adam"
    _GROUP_KEYS = ("lr", "weight_decay", "decoupled")

    def __init__(self, model, lr: float = 1e-6, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0,
                 max_norm=1.0, decoupled: bool = False, groups=None):
        self.m = self.v = None
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay)
        if decoupled or any(isinstance(g, dict) and "decoupled" in g for g in groups or ()):
            # AdamW (``torch.optim.AdamW``): p *= 1 - lr * weight_decay, no decay term in the gradient.  The group key is torch's,
            # so that a state_dict loaded into torch.optim.AdamW keeps the decoupled form.
            defaults["decoupled_weight_decay"] = bool(decoupled)
        super().__init__(model, max_norm, defaults, groups)

    def _group_hyper(self, g):
        hyper = super()._group_hyper(g)
        if "decoupled" in g:
            hyper["decoupled_weight_decay"] = bool(g["decoupled"])
        return hyper

    @property
    def betas(self):
        return self.param_groups[0]["betas"]

    @property
    def eps(self):
        return self.param_groups[0]["eps"]

    def _rule_args(self, sumsq, grouped):
        if grouped:
            return (self.betas[0], self.betas[1], self.eps, self.step_count)
        return (ptr(sumsq), self.max_norm or 0.0, float(self.lr), self.betas[0], self.betas[1], self.eps, self.weight_decay, self.step_count)

    def _after_step(self, sharded):
        if sharded:
            self._moments_stale = True

    def state_dict(self):
        self._state()
        self._refuse_sharded_state("Adam moments are")
        state = {}
        if self.step_count > 0:
            for i, (m, v) in enumerate(zip(self._pieces(self.m), self._pieces(self.v))):
                state[i] = {"step": torch.tensor(float(self.step_count)), "exp_avg": m.clone(), "exp_avg_sq": v.clone()}
        return self._state_dict_of(state)

    def load_state_dict(self, sd):
        self._moments_stale = False          # (every rank loads the same tensors)
        self._state()
        self._adopt_group(self._matching_group(sd))
        self.m.zero_()
        self.v.zero_()
        m, v = self._pieces(self.m), self._pieces(self.v)
        steps = set()
        with torch.no_grad():
            for key, st in sd["state"].items():
                m[int(key)].copy_(st["exp_avg"].reshape(m[int(key)].shape))
                v[int(key)].copy_(st["exp_avg_sq"].reshape(v[int(key)].shape))
                steps.add(int(st["step"]))
        if len(steps) > 1:
            raise ValueError("per-parameter step counts differ; the fused kernel keeps one")
        self.step_count = steps.pop() if steps else 0


class FusedSGD(_FusedFlatOptimizer):
    """``torch.optim.SGD(params, lr, momentum, dampening, weight_decay, nesterov)`` semantics preceded by the global-norm clip
    of ``clip_grad_norm_(params, max_norm)`` (engine.py:89-90 with engine.py:136-140's optimiser).  ``max_norm=None`` disables
    clipping.

    A real ``torch.optim.Optimizer`` like ``FusedAdam``: one param group that carries torch SGD's keys, ``state_dict()`` /
    ``load_state_dict()`` in ``torch.optim.SGD``'s format (per-parameter ``momentum_buffer``; empty before the first step and
    with momentum 0).  The momentum lives in ONE flat buffer next to the flat parameters -- none at all with momentum 0 -- and,
    as in torch, "first step" means "no buffer yet", not a counter (the arithmetic never reads ``step_count``): the first step
    copies the decayed gradient into it whatever the dampening is."""

    _rule, _STATE, _stock = "sgd", ("buf",), "torch.optim.SGD"

    def __init__(self, model, lr: float = 1e-3, momentum: float = 0.0, dampening: float = 0.0, weight_decay: float = 0.0,
                 nesterov: bool = False, max_norm=1.0, groups=None):
        if lr < 0.0:
            raise ValueError(f"Invalid learning rate: {lr}")
        if momentum < 0.0:
            raise ValueError(f"Invalid momentum value: {momentum}")
        if weight_decay < 0.0:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        self.buf = None
        self._has_buf = False              # a momentum buffer exists: the next step is not the first
        super().__init__(model, max_norm, dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay,
                                               nesterov=nesterov, maximize=False, foreach=None, differentiable=False, fused=None),
                         groups)

    @property
    def momentum(self):
        return self.param_groups[0]["momentum"]

    def _state_names(self):
        return self._STATE if self.momentum != 0 else ()       # no buffer at momentum 0

    def _new_state(self):
        self._has_buf = False

    def _rule_args(self, sumsq, grouped):
        group = self.param_groups[0]
        if any(g.get("maximize") for g in self.param_groups):
            raise NotImplementedError("FusedSGD: maximize is not supported")
        lr, mu, damp, wd = (float(group[k]) for k in ("lr", "momentum", "dampening", "weight_decay"))
        flags = (int(bool(group["nesterov"])), int(not self._has_buf))
        return (mu, damp, *flags) if grouped else (ptr(sumsq), self.max_norm or 0.0, lr, mu, damp, wd, *flags)

    def _after_step(self, sharded):
        if sharded:
            self._moments_stale = self.momentum != 0       # the momentum stays sharded
        self._has_buf = self.momentum != 0

    def state_dict(self):
        self._state()
        self._refuse_sharded_state("momentum buffer is")
        state = {}
        if self._has_buf and self.momentum != 0:
            state = {i: {"momentum_buffer": b.clone()} for i, b in enumerate(self._pieces(self.buf))}
        return self._state_dict_of(state)

    def load_state_dict(self, sd):
        self._moments_stale = False          # (every rank loads the same tensors)
        group = self._matching_group(sd)
        params = self._params()
        bufs = {int(k): st["momentum_buffer"] for k, st in sd["state"].items() if st.get("momentum_buffer") is not None}
        if bufs and len(bufs) != len(params):
            raise ValueError("only %d of %d parameters carry a momentum_buffer; the fused kernel keeps one buffer and one "
                             "first-step flag for all of them" % (len(bufs), len(params)))
        self._adopt_group(group)
        self._state()
        self._has_buf = False
        if bufs and self.momentum != 0:
            with torch.no_grad():
                self.buf.zero_()
                for i, b in enumerate(self._pieces(self.buf)):
                    b.copy_(bufs[i].reshape(b.shape))
            self._has_buf = True


class FusedLion(_FusedFlatOptimizer):
    """Lion (Chen et al. 2023, "Symbolic Discovery of Optimization Algorithms") preceded by the global-norm clip of
    ``clip_grad_norm_(params, max_norm)``: ``c = b1 m + (1 - b1) g``, ``p <- p (1 - lr weight_decay) - lr sign(c)``, then
    ``m <- b2 m + (1 - b2) g`` (include/clip_event_hip.h, ``ce_lion_step``, has the arithmetic rounding by rounding).  The weight
    decay is always decoupled -- the update has magnitude ``lr`` whatever the gradient is, so a decay folded into the gradient
    would only vote on the sign -- and there is no bias correction and no step counter: zero momentum is the initial state.
    ``max_norm=None`` disables clipping.  The usual learning rate is a tenth to a third of Adam's, with the weight decay
    raised by the same factor.

    A real ``torch.optim.Optimizer`` like ``FusedAdam`` / ``FusedSGD``, with everything ``_FusedFlatOptimizer`` provides (tiles,
    frozen ranges and parameter groups, weight EMA, first-touch zero-fill, the sharded step).  The momentum lives in ONE flat
    buffer next to the flat parameters -- the streams and bytes of SGD with momentum.  ``state_dict()`` / ``load_state_dict()`` speak the
    layout of the common Lion implementations (timm, lion-pytorch): per-parameter ``{"exp_avg": tensor}``, group keys ``lr`` /
    ``betas`` / ``weight_decay``, an empty state before the first step."""

    _rule, _STATE, _stock = "lion", ("exp_avg",), "a stock Lion (timm.optim.Lion, lion_pytorch.Lion)"

    def __init__(self, model, lr: float = 1e-4, betas=(0.9, 0.99), weight_decay: float = 0.0, max_norm=1.0, groups=None):
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        betas = tuple(betas)
        if len(betas) != 2:
            raise ValueError(f"Invalid betas: {betas} (need two)")
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 0: {betas[0]}")
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 1: {betas[1]}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        for gi, g in enumerate(groups or ()):
            if isinstance(g, dict) and (g.get("lr", 0.0) < 0.0 or g.get("weight_decay", 0.0) < 0.0):
                raise ValueError(f"Invalid learning rate or weight_decay value in group {gi}")
        self.exp_avg = None
        self._has_state = False            # a step was taken or a momentum loaded: state_dict() has something to say
        super().__init__(model, max_norm, dict(lr=lr, betas=betas, weight_decay=weight_decay), groups)

    @property
    def betas(self):
        return self.param_groups[0]["betas"]

    def _new_state(self):
        self._has_state = False

    def _rule_args(self, sumsq, grouped):
        b1, b2 = float(self.betas[0]), float(self.betas[1])
        return (b1, b2) if grouped else (ptr(sumsq), self.max_norm or 0.0, float(self.lr), b1, b2, float(self.weight_decay))

    def _after_step(self, sharded):
        if sharded:
            self._moments_stale = True     # the momentum stays sharded
        self._has_state = True

    def state_dict(self):
        self._state()
        self._refuse_sharded_state("Lion momentum is")
        state = {}
        if self._has_state:
            state = {i: {"exp_avg": b.clone()} for i, b in enumerate(self._pieces(self.exp_avg))}
        return self._state_dict_of(state)

    def load_state_dict(self, sd):
        self._moments_stale = False          # (every rank loads the same tensors)
        group = self._matching_group(sd)
        params = self._params()
        bufs = {int(k): st["exp_avg"] for k, st in sd["state"].items() if st.get("exp_avg") is not None}
        if bufs and len(bufs) != len(params):
            raise ValueError("only %d of %d parameters carry an exp_avg; the fused kernel keeps one flat momentum for all of them"
                             % (len(bufs), len(params)))
        self._adopt_group(group)
        self._state()
        self.exp_avg.zero_()
        self._has_state = False
        if bufs:
            with torch.no_grad():
                for i, b in enumerate(self._pieces(self.exp_avg)):
                    b.copy_(bufs[i].reshape(b.shape))
            self._has_state = True


def _warmup_factor_at(method: str, it: int, warmup_iters: int, warmup_factor: float) -> float:
    """utils.py:393-416: 1 after the warm-up; before it a constant, or a line from warmup_factor to 1."""
    if it >= warmup_iters:
        return 1.0
    if method == "constant":
        return warmup_factor
    if method == "linear":
        a = it / warmup_iters
        return warmup_factor * (1.0 - a) + a
    raise ValueError("Unknown warmup method: {}".format(method))


class WarmupMultiStepLR(torch.optim.lr_scheduler._LRScheduler):
    """utils.py:310-347: base_lr x warm-up x gamma^(milestones passed)."""

    def __init__(self, optimizer, milestones: Sequence[int], gamma: float = 0.1, warmup_factor: float = 0.001,
                 warmup_epochs: int = 5, warmup_method: str = "linear", last_epoch: int = -1):
        if list(milestones) != sorted(milestones):
            raise ValueError("Milestones should be a list of increasing integers. Got {}".format(milestones))
        self.milestones, self.gamma = list(milestones), gamma
        self.warmup_factor, self.warmup_epochs, self.warmup_method = warmup_factor, warmup_epochs, warmup_method
        super().__init__(optimizer, last_epoch)

    def get_lr(self) -> List[float]:
        w = _warmup_factor_at(self.warmup_method, self.last_epoch, self.warmup_epochs, self.warmup_factor)
        k = bisect_right(self.milestones, self.last_epoch)
        return [b * w * self.gamma ** k for b in self.base_lrs]


class WarmupCosineLR(torch.optim.lr_scheduler._LRScheduler):
    """utils.py:350-390: base_lr x warm-up x half cosine over ``max_iters``."""

    def __init__(self, optimizer, max_iters: int, warmup_factor: float = 0.001, warmup_epochs: int = 5,
                 warmup_method: str = "linear", last_epoch: int = -1):
        self.max_iters = max_iters
        self.warmup_factor, self.warmup_epochs, self.warmup_method = warmup_factor, warmup_epochs, warmup_method
        super().__init__(optimizer, last_epoch)

    def get_lr(self) -> List[float]:
        w = _warmup_factor_at(self.warmup_method, self.last_epoch, self.warmup_epochs, self.warmup_factor)
        c = 0.5 * (1.0 + math.cos(math.pi * self.last_epoch / self.max_iters))
        return [b * w * c for b in self.base_lrs]


def no_decay_groups(model, weight_decay: float):
    """The usual fine-tuning split as ``groups`` for ``FusedAdam`` / ``FusedSGD`` / ``FusedLion``: gains, biases, every other tensor of one
    dimension or none, ``logit_scale`` and ``logit_bias`` get weight decay 0, the matrices (and embeddings) ``weight_decay``.  Trainable
    parameters only, by name."""
    decay, no_decay = [], []
    for n, p in model.named_parameters():
        if p.requires_grad:
            (no_decay if p.ndim < 2 or n.endswith(".bias") or n in ("logit_scale", "logit_bias") else decay).append(n)
    return [g for g in ({"params": decay, "weight_decay": float(weight_decay)}, {"params": no_decay, "weight_decay": 0.0}) if g["params"]]


def build_optimizer(cfg: dict, model, fused: bool = True):
    """engine.py:129-151 (``cfg['optimizer']`` in {'sgd','adam'}); with ``fused`` both return the fused step, which also
    performs engine.py:89's clip_grad_norm_(.,1).  ``'lion'`` (not in the reference) returns ``FusedLion`` with ``cfg['lr']``,
    ``cfg['weight_decay']`` and ``cfg.get('betas', (0.9, 0.99))``; torch ships no Lion, so ``fused=False`` raises.  Frozen parameters: a model that describes its trainable ranges
    (``trainable_plan``: model.CLIP) keeps the fused step, which then updates those ranges only; any other model gets the stock
    SGD over the trainable ones (the fused step would update the whole flat buffer)."""
    if cfg["optimizer"] == "sgd":
        if fused and (hasattr(model, "trainable_plan") or all(p.requires_grad for p in model.parameters())):
            return FusedSGD(model, lr=cfg["lr"], momentum=cfg["momentum"], weight_decay=cfg["weight_decay"], max_norm=1.0)
        return torch.optim.SGD([p for p in model.parameters() if p.requires_grad], lr=cfg["lr"],
                               momentum=cfg["momentum"], weight_decay=cfg["weight_decay"])
    if cfg["optimizer"] == "adam":
        if fused:
            return FusedAdam(model, lr=cfg["lr"], weight_decay=cfg["weight_decay"], max_norm=1.0)
        return torch.optim.Adam([p for p in model.parameters() if p.requires_grad], lr=cfg["lr"],
                                weight_decay=cfg["weight_decay"])
    if cfg["optimizer"] == "lion":
        # not one of the reference's: the third optimiser of the CLIP recipes (FusedLion), with the reference's clip in front
        if not fused:
            raise NotImplementedError("build_optimizer: torch ships no Lion; 'lion' exists as the fused step only (fused=True), or "
                                      "build timm.optim.Lion / lion_pytorch.Lion yourself")
        return FusedLion(model, lr=cfg["lr"], betas=cfg.get("betas", (0.9, 0.99)), weight_decay=cfg["weight_decay"], max_norm=1.0)
    raise RuntimeError("Invalid optimizer '{}'. ".format(cfg["optimizer"]))


def build_lr_scheduler(cfg: dict, optimizer, begin_epoch: int = 0):
    """engine.py:154-176."""
    kind = cfg["lr_scheduler"]
    if kind == "multisteplr":
        return torch.optim.lr_scheduler.MultiStepLR(optimizer, milestones=cfg["lr_steps"], gamma=cfg["lr_gamma"])
    if kind == "cosineannealinglr":
        return torch.optim.lr_scheduler.CosineAnnealingLR(optimizer, T_max=cfg["max_epoch"] - begin_epoch)
    if kind == "warmup":
        return WarmupCosineLR(optimizer, cfg["max_epoch"], warmup_epochs=cfg["warmup_epoch"], last_epoch=begin_epoch - 1)
    if kind == "none":
        return None
    raise RuntimeError("Invalid lr scheduler '{}'. Only MultiStepLR and CosineAnnealingLR are supported.".format(kind))
