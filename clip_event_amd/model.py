"""Drop-in for the reference's ``model_clip.CLIP`` / ``build_model`` on MI355X.

Host-side mirror of ``/root/reference/src/clip-event/model_clip.py`` (ViT towers only):
same constructor signature (incl. the ``constrastive_overbatch`` spelling), attribute names,
state-dict keys/shapes, ``forward`` / ``encode_image`` / ``encode_text`` / ``sim_entity`` /
``set_hyps`` behaviour and return arity.  All device math is hand-written HIP behind the C ABI
(``include/clip_event_hip.h``); PyTorch only owns memory, the autograd graph edges between
the coarse ops and the process group.  No CPU / eager fallback: without the HIP library every
compute call raises.

Memory layout (MI355X-first): all fp32 master parameters live in ONE flat HBM buffer and all
gradients in another (``nn.Parameter``s are views), so the optimiser is two launches and the
data-parallel gradient exchange is one bucket per tower; bf16 GEMM operand copies (straight
and transposed) are refreshed from the masters when their version counters move.
"""
from __future__ import annotations

import contextlib
import ctypes
import math
import os
from ctypes import c_int, c_void_p
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import nn

from . import _lib as L
from ._lib import check, lib, ptr, stream
from .utils_image import patch_from_norm_bbox


# --------------------------------------------------------------------------- ctypes structs

class _BlockParams(ctypes.Structure):
    _fields_ = [(n, c_void_p) for n in (
        "ln1_w", "ln1_b", "ln2_w", "ln2_b", "b_qkv", "b_out", "b_fc", "b_proj",
        "w_qkv", "w_out", "w_fc", "w_proj", "wt_qkv", "wt_out", "wt_fc", "wt_proj",
        "g_ln1_w", "g_ln1_b", "g_ln2_w", "g_ln2_b", "g_b_qkv", "g_b_out", "g_b_fc", "g_b_proj",
        "g_w_qkv", "g_w_out", "g_w_fc", "g_w_proj",
        "w8_qkv", "w8_out", "w8_fc", "w8_proj", "s8_qkv", "s8_out", "s8_fc", "s8_proj",
        "wt8_qkv", "wt8_out", "wt8_fc", "wt8_proj", "st8_qkv", "st8_out", "st8_fc", "st8_proj")]


class _TowerDesc(ctypes.Structure):
    _fields_ = [("layers", c_int), ("width", c_int), ("heads", c_int), ("tokens", c_int), ("causal", c_int),
                ("blocks", ctypes.POINTER(_BlockParams)), ("fp8", c_int), ("stream16", c_int), ("wgrad_overwrite", c_int), ("grad_scale", c_void_p)]


# --------------------------------------------------------------------------- parameter holders
# Plain containers that reproduce the reference's module tree so that state_dict() yields the
# same keys in the same order (model_clip.py:171-183, :214-230, :317-330).

class _Affine(nn.Module):
    def __init__(self, d: int, bias_init: float = 0.0):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(d))
        self.bias = nn.Parameter(torch.zeros(d))


class _Linear(nn.Module):
    def __init__(self, d_in: int, d_out: int):
        super().__init__()
        bound = 1.0 / math.sqrt(d_in)
        self.weight = nn.Parameter(torch.empty(d_out, d_in).uniform_(-bound, bound))
        self.bias = nn.Parameter(torch.empty(d_out).uniform_(-bound, bound))


class _MHAParams(nn.Module):
    def __init__(self, d: int):
        super().__init__()
        self.in_proj_weight = nn.Parameter(torch.empty(3 * d, d))
        nn.init.xavier_uniform_(self.in_proj_weight)
        self.in_proj_bias = nn.Parameter(torch.zeros(3 * d))
        self.out_proj = _Linear(d, d)
        with torch.no_grad():
            self.out_proj.bias.zero_()


class _MLP(nn.Module):
    def __init__(self, d: int):
        super().__init__()
        self.c_fc = _Linear(d, 4 * d)
        self.c_proj = _Linear(4 * d, d)


class ResidualAttentionBlock(nn.Module):
    def __init__(self, d_model: int, n_head: int):
        super().__init__()
        self.attn = _MHAParams(d_model)
        self.ln_1 = _Affine(d_model)
        self.mlp = _MLP(d_model)
        self.ln_2 = _Affine(d_model)
        self.n_head = n_head


class Transformer(nn.Module):
    def __init__(self, width: int, layers: int, heads: int):
        super().__init__()
        self.width, self.layers, self.heads = width, layers, heads
        self.resblocks = nn.ModuleList([ResidualAttentionBlock(width, heads) for _ in range(layers)])


class _Conv1(nn.Module):
    def __init__(self, width: int, patch: int):
        super().__init__()
        fan_in = 3 * patch * patch
        bound = 1.0 / math.sqrt(fan_in)
        self.weight = nn.Parameter(torch.empty(width, 3, patch, patch).uniform_(-bound, bound))


class VisualTransformer(nn.Module):
    def __init__(self, input_resolution: int, patch_size: int, width: int, layers: int, heads: int, output_dim: int):
        super().__init__()
        self.input_resolution, self.output_dim, self.patch_size = input_resolution, output_dim, patch_size
        scale = width ** -0.5
        self.class_embedding = nn.Parameter(scale * torch.randn(width))
        self.patch_num = input_resolution // patch_size
        # the size and grid ``positional_embedding`` was built for; ``input_resolution`` / ``patch_num`` are those the tower RUNS at
        # (CLIP.set_image_size resamples the table for another size) and equal these until it is called
        self.native_resolution, self.native_patch_num = input_resolution, self.patch_num
        self.positional_embedding = nn.Parameter(scale * torch.randn(self.patch_num ** 2 + 1, width))
        self.proj = nn.Parameter(scale * torch.randn(width, output_dim))
        self.conv1 = _Conv1(width, patch_size)
        self.ln_pre = _Affine(width)
        self.transformer = Transformer(width, layers, heads)
        self.ln_post = _Affine(width)
        self.patch_dropout = 0.0          # CLIP.set_patch_dropout: fraction of the patches a training pass leaves out

    def patch_keep(self, p: Optional[float] = None) -> int:
        """Patches a pass keeps at dropout rate ``p`` (default: this tower's): ``max(1, int(N * (1 - p)))``, open_clip's rule."""
        p = self.patch_dropout if p is None else p
        n = self.patch_num ** 2
        return max(1, int(n * (1.0 - p)))


class _Embedding(nn.Module):
    def __init__(self, vocab: int, d: int):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(vocab, d))


# --------------------------------------------------------------------------- workspace pool

class _Pool:
    """Reusable device buffers keyed by (tag, bytes); a buffer is busy from a forward until the
    matching backward (or until the autograd context is dropped)."""

    def __init__(self):
        self.free: Dict[Tuple, List[torch.Tensor]] = {}

    def take(self, tag, nbytes: int, device) -> torch.Tensor:
        key = (tag, nbytes, str(device))
        lst = self.free.get(key)
        if lst:
            return lst.pop()
        return torch.empty(nbytes, dtype=torch.uint8, device=device)

    def give(self, tag, buf: torch.Tensor):
        self.free.setdefault((tag, buf.numel(), str(buf.device)), []).append(buf)


class _Lease:
    """Returns its buffer to the pool when garbage-collected (ctx freed) or released."""

    def __init__(self, pool: _Pool, tag, buf):
        self.pool, self.tag, self.buf = pool, tag, buf

    def release(self):
        if self.buf is not None:
            self.pool.give(self.tag, self.buf)
            self.buf = None

    def __del__(self):
        self.release()


class Stream16Saturation(FloatingPointError):
    """An fp16 residual-stream activation or gradient-stream value hit the +-65504 clamp (``CLIP.stream16``)."""

    def __init__(self, forward: int, gradient: int):
        self.forward, self.gradient = forward, gradient
        super().__init__(
            f"fp16 stream saturated: {forward} forward-stream and {gradient} gradient-stream LayerNorm slots saw a value at the "
            "+-65504 clamp; the affected step(s) used a clipped activation / gradient.  Set model.stream16 = False "
            "(CE_STREAM16=0: fp32 streams, as the reference) or, for the gradient stream, lower CE_GRAD_TARGET.")


# --------------------------------------------------------------------------- the model

_GEMM_SUFFIXES = ("attn.in_proj_weight", "attn.out_proj.weight", "mlp.c_fc.weight", "mlp.c_proj.weight")


# ---- partial fine-tuning: what is trainable, as tables over the flat layout ---------------------------------------------------
TOWERS = ("visual", "text")
_INPUT_SIDE = {"visual": ("visual.ln_pre.", "visual.conv1.", "visual.positional_embedding", "visual.class_embedding"),
               "text": ("token_embedding.", "positional_embedding")}
# low-rank adapters (CLIP.enable_lora): the block matrices that can carry them, and the matrix behind each name
LORA_TARGETS = ("in_proj", "out_proj", "c_fc", "c_proj")
_LORA_WEIGHT = dict(zip(LORA_TARGETS, _GEMM_SUFFIXES))
_LORA_SUFFIXES = ("lora_A", "lora_B")
SEGMENT, CHUNK = 2048, 1 << 16       # longest range of one workgroup: the optimiser's segment kernel, the table-driven gradient norm


def tower_of(name: str) -> str:
    """'visual', 'text' or 'head' (``logit_scale``, ``logit_bias``): the range of the flat layout a parameter lives in."""
    if name.startswith("visual."):
        return "visual"
    return "text" if name.startswith(("transformer.", "token_embedding.", "positional_embedding", "ln_final.", "text_projection")) else "head"


def block_of(name: str):
    """Index of the residual block a parameter belongs to, or None."""
    parts = name.split(".")
    return int(parts[parts.index("resblocks") + 1]) if "resblocks" in parts else None


def trainable_tables(offsets, shapes, flags, group_of=None, tile_names=()):
    """What a partially trainable model updates and runs, from names alone -- pure host arithmetic (no tensors, no GPU).

    ``offsets`` / ``shapes`` / ``flags``: flat offset, shape and ``requires_grad`` of every parameter name; ``group_of``: the
    parameter group of a name (missing: 0); ``tile_names``: the matrices that the optimiser updates in 64 x 64 tiles (in the order
    of the model's transpose-job table), everything else goes through segments.  Returns a dict:

      ``locked[tower]``      every parameter of the tower is frozen: it runs forward-only, without a stash;
      ``stop_layer[tower]``  the lowest block that owns a trainable parameter -- the backward ends there -- 0 when an input-side
                             parameter is trainable, and the number of blocks when only the output side (or nothing) is;
      ``tiles``              [(name, group)] of the trainable ``tile_names``;
      ``segments`` / ``segment_group``   [lo, hi) element ranges of at most 2048 elements covering every other trainable tensor,
                             and the group of each;
      ``chunks``             [lo, hi) ranges of at most 65536 elements covering every trainable tensor (the gradient norm).

    A range never crosses a tensor: the padding between tensors (offsets are multiples of 64) belongs to no range, except that the
    end of a tensor is rounded up to a multiple of 4 (the kernels move 16 bytes) -- up to three elements of its OWN padding, which
    hold zeros in every flat buffer and stay zero under every update rule.  A frozen tensor is in no table."""
    group_of = group_of or {}
    names = sorted(offsets, key=lambda n: offsets[n])
    numel = {n: int(np.prod(shapes[n], dtype=np.int64)) if len(shapes[n]) else 1 for n in names}
    layers = {t: 1 + max([block_of(n) for n in names if tower_of(n) == t and block_of(n) is not None], default=-1) for t in TOWERS}
    locked, stop = {}, {}
    for t in TOWERS:
        live = [n for n in names if tower_of(n) == t and flags[n]]
        locked[t] = not live
        if any(n.startswith(_INPUT_SIDE[t]) for n in live):
            stop[t] = 0
        else:
            stop[t] = min([block_of(n) for n in live if block_of(n) is not None], default=layers[t])
    tile_set = set(tile_names)
    tiles = [(n, int(group_of.get(n, 0))) for n in tile_names if flags[n]]
    segments, segment_group, chunks = [], [], []
    for n in names:
        if not flags[n]:
            continue
        lo, hi = offsets[n], offsets[n] + (numel[n] + 3) // 4 * 4
        for c in range(lo, hi, CHUNK):
            chunks.append((c, min(c + CHUNK, hi)))
        if n not in tile_set:
            for c in range(lo, hi, SEGMENT):
                segments.append((c, min(c + SEGMENT, hi)))
                segment_group.append(int(group_of.get(n, 0)))
    return {"locked": locked, "stop_layer": stop, "tiles": tiles, "segments": segments, "segment_group": segment_group,
            "chunks": chunks}


class TrainablePlan:
    """``CLIP.trainable_plan()``: ``trainable_tables`` of the model's current ``requires_grad`` flags, and -- once the model has
    its flat buffers -- the same tables in device memory, in the forms the kernels take: ``tjobs`` (transpose-job table, group in
    ``pad_``; ``(tensor, njobs, tiles)``), ``segments`` ([n, 2] int64), ``segment_group`` ([n] int32), ``chunks`` ([n, 2] int64).
    ``plain``: nothing is frozen."""

    def __init__(self, flags, tables):
        self.flags = flags
        self.plain = all(flags)
        self.locked, self.stop_layer = tables["locked"], tables["stop_layer"]
        self.host = tables
        self.tjobs = self.segments = self.segment_group = self.chunks = None


class CLIP(nn.Module):
    """``CLIP`` of model_clip.py:266-552 (ViT vision tower)."""

    def __init__(self, embed_dim: int, image_resolution: int, vision_layers: int, vision_width: int,
                 vision_patch_size: int, context_length: int, vocab_size: int, transformer_width: int,
                 transformer_heads: int, transformer_layers: int, constrastive_overbatch=True, alignment=False,
                 multiattention=False):
        super().__init__()
        if isinstance(vision_layers, (tuple, list)):
            raise NotImplementedError("ModifiedResNet towers are out of scope (BASELINE.json names ViT only)")
        # the length ``positional_embedding`` was built for; ``context_length`` is the one the text tower RUNS at
        # (set_context_length stretches or truncates the table for another length) and equals it until that is called
        self.context_length = self.native_context_length = context_length
        self.context_keep = 20
        self.vision_width = vision_width
        self.embed_dim = embed_dim
        vision_heads = vision_width // 64
        self.visual = VisualTransformer(image_resolution, vision_patch_size, vision_width, vision_layers,
                                        vision_heads, embed_dim)
        self.transformer = Transformer(transformer_width, transformer_layers, transformer_heads)
        self.vocab_size = vocab_size
        self.token_embedding = _Embedding(vocab_size, transformer_width)
        self.positional_embedding = nn.Parameter(torch.empty(context_length, transformer_width))
        self.ln_final = _Affine(transformer_width)
        self.text_projection = nn.Parameter(torch.empty(transformer_width, embed_dim))
        self.logit_scale = nn.Parameter(torch.ones([]) * np.log(1 / 0.07))
        self.initialize_parameters()
        self.constrastive_overbatch = constrastive_overbatch
        self.alignment = alignment
        self.multiattention = multiattention      # stored, never read: as in the reference
        from .losses import cross_entropy
        self.loss_func = cross_entropy            # the reference forgets to define it
        # device state (built lazily on the first forward on a GPU)
        self._flat: Optional[torch.Tensor] = None
        self._flat_grad: Optional[torch.Tensor] = None
        self._pool = _Pool()
        self._trigger = None
        self._versions = None
        self.grad_sync = None                     # optional callable(model, tower_name) for DP overlap
        # text tower on the live tokens only (rows after a caption's EOT are dead under the causal mask); results
        # are unchanged, see functional.text_packing.  CE_TEXT_PACK=0 keeps the dense [n, 77] layout.
        self.pack_text = os.environ.get("CE_TEXT_PACK", "1") != "0"
        # fp8 (OCP e4m3) operand path for the blocks' Linear GEMMs (BASELINE config 5; which tensors may go to low
        # precision follows convert_weights, model_clip.py:554-575): bit 0 = forward GEMMs, bit 1 = input-gradient
        # GEMMs.  fp32 masters, bf16 copies (weight gradients) and everything else are unchanged.  Off by default.
        self.fp8 = int(os.environ.get("CE_FP8", "0"))
        # Residual stream and gradient stream of both towers in IEEE fp16 instead of fp32 (include/clip_event_hip.h,
        # CE_T_F16): the stream is read and written four times per block and direction and never enters a matrix unit,
        # so this halves 40 % of a block's HBM traffic.  fp16's 11 significand bits keep the gradient noise floor where
        # the bf16 GEMM operands put it (tests/stream16_emulation.py).  The gradient stream is stored multiplied by a
        # power of two chosen per backward pass so that the largest element of the gradient entering the tower sits at
        # ``grad_target`` (ce_grad_scale; fp16 stores saturate at 65504, so 65504 / grad_target = 1024x is the growth the
        # gradient may see on its way down: measured x17-34 in the text tower, x1.1-1.3 in the image tower, tools/diag/grad_growth.py).  CE_STREAM16=0 keeps both streams in fp32 as the reference does.
        self.stream16 = os.environ.get("CE_STREAM16", "1") != "0"
        self.grad_target = float(os.environ.get("CE_GRAD_TARGET", "64"))
        # patch dropout (set_patch_dropout): the sampler's seed and the draw counter; neither is a parameter or a buffer, so
        # neither enters state_dict() or a checkpoint
        self.patch_seed = 0
        self.patch_draw = 0

    # ---- copy / pickle: the device-side tables (ctypes descriptors, workspace pool, streams, operand copies) are
    # rebuilt lazily by _prepare(); only the parameters and the plain attributes travel --------------------------
    _RUNTIME = ("_flat", "_flat_grad", "_flat16", "_offsets", "_ranges", "_layer_end", "_pmap", "_pool", "_trigger",
                "_versions", "_w16", "_w16t", "_kp", "_kp_real", "_conv_pad", "_conv_gpad", "_cast_list", "_tjobs",
                "_tjobs_bwd", "_adam_tiles_ok", "_wt_fresh", "_wt_event", "_aux_stream", "_mirror_fresh", "_mirror_versions", "_vdesc", "_tdesc", "_vblocks", "_tblocks",
                "_side_streams", "_main_stream", "_pack_cache", "_cls_rows", "_sat", "_sat_poll", "_step_events", "grad_sync", "_w8", "_fp8_fresh", "_zero_table", "_zero_tables", "_adam_segs", "_first_touch", "_lease_batch", "_route_longest", "_plist", "_plans", "_patch_pin", "_patch_off", "_lora_tab", "_pos_cache", "_pos_epoch", "_tpos_cache")

    def __getstate__(self):
        state = dict(self.__dict__)
        for k in self._RUNTIME:
            state.pop(k, None)
        return state

    def __setstate__(self, state):
        super().__setstate__(state)
        self._flat = None
        self._flat_grad = None
        self._pool = _Pool()
        self._trigger = None
        self._versions = None
        self.grad_sync = None
        for p in self.parameters():            # parameters arrive as copies of the views: gradients start afresh
            p.grad = None

    # ---- reference API -------------------------------------------------------------------
    def set_hyps(self, constrastive_overbatch=True, alignment=False, multiattention=False):
        self.constrastive_overbatch = constrastive_overbatch
        self.alignment = alignment
        self.multiattention = multiattention

    def enable_logit_bias(self, init: float = -10.0):
        """Register the scalar parameter ``logit_bias`` (the sigmoid pairwise loss adds it to every logit; SigLIP starts it at
        -10).  Opt-in: without this call the model has exactly the reference's parameters.  Call it before the optimiser is
        built.  The flat buffers, if they exist already, are dropped and rebuilt lazily with one more 64-element slot in the
        ``head`` range (``tower_of`` answers 'head').  A second call sets the value."""
        if getattr(self, "logit_bias", None) is not None:
            with torch.no_grad():
                self.logit_bias.fill_(float(init))
            return self.logit_bias
        dev = self.logit_scale.device
        self.logit_bias = nn.Parameter(torch.full([], float(init), dtype=torch.float32, device=dev))
        for k in ("_plist", "_plans"):
            self.__dict__.pop(k, None)
        if self._flat is not None:   # drop the device state as pickling does: _prepare() lays the parameters out anew on the next forward
            state = self.__getstate__()          # (the parameters stay views of the old buffer until then)
            self.__dict__.clear()
            self.__setstate__(state)
        return self.logit_bias

    # ---- low-rank adapters (LoRA), merged-operand form: DESIGN.md 4l ------------------------------------------------------------
    def _drop_layout(self):
        """Forget the flat layout (a parameter was added or removed): ``_prepare()`` lays the parameters out anew on the next
        forward; until then they stay views of the old buffer."""
        for k in ("_plist", "_plans"):
            self.__dict__.pop(k, None)
        if self._flat is not None:
            state = self.__getstate__()
            self.__dict__.clear()
            self.__setstate__(state)

    def _lora_holder(self, w0_name: str):
        """``(module, name of the A parameter, name of the B parameter)`` for the adapted matrix ``w0_name``."""
        mod_path, leaf = w0_name.rsplit(".", 1)
        mod = self.get_submodule(mod_path)
        return (mod, "in_proj_lora_A", "in_proj_lora_B") if leaf == "in_proj_weight" else (mod, "lora_A", "lora_B")

    def enable_lora(self, rank: int = 8, alpha: float = 16.0, targets=LORA_TARGETS, towers=TOWERS, layers=None,
                    freeze_base: bool = True, seed: int = 0):
        """Give the block matrices named by ``targets`` (of ``in_proj`` / ``out_proj`` / ``c_fc`` / ``c_proj``) in ``towers``
        low-rank adapters: ``W = W0 + (alpha / rank) B A`` with ``A [rank, in]`` and ``B [out, rank]`` registered as
        ``...attn.in_proj_lora_A/_B``, ``...attn.out_proj.lora_A/_B``, ``...mlp.c_fc.lora_A/_B``, ``...mlp.c_proj.lora_A/_B`` (fp32
        parameters in their block's range of the flat layout).  ``layers=n``: the top ``n`` blocks of each tower only.  Init as
        loralib / PEFT: ``A`` is ``kaiming_uniform_(a=sqrt(5))`` drawn from a ``torch.Generator`` seeded with ``seed``, ``B`` is 0,
        so the model computes what it computed before.  Every adapted ``W0`` is frozen (always), and with ``freeze_base`` every
        other parameter that is no adapter too; unfreeze what else should train (``logit_scale``, LayerNorms, ...) afterwards.

        The towers do not change: ``refresh_operands`` writes ``bf16(W0 + s B A)`` into the operand copies (``ce_lora_merge``) and
        ``finish_lora_grads`` turns the towers' weight gradient of ``W0`` into the gradients of ``A`` and ``B``.  Opt-in: call it
        before the optimiser is built.  A second call raises."""
        if getattr(self, "_lora", None) is not None:
            raise RuntimeError("enable_lora: the model has adapters already (merge_lora() folds them in and removes them)")
        if isinstance(rank, bool) or not isinstance(rank, int) or not 1 <= rank <= 64:
            raise ValueError(f"enable_lora: rank must be an integer in 1..64 (got {rank!r})")
        alpha = float(alpha)
        if not (math.isfinite(alpha) and alpha > 0.0):
            raise ValueError(f"enable_lora: alpha must be positive and finite (got {alpha})")
        targets = (targets,) if isinstance(targets, str) else tuple(targets)
        towers = (towers,) if isinstance(towers, str) else tuple(towers)
        if not targets or any(t not in LORA_TARGETS for t in targets) or len(set(targets)) != len(targets):
            raise ValueError(f"enable_lora: targets must be distinct names out of {LORA_TARGETS} (got {targets})")
        if not towers or any(t not in TOWERS for t in towers) or len(set(towers)) != len(towers):
            raise ValueError(f"enable_lora: towers must be distinct names out of {TOWERS} (got {towers})")
        if layers is not None and (isinstance(layers, bool) or not isinstance(layers, int) or layers < 1):
            raise ValueError(f"enable_lora: layers must be None or a positive integer (got {layers!r})")
        dev = self.logit_scale.device
        gen = torch.Generator().manual_seed(int(seed))
        saved = {n: p.requires_grad for n, p in self.named_parameters()}
        entries = []
        for tower in TOWERS:
            if tower not in towers:
                continue
            tr, prefix = (self.visual.transformer, "visual.transformer.") if tower == "visual" else (self.transformer, "transformer.")
            first = 0 if layers is None else max(0, tr.layers - layers)
            for blk in range(first, tr.layers):
                for t in LORA_TARGETS:
                    if t not in targets:
                        continue
                    w0_name = f"{prefix}resblocks.{blk}.{_LORA_WEIGHT[t]}"
                    mod, a_attr, b_attr = self._lora_holder(w0_name)
                    w0 = getattr(mod, w0_name.rsplit(".", 1)[1])
                    out_f, in_f = w0.shape
                    if out_f % 8 or in_f % 8:
                        raise ValueError(f"enable_lora: {w0_name} is {out_f} x {in_f}; adapted matrices need multiples of 8")
                    bound = 1.0 / math.sqrt(in_f)         # kaiming_uniform_(a = sqrt(5)): gain sqrt(1/3), bound sqrt(3) gain / sqrt(fan_in)
                    a = torch.empty(rank, in_f, dtype=torch.float32).uniform_(-bound, bound, generator=gen)
                    mod.register_parameter(a_attr, nn.Parameter(a.to(dev)))
                    mod.register_parameter(b_attr, nn.Parameter(torch.zeros(out_f, rank, dtype=torch.float32, device=dev)))
                    stem = w0_name.rsplit(".", 1)[0]
                    entries.append((w0_name, f"{stem}.{a_attr}", f"{stem}.{b_attr}"))
        adapters = {n for e in entries for n in e[1:]}
        frozen_w0 = {e[0] for e in entries}
        for n, p in self.named_parameters():
            if n in frozen_w0 or (freeze_base and n not in adapters):
                p.requires_grad_(False)
        self._lora = {"config": {"rank": rank, "alpha": alpha, "targets": list(targets), "towers": list(towers), "layers": layers,
                                 "freeze_base": bool(freeze_base), "seed": int(seed)},
                      "entries": entries, "saved_flags": saved}
        self._drop_layout()
        return self

    def lora_config(self):
        """``enable_lora``'s arguments as a plain dict (lists for the tuples), or None without adapters."""
        lora = getattr(self, "_lora", None)
        return None if lora is None else {k: (list(v) if isinstance(v, list) else v) for k, v in lora["config"].items()}

    def lora_parameter_names(self):
        """The adapters' parameter names, ``A`` before ``B`` for every adapted matrix, in table order."""
        lora = getattr(self, "_lora", None)
        return [] if lora is None else [n for e in lora["entries"] for n in e[1:]]

    def _lora_adapter_of(self):
        """adapter name -> the adapted matrix it belongs to (empty without adapters)."""
        lora = getattr(self, "_lora", None)
        return {} if lora is None else {n: e[0] for e in lora["entries"] for n in e[1:]}

    def lora_scale(self) -> float:
        """``alpha / rank`` rounded once to fp32."""
        cfg = self._lora["config"]
        return float(np.float32(cfg["alpha"] / cfg["rank"]))

    def _check_lora_frozen(self):
        lora = getattr(self, "_lora", None)
        if lora is None:
            return
        idx = lora.get("w0_index")
        if idx is None:
            names = [n for n, _ in self.named_parameters()]
            idx = lora["w0_index"] = [(names.index(e[0]), e[0]) for e in lora["entries"]]
        flags = self._flags()
        for i, n in idx:
            if flags[i]:
                raise RuntimeError(f"{n} carries adapters and has requires_grad=True: an adapted matrix stays frozen (its weight "
                                   "gradient is the adapters' input); merge_lora() first to train it directly")

    def _build_lora_table(self):
        """The ``ce_lora_job`` table of the adapters over the current flat layout: ``(host array, device copy, njobs, tiles, strips,
        workspace bytes)``, or None without adapters."""
        lora = getattr(self, "_lora", None)
        if lora is None:
            return None
        scale = self.lora_scale()
        rank = lora["config"]["rank"]
        specs = []
        for w, a, b in lora["entries"]:
            rows, cols = self._pmap[w].shape
            specs.append((self._pmap[w].data_ptr(), self._w16[w].data_ptr(), self._w16t[w].data_ptr(), self._pmap[a].data_ptr(),
                          self._pmap[b].data_ptr(), self._gview(w).data_ptr(), self._gview(a).data_ptr(), self._gview(b).data_ptr(),
                          rows, cols, rank, scale))
        host, tiles, strips = L.lora_job_table(specs)
        dev = torch.frombuffer(bytearray(bytes(host)), dtype=torch.uint8).to(self._flat.device)
        ws = int(lib().ce_lora_grad_workspace_bytes(host, len(specs)))
        if ws == 0:
            raise RuntimeError(f"ce_lora_grad_workspace_bytes refused the adapter table: {lib().ce_last_error().decode()}")
        return host, dev, len(specs), tiles, strips, ws

    def _operand_versions(self):
        """Versions of every master an operand copy is made from: the cast list and, with adapters, ``A`` and ``B``."""
        return tuple(self._pmap[n]._version for n in self._cast_list) + tuple(self._pmap[n]._version for n in self.lora_parameter_names())

    def _lora_merge(self, write_master: bool):
        host, dev, n, tiles, _, _ = self._lora_tab
        check(lib().ce_lora_merge(host, ptr(dev), n, tiles, int(write_master), stream()), "ce_lora_merge")

    def finish_lora_grads(self):
        """Turn the weight gradients of the adapted matrices into the adapters' gradients (``ce_lora_grad``, on the current stream):
        ``A.grad = s B^T dW``, ``B.grad = s dW A^T``, stored.  After ``backward()`` -- and after the gradient exchange of a
        data-parallel step -- and before anything reads ``A.grad`` / ``B.grad``: the fused optimisers call it in ``step()``, a loop
        with a stock optimiser calls it itself.  No-op without adapters; calling it again gives the same values."""
        if getattr(self, "_lora", None) is None or self._flat is None or not self._flat_ok():
            return
        self._check_lora_frozen()
        host, dev, n, _, strips, ws_bytes = self._lora_tab
        ws = self._pool.take("lora", ws_bytes, self._flat.device)
        check(lib().ce_lora_grad(host, ptr(dev), n, strips, ptr(ws), ws_bytes, stream()), "ce_lora_grad")
        self._pool.give("lora", ws)          # only this method takes the tag, always on the stream the step runs on
        base = self._flat_grad.data_ptr()
        for name in self.lora_parameter_names():
            p = self._pmap[name]
            if p.requires_grad and (p.grad is None or p.grad.data_ptr() != base + self._offsets[name] * 4):
                p.grad = self._gview(name)

    def lora_state_dict(self):
        """``{"config": lora_config(), "state": {adapter name: tensor}}`` (copies): the whole of a task's checkpoint."""
        if getattr(self, "_lora", None) is None:
            raise RuntimeError("lora_state_dict: the model has no adapters (enable_lora first)")
        pm = dict(self.named_parameters())
        return {"config": self.lora_config(), "state": {n: pm[n].detach().clone() for n in self.lora_parameter_names()}}

    def load_lora_state_dict(self, sd):
        """Load ``lora_state_dict()``'s format; a model without adapters gets them from ``sd["config"]`` first.  Names and shapes
        must match the model's."""
        if getattr(self, "_lora", None) is None:
            self.enable_lora(**sd["config"])
        state = sd["state"]
        pm = dict(self.named_parameters())
        names = self.lora_parameter_names()
        missing, extra = sorted(set(names) - set(state)), sorted(set(state) - set(names))
        if missing or extra:
            raise ValueError(f"adapter state does not match the model: missing {missing[:3]}, unexpected {extra[:3]}")
        for n in names:
            if tuple(state[n].shape) != tuple(pm[n].shape):
                raise ValueError(f"adapter state does not match the model: {n} is {tuple(state[n].shape)}, expected {tuple(pm[n].shape)}")
        with torch.no_grad():
            for n in names:
                pm[n].copy_(state[n])        # in place: the version moves, the next forward merges again

    def merge_lora(self):
        """Fold the adapters into the masters (``W0 <- fmaf(s, B A, W0)`` in fp32; on the GPU ``ce_lora_merge`` with
        ``write_master``), remove them and give every parameter the ``requires_grad`` flag it had before ``enable_lora``:
        afterwards the model is a plain one again and ``state_dict()`` has exactly the reference's keys."""
        lora = getattr(self, "_lora", None)
        if lora is None:
            raise RuntimeError("merge_lora: the model has no adapters")
        if self.positional_embedding.device.type == "cuda":
            self._check_lora_frozen()
            if not self._flat_ok():
                self._prepare()
            self.wait_transposes()
            self._lora_merge(write_master=True)
        else:
            s = self.lora_scale()
            pm = dict(self.named_parameters())
            with torch.no_grad():
                for w, a, b in lora["entries"]:
                    pm[w].add_(pm[b] @ pm[a], alpha=s)
        for w, _, _ in lora["entries"]:
            mod, a_attr, b_attr = self._lora_holder(w)
            del mod._parameters[a_attr], mod._parameters[b_attr]
        self._lora = None
        for n, p in self.named_parameters():
            p.requires_grad_(lora["saved_flags"].get(n, True))
        self._drop_layout()
        return self

    def load_state_dict(self, state_dict, strict: bool = True, **kw):
        """``nn.Module.load_state_dict``; a state dict without ``logit_bias`` (a reference checkpoint) loaded into a model that has
        the bias leaves the current bias value in place."""
        if getattr(self, "logit_bias", None) is not None and "logit_bias" not in state_dict:
            state_dict = dict(state_dict)
            state_dict["logit_bias"] = self.logit_bias.detach().clone()
        lora = getattr(self, "_lora", None)
        if lora is not None and not any(n in state_dict for n in self.lora_parameter_names()):
            # a plain state dict (the base model's) loaded under adapters: the adapters keep their values
            state_dict = dict(state_dict)
            pm = dict(self.named_parameters())
            for n in self.lora_parameter_names():
                state_dict[n] = pm[n].detach().clone()
        return super().load_state_dict(state_dict, strict=strict, **kw)

    def initialize_parameters(self):
        """model_clip.py:348-375 (text tower only; the vision tower keeps its constructor init)."""
        nn.init.normal_(self.token_embedding.weight, std=0.02)
        nn.init.normal_(self.positional_embedding, std=0.01)
        w, layers = self.transformer.width, self.transformer.layers
        proj_std = (w ** -0.5) * ((2 * layers) ** -0.5)
        attn_std = w ** -0.5
        fc_std = (2 * w) ** -0.5
        for block in self.transformer.resblocks:
            nn.init.normal_(block.attn.in_proj_weight, std=attn_std)
            nn.init.normal_(block.attn.out_proj.weight, std=proj_std)
            nn.init.normal_(block.mlp.c_fc.weight, std=fc_std)
            nn.init.normal_(block.mlp.c_proj.weight, std=proj_std)
        nn.init.normal_(self.text_projection, std=w ** -0.5)

    @property
    def dtype(self):
        return self.visual.conv1.weight.dtype

    # ---- flat parameter / gradient buffers ---------------------------------------------------
    def _flat_ok(self) -> bool:
        if self._flat is None:
            return False
        p = self.positional_embedding
        return p.device == self._flat.device and p.data_ptr() == self._flat.data_ptr() + self._offsets["positional_embedding"] * 4

    def _prepare(self):
        """Move every parameter into one flat fp32 buffer (views keep the reference's names)."""
        dev = self.positional_embedding.device
        if dev.type != "cuda":
            raise L.HipExtensionMissing("clip_event_amd computes on an AMD GPU only; move the model with .cuda() first")
        lib()
        named = list(self.named_parameters())
        offsets, off = {}, 0
        pmap = dict(named)
        # Contiguous range per tower, and inside a tower the parameters in the order their gradients become final
        # during the backward (output side first, residual blocks top-down, input embeddings last): the gradients
        # of "everything above block l" are then one contiguous prefix of the tower's range, which lets the
        # data-parallel all-reduce start on it while the lower blocks are still running (distributed.GradSync).
        text_side = ("token_embedding.", "positional_embedding", "ln_final.", "text_projection")

        def block_of(n):
            parts = n.split(".")
            return int(parts[parts.index("resblocks") + 1]) if "resblocks" in parts else None

        def tower_order(names, first, last_):
            head = [n for n in names if block_of(n) is None and any(n.startswith(f) for f in first)]
            tail = [n for n in names if block_of(n) is None and any(n.startswith(f) for f in last_)]
            rest = [n for n in names if block_of(n) is None and n not in head and n not in tail]
            if rest:
                raise RuntimeError(f"unplaced parameters {rest}")
            blocks = sorted({block_of(n) for n in names if block_of(n) is not None}, reverse=True)
            return head, [[n for n in names if block_of(n) == b] for b in blocks], blocks, tail

        groups = {
            "head": ([n for n, _ in named if not n.startswith(("visual.", "transformer.") + text_side)], [], [], []),
            "visual": tower_order([n for n, _ in named if n.startswith("visual.")],
                                  ("visual.ln_post.", "visual.proj"),
                                  ("visual.ln_pre.", "visual.conv1.", "visual.positional_embedding", "visual.class_embedding")),
            "text": tower_order([n for n, _ in named if n.startswith(("transformer.",) + text_side)],
                                ("ln_final.", "text_projection"), ("positional_embedding", "token_embedding.")),
        }
        ranges, layer_end = {}, {}
        # every boundary a gradient piece can end on (tower start / end, the end of every block) is a multiple of 8 x 64 elements:
        # a piece then splits into 2, 4 or 8 equal shards of whole 64-element groups (distributed.ShardPlan: reduce-scatter +
        # sharded Adam + all-gather of the bf16 mirror)
        PIECE = 512
        for group in ("head", "visual", "text"):
            head, per_block, blocks, tail = groups[group]
            off = (off + PIECE - 1) // PIECE * PIECE
            start = off
            layer_end[group] = {}
            for n in head:
                offsets[n] = off
                off += (pmap[n].numel() + 63) // 64 * 64
            for b, names_b in zip(blocks, per_block):
                for n in names_b:
                    offsets[n] = off
                    off += (pmap[n].numel() + 63) // 64 * 64
                off = (off + PIECE - 1) // PIECE * PIECE
                layer_end[group][b] = off          # gradients of blocks >= b (and the output side) end here
            for n in tail:
                offsets[n] = off
                off += (pmap[n].numel() + 63) // 64 * 64
            off = (off + PIECE - 1) // PIECE * PIECE
            ranges[group] = (start, off)
        if len(offsets) != len(named):
            raise RuntimeError("flat layout lost a parameter")
        self._layer_end = layer_end
        flat = torch.zeros(off, dtype=torch.float32, device=dev)
        flat_grad = torch.zeros(off, dtype=torch.float32, device=dev)
        with torch.no_grad():
            for n, p in named:
                if p.dtype != torch.float32:
                    raise RuntimeError(f"parameter {n} is {p.dtype}; master weights are fp32")
                view = flat[offsets[n]: offsets[n] + p.numel()].view(p.shape)
                view.copy_(p.data)
                p.data = view
                p.grad = None
        self._flat, self._flat_grad, self._offsets, self._ranges = flat, flat_grad, offsets, ranges
        self._pmap = pmap
        self._trigger = torch.zeros(1, device=dev, requires_grad=True)
        # fp16-stream saturation counters (include/clip_event_hip.h, ce_stream16_set_counters): [forward stream, gradient stream]
        self._sat = L.sat_counters(dev)
        self._sat_poll = None
        self._build_device_tables()
        self._versions = None

    def _gview(self, name: str) -> torch.Tensor:
        p = self._pmap[name]
        o = self._offsets[name]
        return self._flat_grad[o: o + p.numel()].view(p.shape)

    def _attach_grads(self):
        """Point every ``p.grad`` at its slice of the flat gradient buffer.  A slice whose
        ``p.grad`` was None (``zero_grad(set_to_none=True)``) is zero-filled first; a foreign
        ``p.grad`` tensor (autograd accumulated into a parameter before our backward ran, e.g.
        ``logit_scale``) is copied into its slice."""
        base = self._flat_grad.data_ptr()
        live = [(n, p) for n, p in self._pmap.items() if p.requires_grad]      # a frozen parameter keeps .grad None (torch's contract)
        todo = [(n, p) for n, p in live if p.grad is None or p.grad.data_ptr() != base + self._offsets[n] * 4]
        if not todo:
            return
        if all(p.grad is None for _, p in todo) and len(todo) == len(live) == len(self._pmap):
            self._flat_grad.zero_()
            for n, p in todo:
                p.grad = self._gview(n)
        else:
            adapters = self._lora_adapter_of()
            if any(p.grad is None and n in adapters for n, p in todo):
                # an adapter whose gradient was dropped (zero_grad(set_to_none=True)): the weight gradient of its frozen matrix, which
                # finish_lora_grads reads, starts from zero with it
                for w in {adapters[n] for n, p in todo if p.grad is None and n in adapters}:
                    self._gview(w).zero_()
            for n, p in todo:
                view = self._gview(n)
                if p.grad is None:
                    view.zero_()
                else:
                    view.copy_(p.grad)
                p.grad = view
        # The fills above ran on the stream of whichever backward node came first (a tower's side stream).  The
        # other tower's backward writes the same buffer from ITS stream: order it behind the fills, or its first
        # weight gradients land before the zero-fill and are wiped.
        cur = torch.cuda.current_stream()
        for s_ in (getattr(self, "_side_streams", None) or ()):
            if s_ != cur:
                s_.wait_stream(cur)
        ms = getattr(self, "_main_stream", None)
        if ms is not None and ms != cur:
            ms.wait_stream(cur)

    # ---- first-touch weight gradients ------------------------------------------------------------------------
    # The four Linear weights of every residual block are 85 % of the gradient buffer, and each receives its gradient
    # from exactly one (grouped) launch per tower pass.  A step that starts with ``zero_grad_first_touch`` zero-fills
    # only the OTHER tensors; the first backward pass of each tower then WRITES its block weight gradients
    # (ce_tower_desc.wgrad_overwrite: plain stores from unsplit tiles instead of float atomics), later passes of the
    # same step accumulate.  Until that first pass has run, ``.grad`` of those weights holds the previous step's
    # values, so only code that owns the whole step (engine.train_step with FusedAdam) takes this path;
    # ``zero_grad()`` keeps torch's contract.
    _BLOCK_WEIGHTS = ("attn.in_proj_weight", "attn.out_proj.weight", "mlp.c_fc.weight", "mlp.c_proj.weight")

    def _is_block_weight(self, name: str) -> bool:
        return "resblocks." in name and name.endswith(self._BLOCK_WEIGHTS)

    def _zero_table_for(self):
        """Chunk table of the gradient segments a first-touch step zero-fills: every element outside the block weights."""
        if getattr(self, "_zero_tables", None) is None:
            keep = sorted((self._offsets[n], self._offsets[n] + self._pmap[n].numel()) for n in self._pmap if self._is_block_weight(n))
            segs, pos = [], 0
            for lo, hi in keep:
                if lo > pos:
                    segs.append((pos, lo))
                pos = (hi + 63) // 64 * 64          # the padding behind a tensor is never read
            if pos < self._flat_grad.numel():
                segs.append((pos, self._flat_grad.numel()))
            chunks = []
            for lo, hi in segs:
                for c in range(lo, hi, 1 << 16):
                    chunks.append((c, min(c + (1 << 16), hi)))
            self._zero_tables = torch.tensor(chunks, dtype=torch.int64).reshape(-1, 2).to(self._flat_grad.device)
        return self._zero_tables

    def _adam_segment_table(self):
        """The zero-fill chunk table (= every element outside the block weights) cut into pieces of at most 2048 elements: one
        workgroup of ``ce_adam_step_tiles``' segment kernel each."""
        if getattr(self, "_adam_segs", None) is None:
            rows = []
            for lo, hi in self._zero_table_for().tolist():
                for c in range(lo, hi, 2048):
                    rows.append((c, min(c + 2048, hi)))
            self._adam_segs = torch.tensor(rows, dtype=torch.int64).reshape(-1, 2).to(self._flat_grad.device)
        return self._adam_segs

    def _zero_segments(self, table):
        if table.shape[0]:
            check(lib().ce_zero_segments(ptr(self._flat_grad), ptr(table), table.shape[0], stream()), "ce_zero_segments")

    def zero_grad_first_touch(self):
        if self._flat_grad is None or os.environ.get("CE_WGRAD_FIRST_TOUCH", "1") == "0":
            return self.zero_grad()
        self._zero_segments(self._zero_table_for())
        self._attach_grads_fast()
        self._first_touch = {"visual", "text"}

    def _settle_first_touch(self):
        """A tower whose backward did not run since ``zero_grad_first_touch``: its block weight gradients were neither
        zeroed nor written -- zero them now (called before the gradients are consumed)."""
        pending = getattr(self, "_first_touch", None)
        if not pending:
            return
        adapted = set(self._lora_adapter_of().values())
        for n, p in self._pmap.items():
            # (a frozen weight's gradient is in no table of the optimiser: nothing consumes it, nothing to settle -- unless it
            #  carries adapters: finish_lora_grads reads it)
            if (p.requires_grad or n in adapted) and self._is_block_weight(n) and (("visual" in pending and n.startswith("visual.")) or
                                                                 ("text" in pending and not n.startswith("visual."))):
                self._gview(n).zero_()
        self._first_touch = set()

    def zero_grad(self, set_to_none: bool = False):  # noqa: D401 - nn.Module API
        self._first_touch = set()
        if self._flat_grad is not None and not set_to_none:
            self._flat_grad.zero_()
            self._attach_grads_fast()
        else:
            super().zero_grad(set_to_none=set_to_none)

    def _attach_grads_fast(self):
        base = self._flat_grad.data_ptr()
        for n, p in self._pmap.items():
            if not p.requires_grad:
                if p.grad is not None and p.grad.data_ptr() == base + self._offsets[n] * 4:
                    p.grad = None         # frozen since it was attached: its slice is still written, and nothing consumes it
            elif p.grad is None or p.grad.data_ptr() != base + self._offsets[n] * 4:
                p.grad = self._gview(n)

    # ---- partial fine-tuning ---------------------------------------------------------------------------------------
    def _flags(self):
        """``requires_grad`` of every parameter, in ``named_parameters()`` order."""
        ps = self.__dict__.get("_plist")
        if ps is None:
            ps = self.__dict__["_plist"] = [p for _, p in self.named_parameters()]
        return tuple(p.requires_grad for p in ps)

    def trainable_plan(self, group_of=None, tiles: bool = True) -> TrainablePlan:
        """What the current ``requires_grad`` flags leave to train (``TrainablePlan``): which tower is locked, where each tower's
        backward may stop, and the optimiser's tables.  ``group_of`` (name -> parameter group, from the optimiser) and ``tiles``
        (block weights in 64 x 64 tiles rather than in segments) shape the tables only.  Cached; rebuilt when a flag, the groups
        or the flat buffers change."""
        flags = self._flags()
        flat = self._flat if self._flat is not None and self._flat_ok() else None
        key = (flags, tuple(sorted(group_of.items())) if group_of else None, bool(tiles), None if flat is None else flat.data_ptr())
        plans = self.__dict__.setdefault("_plans", {})
        plan = plans.get(key)
        if plan is not None:
            return plan
        named = list(self.named_parameters())
        fl = {n: f for (n, _), f in zip(named, flags)}
        if flat is None:           # no flat layout yet (a model on the host): towers only, the tables come with the layout
            offsets, off = {}, 0
            for n, p in named:
                offsets[n] = off
                off += (p.numel() + 63) // 64 * 64
            tile_names = []
        else:
            offsets = self._offsets
            tile_names = [n for n in self._pmap if n.endswith(_GEMM_SUFFIXES)] if tiles else []
        tables = trainable_tables(offsets, {n: tuple(p.shape) for n, p in named}, fl, group_of, tile_names)
        if flat is None:
            tables = {"locked": tables["locked"], "stop_layer": tables["stop_layer"]}
        plan = TrainablePlan(flags, tables)
        if flat is not None:
            dev = flat.device
            plan.tjobs = self._job_table([n for n, _ in tables["tiles"]], [g for _, g in tables["tiles"]])
            plan.segments = torch.tensor(tables["segments"], dtype=torch.int64).reshape(-1, 2).to(dev)
            plan.segment_group = torch.tensor(tables["segment_group"], dtype=torch.int32).to(dev)
            plan.chunks = torch.tensor(tables["chunks"], dtype=torch.int64).reshape(-1, 2).to(dev)
        if len(plans) >= 8:
            plans.clear()
        plans[key] = plan
        return plan

    def _lock_tower(self, tower: str, unlocked_layers: int):
        layers = (self.visual.transformer if tower == "visual" else self.transformer).layers
        n_open = max(0, min(int(unlocked_layers), layers))
        out_side = ("visual.ln_post.", "visual.proj") if tower == "visual" else ("ln_final.", "text_projection")
        for n, p in self.named_parameters():
            if tower_of(n) != tower:
                continue
            b = block_of(n)
            p.requires_grad_(n_open > 0 and ((b is not None and b >= layers - n_open) or n.startswith(out_side)))

    def lock_image_tower(self, unlocked_layers: int = 0):
        """Freeze the image tower except its top ``unlocked_layers`` blocks and, with any block open, ``ln_post`` + ``proj``
        (open_clip's spelling; only ``requires_grad`` flags are set).  Fully locked, the tower runs forward-only (LiT)."""
        self._lock_tower("visual", unlocked_layers)

    def lock_text_tower(self, unlocked_layers: int = 0):
        """The same for the text tower; the output side is ``ln_final`` + ``text_projection``."""
        self._lock_tower("text", unlocked_layers)

    # ---- fp16 residual / gradient stream: saturation telemetry ------------------------------------------------
    def stream16_saturation(self, reset: bool = False):
        """``(forward, gradient)`` counts of fp16-stream values that hit the +-65504 clamp since the counters were last
        reset (sticky device counters fed by every LayerNorm launch; synchronises).  Non-zero = some step computed with a
        clipped activation or gradient -- something the reference's non-finite-loss exit (engine.py:79-82) cannot see."""
        if getattr(self, "_sat", None) is None:
            return (0, 0)
        f, g = (int(v) for v in self._sat.cpu())
        if reset:
            self._sat.zero_()
        return (f, g)

    def poll_stream16_saturation(self):
        """The same check without a host synchronisation: starts an asynchronous copy of the counters and examines the copy
        the PREVIOUS call started (by then long complete).  Raises ``Stream16Saturation`` once a copy shows a clamp."""
        if getattr(self, "_sat", None) is None or not self.stream16:
            return
        prev = self._sat_poll
        if prev is not None and prev[1].query():
            f, g = (int(v) for v in prev[0])
            self._sat_poll = prev = None
            if f or g:
                raise Stream16Saturation(f, g)
        if prev is None:
            host = torch.empty(2, dtype=torch.int32, pin_memory=True)
            host.copy_(self._sat, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            self._sat_poll = (host, ev)

    # ---- bf16 operand copies + tower descriptors -------------------------------------------
    def _build_device_tables(self):
        dev = self._flat.device
        self._w16: Dict[str, torch.Tensor] = {}
        self._w16t: Dict[str, torch.Tensor] = {}
        # bf16 mirror of the whole flat parameter buffer (same offsets): the straight [out,in] operand copies
        # are views of it; the fused Adam kernel writes it together with the fp32 masters.
        self._flat16 = torch.empty(self._flat.numel(), dtype=torch.bfloat16, device=dev)

        def view16(n, shape=None):
            p = self._pmap[n]
            o = self._offsets[n]
            return self._flat16[o: o + p.numel()].view(p.shape if shape is None else shape)

        gemm_names = [n for n in self._pmap if n.endswith(_GEMM_SUFFIXES)]
        for n in gemm_names:
            p = self._pmap[n]
            self._w16[n] = view16(n)
            self._w16t[n] = torch.empty(p.shape[1], p.shape[0], dtype=torch.bfloat16, device=dev)
        v = self.visual
        kp = 3 * v.patch_size * v.patch_size
        self._kp_real = kp
        if kp % 8 == 0:
            self._kp = kp
            self._conv_pad = None
            self._w16["visual.conv1.weight"] = view16("visual.conv1.weight", (self.vision_width, kp))
        else:
            # patch 14 (ViT-L/14): 588 input columns.  The GEMM operands need 16-byte rows, so the patch matrix and
            # a private bf16 copy of the weight are zero-padded to a multiple of 64 columns; the weight gradient is
            # formed in a padded fp32 scratch and its real columns are added into the flat gradient buffer.
            self._kp = (kp + 63) // 64 * 64
            self._conv_pad = torch.zeros(self.vision_width, self._kp, dtype=torch.bfloat16, device=dev)
            self._conv_gpad = torch.zeros(self.vision_width, self._kp, dtype=torch.float32, device=dev)
            self._w16["visual.conv1.weight"] = self._conv_pad
        for n in ("visual.proj", "text_projection"):
            p = self._pmap[n]
            self._w16[n] = view16(n)                                                               # [width, E]
            self._w16t[n] = torch.empty(p.shape[1], p.shape[0], dtype=torch.bfloat16, device=dev)  # [E, width]
        self._cast_list = gemm_names + ["visual.conv1.weight", "visual.proj", "text_projection"]
        # one-launch transposition table for every W^T copy
        table = self._job_table

        # two tables: the feature projections' W^T are FORWARD operands; the blocks' W^T are read by the backward only
        # (input-gradient GEMMs), so their rebuild can run beside the next forward (refresh_operands)
        self._tjobs = table(["visual.proj", "text_projection"])
        self._tjobs_bwd = table(gemm_names)
        # fused Adam in tiles (optim.FusedAdam.step -> ce_adam_step_tiles) leaves these W^T copies behind itself: possible when the
        # table is exactly the block weights (whose complement is the zero-fill chunk table) and every matrix has 8-multiples
        self._adam_tiles_ok = (set(gemm_names) == {n for n in self._pmap if self._is_block_weight(n)} and
                               all(self._pmap[n].shape[0] % 8 == 0 and self._pmap[n].shape[1] % 8 == 0 for n in gemm_names))
        self._wt_fresh = False            # True when the fused Adam has just written the blocks' W^T copies as well
        self._wt_event = None
        self._mirror_fresh = False        # True when the Adam kernel has just written _flat16 ...
        self._mirror_versions = None      # ... from masters at these parameter versions

        def desc(prefix: str, tr: Transformer, tokens: int, causal: bool):
            arr = (_BlockParams * tr.layers)()
            for i in range(tr.layers):
                b = f"{prefix}resblocks.{i}."
                f = arr[i]

                def P(name):
                    return self._pmap[b + name].data_ptr()

                def G(name):
                    return self._gview(b + name).data_ptr()

                f.ln1_w, f.ln1_b, f.ln2_w, f.ln2_b = P("ln_1.weight"), P("ln_1.bias"), P("ln_2.weight"), P("ln_2.bias")
                f.b_qkv, f.b_out = P("attn.in_proj_bias"), P("attn.out_proj.bias")
                f.b_fc, f.b_proj = P("mlp.c_fc.bias"), P("mlp.c_proj.bias")
                for short, name in (("qkv", "attn.in_proj_weight"), ("out", "attn.out_proj.weight"),
                                    ("fc", "mlp.c_fc.weight"), ("proj", "mlp.c_proj.weight")):
                    setattr(f, "w_" + short, self._w16[b + name].data_ptr())
                    setattr(f, "wt_" + short, self._w16t[b + name].data_ptr())
                    setattr(f, "g_w_" + short, G(name))
                f.g_ln1_w, f.g_ln1_b, f.g_ln2_w, f.g_ln2_b = G("ln_1.weight"), G("ln_1.bias"), G("ln_2.weight"), G("ln_2.bias")
                f.g_b_qkv, f.g_b_out = G("attn.in_proj_bias"), G("attn.out_proj.bias")
                f.g_b_fc, f.g_b_proj = G("mlp.c_fc.bias"), G("mlp.c_proj.bias")
            d = _TowerDesc(tr.layers, tr.width, tr.heads, tokens, 1 if causal else 0, arr, 0, 0, 0, None)
            d._keep = arr
            return d

        self._vdesc = desc("visual.transformer.", self.visual.transformer, self.visual.native_patch_num ** 2 + 1, False)
        self._tdesc = desc("transformer.", self.transformer, self.native_context_length, True)
        self._w8 = None
        self._fp8_fresh = False
        self._lora_tab = self._build_lora_table()
        self._pos_cache = {}              # run grid -> (resampled positional table, what it was made from): _refresh_pos
        self._pos_epoch = 0
        self._tpos_cache = {}             # (run length, keep) -> (text positional table at that length, what it was made from)

    def _job_table(self, names, groups=None):
        """``(device table, njobs, tiles)``: one ``ce_transpose_job`` per name (bf16 operand copy -> its W^T copy); ``groups``
        (optional, one per name) goes into ``pad_``, where the grouped optimiser step reads the job's parameter group."""
        from ._lib import TransposeJob
        jobs = (TransposeJob * len(names))()
        tiles = 0
        for i, n in enumerate(names):
            src, dst = self._w16[n], self._w16t[n]
            jobs[i].src, jobs[i].dst = src.data_ptr(), dst.data_ptr()
            jobs[i].rows, jobs[i].cols, jobs[i].tile_start = src.shape[0], src.shape[1], tiles
            jobs[i].pad_ = 0 if groups is None else int(groups[i])
            tiles += ((src.shape[0] + 63) // 64) * ((src.shape[1] + 63) // 64)
        if not len(names):
            return None, 0, 0
        return torch.frombuffer(bytearray(bytes(jobs)), dtype=torch.uint8).to(self._flat.device), len(names), tiles

    def _build_fp8_tables(self):
        """e4m3 copies of the blocks' GEMM weights, one fp32 scale per row: straight [out,in] (scale per output
        channel) for the forward, transposed [in,out] (scale per input channel) for the input-gradient GEMMs."""
        dev = self._flat.device
        self._w8 = {}
        for prefix, d in (("visual.transformer.", self._vdesc), ("transformer.", self._tdesc)):
            for i in range(d.layers):
                f = d.blocks[i]
                for short, name in (("qkv", "attn.in_proj_weight"), ("out", "attn.out_proj.weight"),
                                    ("fc", "mlp.c_fc.weight"), ("proj", "mlp.c_proj.weight")):
                    n = f"{prefix}resblocks.{i}.{name}"
                    o, k = self._pmap[n].shape
                    t = (torch.empty(o, k, dtype=torch.uint8, device=dev), torch.empty(o, dtype=torch.float32, device=dev),
                         torch.empty(k, o, dtype=torch.uint8, device=dev), torch.empty(k, dtype=torch.float32, device=dev))
                    self._w8[n] = t
                    setattr(f, "w8_" + short, t[0].data_ptr())
                    setattr(f, "s8_" + short, t[1].data_ptr())
                    setattr(f, "wt8_" + short, t[2].data_ptr())
                    setattr(f, "st8_" + short, t[3].data_ptr())
        self._fp8_fresh = False
        self._qjobs_key = None

    def _refresh_fp8(self):
        """Requantise from the bf16 operand copies (they have just been refreshed from the masters)."""
        if self._w8 is None:
            self._build_fp8_tables()
        self.wait_transposes()            # with fp8 & 2 the quantiser reads the W^T copies an asynchronous rebuild may still be writing
        cl, s = lib(), stream()
        key = int(self.fp8) & 2
        if getattr(self, "_qjobs_key", None) != key:
            # one launch for every weight (and, with the input-gradient GEMMs in fp8, every transposed copy): a job table in
            # device memory, as for the transposes
            from ._lib import QuantJob
            jobs, groups = [], 0
            for n, (w8, s8, w8t, s8t) in self._w8.items():
                o, k = w8.shape
                todo = [(self._w16[n], w8, s8, o, k)] + ([(self._w16t[n], w8t, s8t, k, o)] if key else [])
                for src, dst, sc, rows, cols in todo:
                    if cols > 4096:
                        raise RuntimeError("fp8 weight rows longer than 4096 are not supported")
                    jobs.append(QuantJob(src.data_ptr(), dst.data_ptr(), sc.data_ptr(), cols, cols, rows, cols, groups, 0))
                    groups += (rows + 3) // 4
            arr = (QuantJob * len(jobs))(*jobs)
            host = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8)
            self._qjobs = host.to(self._flat.device)
            self._qjobs_n, self._qjobs_groups, self._qjobs_key = len(jobs), groups, key
        check(cl.ce_quant_rows_fp8_multi(ptr(self._qjobs), self._qjobs_n, self._qjobs_groups, s),
              "ce_quant_rows_fp8_multi")
        self._fp8_fresh = True

    def refresh_operands(self, force: bool = False):
        """Re-cast the bf16 GEMM operands from the fp32 masters when a master changed
        (in-place optimiser update, ``load_state_dict``)."""
        vers = self._operand_versions()
        self._vdesc.fp8 = self._tdesc.fp8 = int(self.fp8)
        self._vdesc.stream16 = self._tdesc.stream16 = 1 if self.stream16 else 0
        if not force and vers == self._versions:
            if self.fp8 and not self._fp8_fresh:
                self._refresh_fp8()
            self._refresh_pos(False)
            self._refresh_text_pos(False)
            return
        s = stream()
        cl = lib()
        # the bf16 mirror written by the fused Adam kernel is only as good as the masters it was cast from: if any
        # master has moved since (load_state_dict, a stock optimiser step, an EMA swap), cast again
        if not (self._mirror_fresh and vers == self._mirror_versions):
            self.wait_transposes()        # an earlier asynchronous rebuild may still be reading the mirror
            # masters changed outside the fused optimiser: rebuild the whole bf16 mirror (one launch)
            check(cl.ce_cast_bf16(ptr(self._flat), ptr(self._flat16), self._flat.numel(), s), "ce_cast_bf16")
        if self._lora_tab is not None:
            # adapters: the operand copies of every adapted matrix become bf16(W0 + s B A), the row-major mirror and W^T alike --
            # behind whoever wrote the mirror, in front of everything that reads it (the transposes below, _refresh_fp8)
            self.wait_transposes()
            self._lora_merge(write_master=False)
        tj, tn_, tt = self._tjobs
        check(cl.ce_multi_transpose_bf16(ptr(tj), tn_, tt, s), "ce_multi_transpose_bf16")
        tj, tn_, tt = self._tjobs_bwd
        if self._mirror_fresh and vers == self._mirror_versions and getattr(self, "_wt_fresh", False):
            pass                          # the fused Adam wrote the blocks' W^T copies with the update (ce_adam_step_tiles)
        elif getattr(self, "tower_streams", True) and not self.fp8 and os.environ.get("CE_ASYNC_TRANSPOSE", "1") != "0":
            # the blocks' W^T copies (0.15 ms of pure copying) on a third stream, beside the forward that is about to be
            # enqueued; every tower backward, and whoever rewrites the bf16 mirror next, waits for the event
            cur = torch.cuda.current_stream()
            if getattr(self, "_aux_stream", None) is None or self._aux_stream.device != self._flat.device:
                self._aux_stream = torch.cuda.Stream(device=self._flat.device)
            self._aux_stream.wait_stream(cur)
            with torch.cuda.stream(self._aux_stream):
                check(cl.ce_multi_transpose_bf16(ptr(tj), tn_, tt, stream()), "ce_multi_transpose_bf16(blocks)")
                self._wt_event = torch.cuda.Event()
                self._wt_event.record(self._aux_stream)
        else:
            self.wait_transposes()
            check(cl.ce_multi_transpose_bf16(ptr(tj), tn_, tt, s), "ce_multi_transpose_bf16(blocks)")
        if self._conv_pad is not None:
            check(cl.ce_cast_transpose(ptr(self._pmap["visual.conv1.weight"]), ptr(self._conv_pad), self._kp, None,
                                       0, self.vision_width, self._kp_real, s), "ce_cast_transpose(conv1)")
        self._mirror_fresh = False
        self._wt_fresh = False
        self._versions = vers
        self._fp8_fresh = False
        if self.fp8:
            self._refresh_fp8()
        self._refresh_pos(True)
        self._refresh_text_pos(True)

    # ---- the image tower at another resolution -------------------------------------------------------------------
    def set_image_size(self, size: Optional[int] = None):
        """Run (and train) the image tower on ``size`` x ``size`` inputs: a multiple of the patch size with
        ``(size / patch)^2 + 1 <= 4096`` tokens, square only.  ``None`` or the native size switches the feature off.  The parameter
        ``visual.positional_embedding`` keeps its shape; the tower adds the table resampled to the new grid (``posembed``) and the
        backward applies the transpose.  ``visual.input_resolution`` / ``visual.patch_num`` report the run size from here on,
        ``visual.native_resolution`` / ``visual.native_patch_num`` the parameter's.  A run-time switch like the patch-dropout rate:
        not a parameter or a buffer, so not in ``state_dict()`` or a checkpoint; it may change between steps.  Returns the size."""
        from .posembed import check_image_size
        v = self.visual
        size = v.native_resolution if size is None else int(size)
        g = check_image_size(size, v.patch_size)
        v.input_resolution, v.patch_num = size, g
        return size

    def _refresh_pos(self, moved: bool):
        """Keep the resampled positional table of the current run size in step with the parameter: ``moved`` (refresh_operands saw
        the masters move) drops every cached size; otherwise the table stands while the parameter's version does.  One small
        launch; at the native size nothing is allocated or launched."""
        if moved:
            self._pos_epoch += 1
        v = self.visual
        g = v.patch_num
        if g == v.native_patch_num:
            return
        from . import posembed
        p = self._pmap["visual.positional_embedding"]
        key = (self._pos_epoch, p._version)
        hit = self._pos_cache.get(g)
        if hit is not None and hit[1] == key:
            return
        table = posembed.resample(p.detach(), g, out=None if hit is None else hit[0])
        self._pos_cache[g] = (table, key)

    # ---- the text tower at another context length ----------------------------------------------------------------
    def set_context_length(self, T: Optional[int] = None, keep: int = 20):
        """Run (and train) the text tower on ``[n, T]`` token matrices, ``T`` in 2 .. 1024.  ``None`` or the native length switches
        the feature off.  The parameter ``positional_embedding`` keeps its shape ``[native_context_length, d]``; the tower adds the
        table ``posembed.text_weights(native, T, keep)`` makes of it -- longer: the first ``keep`` rows copied, the rest stretched
        linearly; shorter: truncated -- and the backward applies the transpose.  ``context_length`` reports the run length from here
        on, ``native_context_length`` the parameter's.  A run-time switch like ``set_image_size``: not a parameter or a buffer, so not
        in ``state_dict()`` or a checkpoint; it may change between steps.  Returns the length."""
        from .posembed import check_context_length
        T = self.native_context_length if T is None else check_context_length(T)
        keep = int(keep)
        if keep < 0:
            raise ValueError(f"keep must be non-negative (got {keep})")
        self.context_length, self.context_keep = T, keep
        return T

    def _refresh_text_pos(self, moved: bool):
        """``_refresh_pos`` for the text table: one small launch when the run length's table is missing or older than the
        parameter; at the native length nothing is allocated or launched."""
        T = self.context_length
        if T == self.native_context_length:
            return
        from . import posembed
        p = self._pmap["positional_embedding"]
        key = (self._pos_epoch, p._version)       # (_refresh_pos has advanced the epoch if the masters moved)
        hit = self._tpos_cache.get((T, self.context_keep))
        if hit is not None and hit[1] == key:
            return
        table = posembed.stretch(p.detach(), T, self.context_keep, out=None if hit is None else hit[0])
        self._tpos_cache[(T, self.context_keep)] = (table, key)

    def _text_pos_run(self):
        """The positional table the text tower adds at the current run length: None at the native length (the parameter itself)."""
        T = self.context_length
        return None if T == self.native_context_length else self._tpos_cache[(T, self.context_keep)][0]

    def _pos_run(self):
        """The positional table the image tower adds at the current run size: None at the native size (the parameter itself)."""
        v = self.visual
        return None if v.patch_num == v.native_patch_num else self._pos_cache[v.patch_num][0]

    def wait_transposes(self):
        """Order the current stream behind the asynchronous rebuild of the blocks' W^T copies (refresh_operands)."""
        ev = getattr(self, "_wt_event", None)
        if ev is not None:
            torch.cuda.current_stream().wait_event(ev)

    def mark_operands_stale(self, mirror_fresh: bool = False, wt_fresh: bool = False):
        """``mirror_fresh``: the caller (fused Adam) has already written the bf16 mirror of the new masters,
        only the transposed copies need rebuilding; ``wt_fresh``: it has written the blocks' W^T copies too."""
        self._versions = None
        self._mirror_fresh = mirror_fresh
        self._wt_fresh = bool(mirror_fresh and wt_fresh)
        self._mirror_versions = self._operand_versions() if mirror_fresh else None

    def _ready(self):
        if not self._flat_ok():
            self._prepare()
        dev = self._flat.device
        if torch.cuda.current_device() != dev.index:
            # launches go to the CURRENT device's stream: running a model that lives on another GPU would fault
            raise RuntimeError(f"the model lives on {dev} but the current device is cuda:{torch.cuda.current_device()}: "
                               "call torch.cuda.set_device() first (one process per GPU)")
        self._check_lora_frozen()
        self.refresh_operands()

    # ---- encoders -------------------------------------------------------------------------
    def _note_pass(self, tower: str, locked: bool = False):
        """Bookkeeping before a tower forward: refuse torch's DistributedDataParallel (its reducer waits for
        per-parameter autograd hooks that the HIP backward never fires -- an "unchanged" train.py would die on the
        second iteration inside the reducer with an unrelated message) and tell the gradient exchange that one more
        backward will write this tower's gradient range."""
        from torch.nn.parallel import DistributedDataParallel as TorchDDP
        if getattr(TorchDDP, "_active_ddp_module", None) is not None:
            raise RuntimeError(
                "clip_event_amd.CLIP cannot run inside torch.nn.parallel.DistributedDataParallel: parameter gradients "
                "are written by the HIP backward as side effects, so DDP's autograd hooks never fire.  Wrap the model "
                "with clip_event_amd.distributed.DistributedDataParallel(model, device_ids=[gpu]) instead (same call "
                "site, train.py:222-225; see INTEGRATION.md).")
        if self.grad_sync is not None and torch.is_grad_enabled() and not locked and hasattr(self.grad_sync, "note_forward"):
            self.grad_sync.note_forward(tower)

    # ---- patch dropout (FLIP; open_clip's PatchDropout): a training pass of the image tower sees the class token and a random
    # subset of the patches.  DESIGN.md 4e.
    def set_patch_dropout(self, p: float, seed: int = 0):
        """Leave out the fraction ``p`` of the patches (``0 <= p < 1``; 0 switches it off) in every ``encode_image`` pass with
        ``use_grid=False`` while the model is in training mode: ``visual.patch_keep()`` patches per image remain.  The kept
        patches are a pure function of ``seed``, the rank, ``patch_draw`` and the sample's row (``ce_patch_keep``)."""
        p = float(p)
        if not 0.0 <= p < 1.0:
            raise ValueError(f"patch dropout rate must lie in [0, 1) (got {p})")
        self.visual.patch_dropout = p
        self.patch_seed = int(seed)

    @contextlib.contextmanager
    def pinned_patch_draw(self, draw: int, sample0: int = 0):
        """Inside, every dropping pass uses draw ``draw`` and counts its samples from ``sample0``; ``patch_draw`` does not
        move.  This is how a pass is replayed (the two passes of a micro-batched chunk, a test against a reference)."""
        saved = getattr(self, "_patch_pin", None)
        self._patch_pin = (int(draw), int(sample0))
        try:
            yield self
        finally:
            self._patch_pin = saved

    @contextlib.contextmanager
    def no_patch_dropout(self):
        """Inside, no pass drops patches whatever ``training`` says (the inference helpers)."""
        saved = getattr(self, "_patch_off", False)
        self._patch_off = True
        try:
            yield self
        finally:
            self._patch_off = saved

    def drops_patches(self) -> bool:
        """Whether an ``encode_image(use_grid=False)`` call without an explicit keep list would drop patches now."""
        return bool(self.training and getattr(self.visual, "patch_dropout", 0.0) > 0.0 and not getattr(self, "_patch_off", False))

    def next_patch_draw(self) -> Tuple[int, int]:
        """``(draw, sample0)`` of the next dropping pass: the pinned pair, or the counter, which then advances."""
        pin = getattr(self, "_patch_pin", None)
        if pin is not None:
            return pin
        d = self.patch_draw
        self.patch_draw = d + 1
        return d, 0

    def _check_keep_idx(self, keep_idx, B: int, use_grid: bool):
        """Validate an explicit keep list that lives on the host (list, array, CPU tensor) -> int32 array [B, keep]; a device
        tensor is trusted (the kernels clamp what they read from it) and returned as it is."""
        if use_grid:
            raise ValueError("keep_idx with use_grid=True: a grid pass never drops patches, the grid is its output")
        n = self.visual.patch_num ** 2
        if isinstance(keep_idx, torch.Tensor) and keep_idx.device.type != "cpu":
            if keep_idx.dtype != torch.int32 or keep_idx.dim() != 2 or keep_idx.shape[0] != B or not 1 <= keep_idx.shape[1] <= n:
                raise ValueError(f"a device keep_idx must be int32 [{B}, 1..{n}] (got {keep_idx.dtype} {tuple(keep_idx.shape)})")
            return keep_idx.contiguous()
        try:
            a = np.asarray(keep_idx.numpy() if isinstance(keep_idx, torch.Tensor) else keep_idx)
        except Exception as e:       # ragged rows
            raise ValueError(f"keep_idx is not a rectangular [B, keep] list: {e}") from None
        if a.ndim != 2 or a.shape[0] != B or not 1 <= a.shape[1] <= n or a.dtype.kind not in "iu":
            raise ValueError(f"keep_idx must be integers of shape [{B}, 1..{n}] (got {a.dtype} {a.shape})")
        a = a.astype(np.int64)
        if a.min() < 0 or a.max() >= n:
            raise ValueError(f"keep_idx entries must lie in 0..{n - 1}")
        if a.shape[1] > 1 and not (np.diff(a, axis=1) > 0).all():
            raise ValueError("every row of keep_idx must be strictly ascending")
        return a.astype(np.int32)

    def _patch_tables(self, B: int, keep_idx):
        """Device tables of a dropping pass: ``(keep_idx int32 [B,keep], inv int32 [B,N])``, from the explicit list or from the
        sampler; None for a dense pass."""
        dev = self._flat.device
        n = self.visual.patch_num ** 2
        if keep_idx is not None:
            if isinstance(keep_idx, np.ndarray):
                keep_idx = torch.from_numpy(keep_idx).to(dev)
            # inverse table of a given list (not a training path: the sampler's launch writes both)
            inv = torch.full((B, n), -1, dtype=torch.int32, device=dev)
            slots = torch.arange(keep_idx.shape[1], dtype=torch.int32, device=dev).expand(B, -1)
            inv.scatter_(1, keep_idx.long().clamp_(0, n - 1), slots)
            return keep_idx, inv
        from .functional import patch_keep_seed
        keep = self.visual.patch_keep()
        draw, sample0 = self.next_patch_draw()
        rank = torch.distributed.get_rank() if (torch.distributed.is_available() and torch.distributed.is_initialized()) else 0
        keep_idx = torch.empty((B, keep), dtype=torch.int32, device=dev)
        inv = torch.empty((B, n), dtype=torch.int32, device=dev)
        check(lib().ce_patch_keep(patch_keep_seed(self.patch_seed, rank), draw, sample0, B, n, keep, ptr(keep_idx), ptr(inv),
                                  stream()), "ce_patch_keep")
        return keep_idx, inv

    def encode_image(self, image, use_grid: bool = False, keep_idx=None):
        """model_clip.py:390-391 -> VisualTransformer.forward (:232-263).

        Patch dropout: with ``use_grid=False``, in training mode and ``visual.patch_dropout > 0`` (``set_patch_dropout``) the
        tower runs on the class token and the sampled patches only -- in either grad mode, so that the micro-batched step's
        stash-free pass drops what its second pass drops.  ``keep_idx`` ([B, keep] patch indices, ascending per row) names
        the kept patches itself, in any mode.  A ``use_grid=True`` pass never drops: the grid is its output."""
        if keep_idx is not None:
            keep_idx = self._check_keep_idx(keep_idx, int(image.shape[0]), bool(use_grid))
        self._ready()
        locked = self.trainable_plan().locked["visual"]
        self._note_pass("visual", locked)
        from .functional import EncodeImageFn
        tables = (None, None)
        if keep_idx is not None or (not use_grid and self.drops_patches()):
            tables = self._patch_tables(int(image.shape[0]), keep_idx)
        if locked:       # nothing in the tower trains: forward-only even with grad mode on -- no stash, no autograd node
            with torch.no_grad():
                return EncodeImageFn.apply(image, self._trigger, self, bool(use_grid), True, *tables)
        # decided HERE: inside autograd.Function.forward grad mode is always off.  Without grad the tower keeps no stash.
        return EncodeImageFn.apply(image, self._trigger, self, bool(use_grid), not torch.is_grad_enabled(), *tables)

    def encode_text(self, text, lengths=None):
        """model_clip.py:398-417.  ``lengths`` (optional, host integers: tokens up to and including each caption's EOT) spares
        the text tower its one device read-back per new token tensor; ``functional.attach_lengths`` tags a tensor instead."""
        self._ready()
        locked = self.trainable_plan().locked["text"]
        self._note_pass("text", locked)
        from .functional import EncodeTextFn, attach_lengths
        if lengths is not None:
            attach_lengths(text, lengths)
        if locked:       # as encode_image
            with torch.no_grad():
                return EncodeTextFn.apply(text, self._trigger, self, True)
        return EncodeTextFn.apply(text, self._trigger, self, not torch.is_grad_enabled())

    def encode_both(self, image, text, use_grid: bool = False, keep_idx=None):
        """Image and text towers of one step (``keep_idx``: as in ``encode_image``).  They are independent until the logits, so with
        ``tower_streams`` (default) they run on two HIP streams: the ramp-up / tail of every kernel of one
        tower (and the CUs a ragged tile grid leaves idle) is filled by the other tower's kernels.  The
        autograd engine replays each tower's backward on its forward stream, so the backward overlaps too."""
        if keep_idx is not None:      # checked before anything is enqueued on the side streams
            keep_idx = self._check_keep_idx(keep_idx, int(image.shape[0]), bool(use_grid))
        self._ready()
        if not getattr(self, "tower_streams", True):
            self._main_stream = None
            return self.encode_image(image, use_grid, keep_idx), self.encode_text(text)
        if getattr(self, "_side_streams", None) is None or self._side_streams[0].device != self._flat.device:
            # the image tower is the longer chain: its stream gets the higher priority, the text tower's kernels fill
            # in around it (measured 0.7 % on the step; CE_IMG_STREAM_PRIORITY / CE_TXT_STREAM_PRIORITY override)
            pri = int(os.environ.get("CE_IMG_STREAM_PRIORITY", "-1"))
            self._side_streams = (torch.cuda.Stream(device=self._flat.device, priority=pri),
                                  torch.cuda.Stream(device=self._flat.device, priority=int(os.environ.get("CE_TXT_STREAM_PRIORITY", "0"))))
        s_img, s_txt = self._side_streams
        cur = torch.cuda.current_stream()
        self._main_stream = cur
        s_img.wait_stream(cur)
        s_txt.wait_stream(cur)
        with torch.cuda.stream(s_img):
            image_features = self.encode_image(image, use_grid, keep_idx)
        with torch.cuda.stream(s_txt):
            text_features = self.encode_text(text)
        cur.wait_stream(s_img)
        cur.wait_stream(s_txt)
        image_features.record_stream(cur)
        text_features.record_stream(cur)
        return image_features, text_features

    def forward(self, image, text, train_arg=None, bboxs=None, bbox_desc_vec=None, bbox_label_vec=None):
        """model_clip.py:419-528."""
        from .functional import logits_from_features
        if train_arg is None:
            image_features, text_features = self.encode_both(image, text)
            return logits_from_features(image_features, text_features, self.logit_scale, self.constrastive_overbatch)
        image_features, text_features, loss_per_bbox, loss_per_arg = self.encode_with_regions(
            image, text, train_arg, bboxs, bbox_desc_vec, bbox_label_vec)
        logits_per_image, logits_per_text = logits_from_features(
            image_features, text_features, self.logit_scale, self.constrastive_overbatch)
        return logits_per_image, logits_per_text, loss_per_bbox, loss_per_arg

    def encode_with_regions(self, image, text, train_arg, bboxs, bbox_desc_vec, bbox_label_vec):
        """The ``train_arg`` half of model_clip.py:419-488: both towers (image tower with its patch grid), then the
        region / argument losses from the grid.  Returns ``(image_features [B,E], text_features, loss_per_bbox,
        loss_per_arg)``; the caller forms the logits (locally, or over the all-gathered batch)."""
        from .region import region_losses
        image_features, text_features = self.encode_both(image, text, use_grid=True)
        B = image_features.size(0)
        pn = self.visual.patch_num
        grid_features = image_features[:, 1:, :].reshape(B, pn, pn, -1)
        image_features = image_features[:, 0, :]
        loss_per_bbox, loss_per_arg = region_losses(self, grid_features, bboxs, bbox_desc_vec, bbox_label_vec, train_arg)
        return image_features, text_features, loss_per_bbox, loss_per_arg

    def sim_entity(self, img_obj, txt_ent):
        """model_clip.py:531-552: un-normalised object / entity features."""
        B, n_img, n_txt = img_obj.size(0), img_obj.size(1), txt_ent.size(1)
        image_features = self.encode_image(img_obj.reshape(B * n_img, img_obj.size(2), img_obj.size(3), img_obj.size(4)))
        image_features = image_features.view(B, n_img, -1)
        text_features = self.encode_text(txt_ent.reshape(B * n_txt, txt_ent.size(2)), getattr(txt_ent, "_ce_lengths", None))
        text_features = text_features.view(B, n_txt, -1)
        return image_features, text_features


def build_model(state_dict: dict, lora: Optional[dict] = None) -> CLIP:
    """model_clip.py:578-617 (ViT branch): hyper-parameters inferred from tensor shapes, strict load,
    returned in train mode.  A state dict with adapter keys (``CLIP.enable_lora``) needs ``lora`` = the adapters' config
    (``lora_config()``; the ``'lora'`` entry of a checkpoint): the base model is built from the other keys, then
    ``enable_lora(**lora)``, then the adapters are loaded."""
    adapter_keys = [k for k in state_dict if k.endswith(_LORA_SUFFIXES)]
    if adapter_keys and lora is None:
        raise ValueError(f"the state dict holds low-rank adapters ({adapter_keys[0]}, ...) but no adapter config was given: pass "
                         "lora=<lora_config()> (checkpoint.load_checkpoint reads it from the checkpoint's 'lora' entry)")
    if lora is not None:
        base = {k: v for k, v in state_dict.items() if k not in set(adapter_keys)}
        model = build_model(base)
        model.enable_lora(**lora)
        if adapter_keys:
            model.load_lora_state_dict({"config": lora, "state": {k: state_dict[k] for k in adapter_keys}})
        return model
    if "visual.proj" not in state_dict:
        raise NotImplementedError("ModifiedResNet checkpoints are out of scope (ViT towers only)")
    vision_width = state_dict["visual.conv1.weight"].shape[0]
    vision_layers = len([k for k in state_dict.keys() if k.startswith("visual.") and k.endswith(".attn.in_proj_weight")])
    vision_patch_size = state_dict["visual.conv1.weight"].shape[-1]
    grid_size = round((state_dict["visual.positional_embedding"].shape[0] - 1) ** 0.5)
    image_resolution = vision_patch_size * grid_size
    embed_dim = state_dict["text_projection"].shape[1]
    context_length = state_dict["positional_embedding"].shape[0]
    vocab_size = state_dict["token_embedding.weight"].shape[0]
    transformer_width = state_dict["ln_final.weight"].shape[0]
    transformer_heads = transformer_width // 64
    transformer_layers = len(set(k.split(".")[2] for k in state_dict if k.startswith("transformer.resblocks")))
    model = CLIP(embed_dim, image_resolution, vision_layers, vision_width, vision_patch_size,
                 context_length, vocab_size, transformer_width, transformer_heads, transformer_layers)
    for key in ["input_resolution", "context_length", "vocab_size"]:
        if key in state_dict:
            del state_dict[key]
    if "logit_bias" in state_dict:          # a checkpoint of a model trained with the sigmoid loss
        model.enable_logit_bias(float(state_dict["logit_bias"]))
    model.load_state_dict(state_dict)
    return model
