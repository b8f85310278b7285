"""Coarse autograd nodes of the HIP path: one per tower pass, one for the logits.

Each ``forward`` issues the HIP launches through the C ABI and keeps the activation stash
(a leased workspace carved by the C++ tower runner) -- or, when grad mode was off at the call,
runs the forward-only tower (``ce_tower_forward_infer``) and keeps nothing; each ``backward`` runs the HIP backward
and accumulates parameter gradients directly into the model's flat gradient buffer (the
``nn.Parameter.grad`` views), returning ``None`` for the trigger input that only exists to put
the node on the autograd tape.
"""
from __future__ import annotations

import ctypes
import os
import weakref

import numpy as np
import torch

from . import _lib as L
from . import ops
from . import posembed
from ._lib import check, lib, ptr, stream


def _f32(t: torch.Tensor) -> torch.Tensor:
    return t if (t.dtype == torch.float32 and t.is_contiguous()) else t.contiguous().float()


def _tower_workspace(model, desc, batch: int, tag: str, infer: bool = False):
    """Lease the tower's workspace: the activation stash + backward scratch, or -- ``infer`` -- the forward-only buffers.
    ``model._lease_batch`` ({tag: samples}, set by the micro-batched step) sizes the lease for at least that many samples, so
    that a shorter last chunk runs in the full chunk's buffer (the pool is keyed by byte count and never frees)."""
    from .model import _Lease
    fn = lib().ce_tower_infer_workspace_bytes if infer else lib().ce_tower_workspace_bytes
    hint = getattr(model, "_lease_batch", None)
    nbytes = fn(ctypes.byref(desc), max(batch, hint.get(tag, 0)) if hint else batch)
    if nbytes == 0:
        raise RuntimeError(fn.__name__ + ": " + lib().ce_last_error().decode())
    if infer:
        tag = tag + ".infer"
    buf = model._pool.take(tag, int(nbytes), model._flat.device)
    return _Lease(model._pool, tag, buf)


def _tower_forward_infer(model, desc, tag: str, batch: int, rows: int, cu, x0, x_out, sel):
    """Tower forward that no backward will follow (``ce_tower_forward_infer``): nothing is stashed, the buffers go back to
    the pool as soon as the launches are enqueued (the next lease of this tag is taken on the same stream, as the
    training leases are)."""
    lease = _tower_workspace(model, desc, batch, tag, infer=True)
    check(lib().ce_tower_forward_infer(ctypes.byref(desc), batch, rows, ptr(cu), ptr(x0), ptr(lease.buf),
                                       ptr(x_out), ptr(sel), stream()), f"ce_tower_forward_infer({tag})")
    lease.release()


def _publish_to_main(ctx):
    """Parameter gradients are written as side effects on the stream this backward ran on (the tower's side
    stream); make the stream the step was issued from wait for them, so that an optimiser / clip_grad_norm_ /
    all-reduce enqueued there after ``backward()`` sees complete gradients."""
    ms = ctx.main_stream
    if ms is not None:
        cur = torch.cuda.current_stream()
        if cur != ms:
            ms.wait_stream(cur)


def _tower_backward(model, desc, tower: str, batch: int, rows: int, cu, x0, lease, dx, sel, dx_sel):
    """Tower backward, cut into layer ranges when a data-parallel gradient exchange is attached: after every
    range the gradients of the blocks done so far are handed to ``model.grad_sync`` (they form a contiguous
    prefix of the tower's range in the flat gradient buffer, model._prepare), so their all-reduce overlaps the
    remaining blocks.

    The ranges end at the tower's ``stop_layer`` (model.trainable_plan: the lowest block that owns a trainable parameter), which is
    returned: with a stop above 0 no kernel runs for the blocks below it, ``dx`` is not the gradient of the tower's input, and the
    caller has nothing left to do on the input side."""
    cl, s = lib(), stream()
    layers = desc.layers
    stop = model.trainable_plan().stop_layer[tower]
    cuts = model.grad_sync.layer_cuts(tower, layers) if (model.grad_sync is not None and
                                                           hasattr(model.grad_sync, "layer_cuts")) else []
    cuts = [c for c in cuts if c > stop]        # hand-overs below the stop: nothing is computed there
    # Block l's ln_1 backward also sums the c_proj bias gradient of block l - 1 (tower.cpp: fused into that kernel).  Below the stop
    # that tensor is frozen: the descriptor gets NULL there, as block 0 has for "no block below", and the kernel skips the sum.
    owner = getattr(desc, "_owner", desc)        # a shorter-sequence copy (_vision_desc) shares the owner's block table
    cut = getattr(owner, "_cut", 0)
    if cut != stop:
        prefix = "visual.transformer." if tower == "visual" else "transformer."
        if 0 < cut < layers:
            desc.blocks[cut - 1].g_b_proj = model._gview(f"{prefix}resblocks.{cut - 1}.mlp.c_proj.bias").data_ptr()
        if 0 < stop < layers:
            desc.blocks[stop - 1].g_b_proj = None
        owner._cut = stop
    model.wait_transposes()      # the blocks' W^T copies may still be in flight on the auxiliary stream (model.refresh_operands)
    # the step's first backward pass of this tower writes the block weight gradients instead of accumulating them
    # (model.zero_grad_first_touch); the flag is consumed here, so later passes of the same step accumulate
    pending = getattr(model, "_first_touch", None)
    desc.wgrad_overwrite = 1 if (pending and tower in pending) else 0
    if desc.wgrad_overwrite:
        pending.discard(tower)
    hi = layers - 1
    for lo in (list(cuts) + [stop] if stop < layers else []):
        check(cl.ce_tower_backward_range(ctypes.byref(desc), batch, rows, ptr(cu), ptr(x0), ptr(lease.buf), ptr(dx), ptr(sel),
                                         ptr(dx_sel), hi, lo, s), f"ce_tower_backward_range({tower})")
        if lo > stop:
            model.grad_sync(model, tower, upto_layer=lo)
        hi = lo - 1
    return stop


class TextPacking:
    """Row layout of one caption batch in the text tower.  ``cu is None``: dense, every caption owns
    ``context_length`` rows.  Otherwise only the live tokens (SOT .. EOT) are rows: ``cu`` int32 [n+1] prefix sums,
    ``src`` int32 [rows] flat index into the [n, T] id matrix, ``sel`` int32 [n] = each caption's EOT row, ``longest`` = the
    longest caption's length (host int; ``text_tower_tokens`` routes by it)."""
    __slots__ = ("rows", "cu", "src", "sel", "longest", "_keep")

    def __init__(self, rows, cu, src, sel, keep=None, longest=None):
        self.rows, self.cu, self.src, self.sel, self.longest, self._keep = rows, cu, src, sel, longest, keep


SHORT_ATTENTION_TOKENS = 128      # the one-workgroup-per-(sample, head) attention kernels' limit


def text_tower_tokens(run_length: int, longest: int, packed: bool) -> int:
    """The ``tokens`` the text tower's descriptor gets for one pass (forward, backward, workspace and ``lse`` alike) at run
    length ``run_length`` when the batch's longest caption has ``longest`` tokens.  Dense batches and contexts of at most 128
    tokens run at the run length (what they always did).  A packed batch of a longer context whose captions all fit 128
    tokens is sized for 128, so the short attention kernels run -- ordinary captions cost what they cost in a 77-token
    context; any longer caption sends the pass to the packed long kernels at the run length."""
    run_length, longest = int(run_length), int(longest)
    if not packed or run_length <= SHORT_ATTENTION_TOKENS:
        return run_length
    return SHORT_ATTENTION_TOKENS if longest <= SHORT_ATTENTION_TOKENS else run_length


def attach_lengths(text: torch.Tensor, lengths) -> torch.Tensor:
    """Tag a token tensor with its captions' HOST-side lengths (tokens up to and including the EOT = ``argmax + 1`` per row,
    model_clip.py:415): the tokenizer / data loader knows them before the batch is copied to the GPU, and with them the text
    tower sizes its launches without reading anything back from the device.  The tag lives on this tensor OBJECT (a
    ``.clone()`` / ``.to()`` result needs its own)."""
    text._ce_lengths = np.ascontiguousarray(np.asarray(lengths, dtype=np.int64).reshape(-1))
    return text


def host_lengths(text_cpu: torch.Tensor) -> np.ndarray:
    """``argmax(dim=-1) + 1`` of a CPU token matrix (first occurrence of the row maximum, as torch / numpy both define it)."""
    return text_cpu.reshape(-1, text_cpu.shape[-1]).numpy().argmax(axis=-1).astype(np.int64) + 1


def tokens_to_device(text: torch.Tensor, device) -> torch.Tensor:
    """``text.to(device)`` of engine.py:52 for a token matrix that is still on the host: the copy is asynchronous (pinned
    staging) and the result carries the host-side lengths (``attach_lengths``)."""
    if text.is_cuda:
        return text
    lens = getattr(text, "_ce_lengths", None)
    if lens is None:
        lens = host_lengths(text)
    if torch.device(device).type == "cuda" and not text.is_pinned():
        # a copy from pageable memory blocks the host until the stream has drained (the step could not run ahead any more):
        # stage it through pinned memory ourselves (tens of KB; the caching host allocator keeps the block until the copy is done)
        pin = torch.empty(text.shape, dtype=text.dtype, pin_memory=True)
        pin.copy_(text)
        text = pin
    out = text.to(device, non_blocking=True)
    out._ce_lengths = lens
    return out


_PACK_CACHE_SLOTS = 8


def _pack_key(text):
    base = text._base if text._base is not None else text
    return (id(base), text.storage_offset(), tuple(text.shape), tuple(text.stride()), text._version), base


def text_packing(model, text, lengths=None) -> TextPacking:
    """Drop the rows after each caption's EOT (model_clip.py:415 takes the feature AT the EOT; with the causal mask of
    model_clip.py:377-384 later rows can reach neither that feature nor any gradient, so the result is unchanged).
    The lengths size the launches, so the HOST needs them: from ``lengths`` / the tensor's ``attach_lengths`` tag (what a
    tokenizer or data loader knows anyway: no device round trip), else by one 4*n-byte read-back per NEW token tensor (the
    layout of a tensor seen before -- same storage, same version -- is reused; a small cache, so the fixed entity / role
    tensors of config 4 stay cached beside the captions).  ``CE_CHECK_LENGTHS=1`` checks given lengths against the device."""
    cl, s = lib(), stream()
    n, T = text.shape
    dev = text.device
    if lengths is None:
        lengths = getattr(text, "_ce_lengths", None)
    cache = getattr(model, "_pack_cache", None)
    if not isinstance(cache, dict):
        cache = model._pack_cache = {}
    key, base = _pack_key(text)
    key = key + (bool(model.pack_text),)
    hit = cache.get(key)
    if hit is not None and hit[0]() is base:
        return hit[1]
    if lengths is not None:
        lens = np.asarray(lengths, dtype=np.int64).reshape(-1)
        if lens.shape[0] != n or lens.min() < 1 or lens.max() > T:
            raise RuntimeError(f"text lengths must be {n} values in 1..{T}")
        if os.environ.get("CE_CHECK_LENGTHS", "0") == "1":
            dev_lens = (text.argmax(dim=-1) + 1).cpu().numpy()
            if not np.array_equal(dev_lens, lens):
                raise RuntimeError("attach_lengths / text_lengths disagree with argmax(text) + 1 on the device")
        flat = np.arange(n, dtype=np.int64) * T + lens - 1
        eot = None
    else:
        eot = _empty((n,), torch.int32, dev)
        check(cl.ce_eot_rows(ptr(text), ptr(eot), n, T, s), "ce_eot_rows")
        flat = None
    if not model.pack_text:
        if eot is None:
            meta = torch.empty(n, dtype=torch.int32, pin_memory=True)
            meta.numpy()[:] = flat
            eot = meta.to(dev, non_blocking=True)
            pk = TextPacking(n * T, None, None, eot, keep=(meta,))
        else:
            pk = TextPacking(n * T, None, None, eot)
    else:
        if flat is None:
            flat = eot.cpu().numpy().astype(np.int64)                   # host sync on this stream only
        lens = flat - np.arange(n, dtype=np.int64) * T + 1
        cu = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(lens, out=cu[1:])
        R = int(cu[-1])
        src = np.repeat(np.arange(n, dtype=np.int64) * T - cu[:-1], lens) + np.arange(R, dtype=np.int64)
        meta = torch.empty(2 * n + 1 + R, dtype=torch.int32, pin_memory=True)
        meta.numpy()[: n + 1] = cu
        meta.numpy()[n + 1: 2 * n + 1] = cu[1:] - 1
        meta.numpy()[2 * n + 1:] = src
        meta_d = meta.to(dev, non_blocking=True)
        pk = TextPacking(R, meta_d[: n + 1], meta_d[2 * n + 1:], meta_d[n + 1: 2 * n + 1], keep=(meta, meta_d),
                         longest=int(lens.max()))
    if len(cache) >= _PACK_CACHE_SLOTS:
        for k in [k for k, v in cache.items() if v[0]() is None] or [next(iter(cache))]:
            cache.pop(k, None)
    cache[key] = (weakref.ref(base), pk)
    return pk


def _empty(shape, dtype, dev):
    return torch.empty(shape, dtype=dtype, device=dev)


def _stream_type(model):
    """(torch dtype, CE_T_* code) of the residual stream: fp32, or IEEE fp16 with ``model.stream16``."""
    if getattr(model, "stream16", False):
        return torch.float16, L.T_F16
    return torch.float32, L.T_F32


def _grad_scale(model, desc, top_grad):
    """Device scalar: the power of two this pass's fp16 gradient stream is stored multiplied by, from the largest element
    of the fp32 gradient that enters the tower (``ce_grad_scale``).  None for an fp32 stream.  Also hands it to the tower
    descriptor (``ce_tower_desc.grad_scale``)."""
    if not getattr(model, "stream16", False):
        desc.grad_scale = None
        return None
    gs = ops.grad_scale(top_grad, model.grad_target)
    desc.grad_scale = gs.data_ptr()
    return gs


def _check_stream(ctx, model):
    if ctx.stream16 != bool(getattr(model, "stream16", False)):
        raise RuntimeError("model.stream16 changed between this pass's forward and its backward")


def _tower_top_forward(model, xN, ln: str, proj: str):
    """What follows a tower's blocks -- final LayerNorm, then projection (``visual.ln_post`` / ``visual.proj``,
    model_clip.py:256-261; ``ln_final`` / ``text_projection``, :413-415) -- on the consumed rows ``xN`` [n, D]:
    (features fp32 [n, E], LayerNorm output bf16 [n, D], mean, rstd)."""
    P = model._pmap
    h, mean, rstd = ops.layernorm_fwd_t(xN, P[ln + ".weight"], P[ln + ".bias"])
    return ops.gemm_nt(h, model._w16t[proj], L.EPI_F32), h, mean, rstd       # W^T copy [E, D]: features = h @ proj


def _tower_top_backward(model, desc, dfeat, xN, h, mean, rstd, ln: str, proj: str):
    """Backward of ``_tower_top_forward`` for the feature gradient ``dfeat`` (fp32 [n, E], contiguous): adds the gradients
    of the projection and of the LayerNorm's parameters, and returns (the fp32 gradient at the tower output [n, D], the
    gradient scale of this pass -- ``_grad_scale``, chosen from that tensor)."""
    P, G = model._pmap, model._gview
    dfb = torch.empty_like(dfeat, dtype=torch.bfloat16)
    check(lib().ce_cast_bf16(ptr(dfeat), ptr(dfb), dfeat.numel(), stream()), "ce_cast_bf16")
    dh = ops.gemm_nt(dfb, model._w16[proj], L.EPI_BF16)       # features = h @ proj  ->  dh = dF proj^T
    ops.gemm_tn(h, dfb, G(proj))                              # dproj += h^T dF
    dxn = ops.layernorm_bwd_t(dh, xN, mean, rstd, P[ln + ".weight"], G(ln + ".weight"), G(ln + ".bias"),
                              torch.empty_like(xN, dtype=torch.float32))
    return dxn, _grad_scale(model, desc, dxn)


def _tower_backward_done(ctx, tower: str, n_inputs: int):
    """Close of a tower node's backward: hand the tower's remaining gradients to the data-parallel exchange, make the step's
    stream wait for this one, and return the (absent) input gradients."""
    model = ctx.model
    if model.grad_sync is not None:
        model.grad_sync(model, tower)
    _publish_to_main(ctx)
    return (None,) * n_inputs


def patch_keep_seed(seed: int, rank: int = 0) -> int:
    """The seed ``ce_patch_keep`` receives on data-parallel rank ``rank``: ``(seed + rank * 0x632BE5AB) mod 2**32``, so that
    the ranks drop different patches of their (different) samples."""
    return (int(seed) + int(rank) * 0x632BE5AB) & 0xFFFFFFFF


def _vision_desc(model, tokens: int):
    """The image tower's descriptor at ``tokens`` rows per image: ``model._vdesc`` itself at the full length, otherwise a
    copy (cached per length on ``model._vdesc``, so it goes when the device tables are rebuilt) that shares the block table
    and whose per-pass switches are brought up to date here.  The workspace lease is sized from it: with patch dropout the
    stash shrinks with the rows."""
    return _desc_at(model._vdesc, tokens)


def _text_desc(model, pk: "TextPacking"):
    """The text tower's descriptor for the packing ``pk`` at the current run length (``text_tower_tokens``): ``model._tdesc``
    itself at the native length, otherwise a copy cached on it as ``_vision_desc``'s are.  ``model._route_longest`` (set by the
    micro-batched step: the longest caption of the whole step) keeps every chunk on the attention kernels the unchunked step takes."""
    T = model.context_length
    longest = T if pk.longest is None else max(pk.longest, getattr(model, "_route_longest", None) or 0)
    return _desc_at(model._tdesc, text_tower_tokens(T, longest, pk.cu is not None))


def _desc_at(base, tokens: int):
    if tokens == base.tokens:
        return base
    cache = base.__dict__.setdefault("_by_tokens", {})
    d = cache.get(tokens)
    if d is None:
        d = cache[tokens] = type(base)(base.layers, base.width, base.heads, tokens, base.causal, base.blocks, 0, 0, 0, None)
        d._keep = base._keep          # the block table the pointer refers to
        d._owner = base               # _tower_backward keeps the state of that (shared) table on the owner
    d.fp8, d.stream16 = base.fp8, base.stream16
    return d


class EncodeImageFn(torch.autograd.Function):
    """VisualTransformer.forward (model_clip.py:232-263) as one autograd node.  With ``keep_idx`` / ``inv`` (patch dropout,
    CLIP._patch_tables) the tower sees the class token and the listed patches only; ``use_grid`` is then off."""

    @staticmethod
    def forward(ctx, image, trigger, model, use_grid: bool, infer: bool = False, keep_idx=None, inv=None):
        cl, s = lib(), stream()
        v = model.visual
        dev = model._flat.device
        if image.device != dev:
            raise RuntimeError("image must live on the model's GPU")
        image = _f32(image)                                   # image.type(self.dtype), model_clip.py:391
        B = image.shape[0]
        R, ps, g, D, E = v.input_resolution, v.patch_size, v.patch_num, model.vision_width, model.embed_dim
        P = model._pmap
        if tuple(image.shape[1:]) != (3, R, R):
            raise RuntimeError(f"expected image [B,3,{R},{R}], got {tuple(image.shape)} (CLIP.set_image_size runs the tower at "
                               "another size)")
        N = g * g
        pos = model._pos_run()                                # the table resampled to this run size, DESIGN.md 4m
        if pos is None:
            pos = P["visual.positional_embedding"]
        if keep_idx is not None and (use_grid or tuple(keep_idx.shape) != (B, keep_idx.shape[1]) or tuple(inv.shape) != (B, N)):
            raise RuntimeError("patch dropout tables do not fit this pass")
        keep = N if keep_idx is None else keep_idx.shape[1]  # patch rows per image
        T = keep + 1
        M = B * T
        desc = _vision_desc(model, T)
        patches = _empty((B * keep, model._kp), torch.bfloat16, dev)
        if keep_idx is None:
            check(cl.ce_im2col(ptr(image), ptr(patches), B, R, ps, model._kp, s), "ce_im2col")
        else:
            check(cl.ce_im2col_rows(ptr(image), ptr(keep_idx), ptr(patches), B, keep, R, ps, model._kp, s), "ce_im2col_rows")
        patch_out = ops.gemm_nt(patches, model._w16["visual.conv1.weight"], L.EPI_F32)
        xpre = _empty((M, D), torch.float32, dev)
        if keep_idx is None:
            check(cl.ce_vision_assemble(ptr(patch_out), ptr(P["visual.class_embedding"]), ptr(pos),
                                        ptr(xpre), B, T, D, s), "ce_vision_assemble")
        else:
            check(cl.ce_vision_assemble_rows(ptr(patch_out), ptr(keep_idx), ptr(P["visual.class_embedding"]),
                                             ptr(pos), ptr(xpre), B, N, keep, D, s),
                  "ce_vision_assemble_rows")
        sdt, _ = _stream_type(model)                          # residual stream: fp32, or fp16 (model.stream16)
        x0, mean_pre, rstd_pre = ops.layernorm_fwd_t(xpre, P["visual.ln_pre.weight"], P["visual.ln_pre.bias"], sdt)
        if use_grid:
            rows, n = None, M
        else:                      # only the CLS row of each image is consumed (model_clip.py:256): pruned last block
            cache = model.__dict__.setdefault("_cls_rows", {})
            rows = cache.get((B, T, dev))
            if rows is None:                                   # built once per batch size (two torch launches otherwise)
                rows = cache[(B, T, dev)] = (torch.arange(B, device=dev, dtype=torch.int32) * T)
            n = B
        xN = _empty((n, D), sdt, dev)
        if infer:                  # grad mode was off at the call (CLIP.encode_image): no stash, nothing kept for a backward
            _tower_forward_infer(model, desc, "vision", B, M, None, x0, xN, rows)
        else:
            lease = _tower_workspace(model, desc, B, "vision")
            check(cl.ce_tower_forward(ctypes.byref(desc), B, M, None, ptr(x0), ptr(lease.buf), ptr(xN), ptr(rows), s),
                  "ce_tower_forward(vision)")
        feat, hpost, mean_post, rstd_post = _tower_top_forward(model, xN, "visual.ln_post", "visual.proj")
        if infer:
            return feat.view(B, T, E) if use_grid else feat
        ctx.model, ctx.lease, ctx.use_grid, ctx.B = model, lease, use_grid, B
        ctx.keep, ctx.inv, ctx.g = keep, inv, g
        ctx.stream16 = sdt == torch.float16
        ctx.main_stream = getattr(model, "_main_stream", None)
        ctx.saved = (patches, xpre, mean_pre, rstd_pre, x0, xN, rows, hpost, mean_post, rstd_post)
        return feat.view(B, T, E) if use_grid else feat

    @staticmethod
    def backward(ctx, dfeat):
        model, lease = ctx.model, ctx.lease
        if lease.buf is None:
            raise RuntimeError("backward through encode_image a second time: the activation stash was released")
        cl, s = lib(), stream()
        patches, xpre, mean_pre, rstd_pre, x0, xN, rows, hpost, mean_post, rstd_post = ctx.saved
        v = model.visual
        dev = model._flat.device
        B, g, D, E = ctx.B, ctx.g, model.vision_width, model.embed_dim      # the grid this pass ran at
        keep, inv = ctx.keep, ctx.inv                         # patch rows per image; patch dropout's inverse table or None
        T = keep + 1
        M = B * T
        desc = _vision_desc(model, T)
        model._attach_grads()
        P, G = model._pmap, model._gview
        _check_stream(ctx, model)
        # gradient w.r.t. the tower output (fp32): [B,D] in pruned mode (the tower's dx_sel) or [M,D] in grid mode, where it
        # IS the gradient stream on entry -- an fp16 stream holds gradient * scale, the scale chosen from this tensor
        dxn, gs = _tower_top_backward(model, desc, _f32(dfeat).reshape(-1, E), xN, hpost, mean_post, rstd_post,
                                      "visual.ln_post", "visual.proj")
        if rows is None:           # grid mode
            dx = dxn if gs is None else ops.cast_scaled(dxn, xN.dtype, gs)
            stop = _tower_backward(model, desc, "visual", B, M, None, x0, lease, dx, None, None)
        else:
            dx = _empty((M, D), xN.dtype, dev)
            stop = _tower_backward(model, desc, "visual", B, M, None, x0, lease, dx, rows, dxn)
        lease.release()
        if stop > 0:      # everything below block `stop` is frozen, the input side included: ln_pre, the embedding sums and the
            #               conv1 weight gradient have no reader
            return _tower_backward_done(ctx, "visual", 7)
        # ln_pre: x0 = LN(xpre); its dy is the gradient stream
        dxpre = ops.layernorm_bwd_t(dx, xpre, mean_pre, rstd_pre, P["visual.ln_pre.weight"], G("visual.ln_pre.weight"),
                                    G("visual.ln_pre.bias"), _empty((M, D), torch.float32, dev), gscale=gs)
        # positional / class embedding gradients: sums over the batch axis (with patch dropout a sample adds to the
        # positional rows of the patches it kept)
        if g != v.native_patch_num:
            # the tower ran on the resampled table: reduce into a scratch of that grid, then the transpose of the resampling adds
            # into the parameter's gradient (a frozen parameter has no reader for either)
            if P["visual.positional_embedding"].requires_grad:
                dpos = _empty((g * g + 1, D), torch.float32, dev)
                if inv is None:
                    check(cl.ce_batch_reduce(ptr(dxpre), ptr(dpos), B, T * D, T * D, 0, s), "ce_batch_reduce(pos)")
                else:           # rows that no sample kept stay zero
                    dpos.zero_()
                    check(cl.ce_pos_embed_bwd_rows(ptr(dxpre), ptr(inv), ptr(dpos), B, g * g, keep, D, s), "ce_pos_embed_bwd_rows")
                posembed.resample_backward(dpos, v.native_patch_num, accumulate=True, out=G("visual.positional_embedding"))
        elif inv is None:
            check(cl.ce_batch_reduce(ptr(dxpre), ptr(G("visual.positional_embedding")), B, T * D, T * D, 1, s),
                  "ce_batch_reduce(pos)")
        else:
            check(cl.ce_pos_embed_bwd_rows(ptr(dxpre), ptr(inv), ptr(G("visual.positional_embedding")), B, g * g, keep, D, s),
                  "ce_pos_embed_bwd_rows")
        check(cl.ce_batch_reduce(ptr(dxpre), ptr(G("visual.class_embedding")), B, T * D, D, 1, s), "ce_batch_reduce(cls)")
        # conv1 weight gradient: dW[width, 3*p*p] += dpatch^T patches   (no input gradient is ever needed)
        dpatch = _empty((B * keep, D), torch.bfloat16, dev)
        check(cl.ce_vision_assemble_bwd(ptr(dxpre), ptr(dpatch), B, T, D, s), "ce_vision_assemble_bwd")
        if model._conv_pad is None:        # the gradient view has the weight's 4-D shape: its rows are model._kp apart
            ops.gemm_tn(dpatch, patches, G("visual.conv1.weight"), ldo=model._kp)
        else:       # padded patch columns (model._build_device_tables): gradient through a padded scratch
            gp = model._conv_gpad
            gp.zero_()
            ops.gemm_tn(dpatch, patches, gp)
            check(cl.ce_add_cols(ptr(gp), model._kp, ptr(G("visual.conv1.weight")), model._kp_real, D, model._kp_real, s),
                  "ce_add_cols(conv1)")
        return _tower_backward_done(ctx, "visual", 7)


class EncodeTextFn(torch.autograd.Function):
    """CLIP.encode_text (model_clip.py:398-417) as one autograd node."""

    @staticmethod
    def forward(ctx, text, trigger, model, infer: bool = False):
        cl, s = lib(), stream()
        dev = model._flat.device
        if text.device != dev:
            raise RuntimeError("text must live on the model's GPU")
        if text.dtype != torch.int64:
            text = text.long()
        text = text.contiguous()
        n, T = text.shape
        if T != model.context_length:
            raise RuntimeError(f"expected {model.context_length} tokens per row, got {T}")
        D = model.transformer.width
        P = model._pmap
        pk = text_packing(model, text)
        M = pk.rows                                        # activation rows: live tokens only when packed
        sdt, ST = _stream_type(model)                      # residual stream: fp32, or fp16 (model.stream16)
        x0 = _empty((M, D), sdt, dev)
        pos = model._text_pos_run()                        # the table at this run length, DESIGN.md 4o
        if pos is None:
            pos = P["positional_embedding"]
        desc = _text_desc(model, pk)
        check(cl.ce_token_embed_t(ptr(text), ptr(pk.src), ptr(P["token_embedding.weight"]), ptr(pos),
                                  ptr(x0), ST, M, T, D, model.vocab_size, s), "ce_token_embed")
        rows = pk.sel                                      # EOT row of each caption (argmax token id, model_clip.py:415)
        xN = _empty((n, D), sdt, dev)                      # pruned last block: only the EOT rows are produced
        if infer:                  # grad mode was off at the call (CLIP.encode_text): no stash, nothing kept for a backward
            _tower_forward_infer(model, desc, "text", n, M, pk.cu, x0, xN, rows)
        else:
            lease = _tower_workspace(model, desc, n, "text")
            check(cl.ce_tower_forward(ctypes.byref(desc), n, M, ptr(pk.cu), ptr(x0), ptr(lease.buf), ptr(xN), ptr(rows),
                                      s), "ce_tower_forward(text)")
        feat, hfin, mean_f, rstd_f = _tower_top_forward(model, xN, "ln_final", "text_projection")
        if infer:
            return feat
        ctx.model, ctx.lease, ctx.n = model, lease, n
        ctx.T, ctx.keep, ctx.desc = T, model.context_keep, desc      # the run length, stretch and descriptor of THIS pass
        ctx.stream16 = sdt == torch.float16
        ctx.main_stream = getattr(model, "_main_stream", None)
        ctx.saved = (text, x0, xN, pk, hfin, mean_f, rstd_f)
        return feat

    @staticmethod
    def backward(ctx, dfeat):
        model, lease, n = ctx.model, ctx.lease, ctx.n
        if lease.buf is None:
            raise RuntimeError("backward through encode_text a second time: the activation stash was released")
        cl, s = lib(), stream()
        text, x0, xN, pk, hfin, mean_f, rstd_f = ctx.saved
        dev = model._flat.device
        T, D, desc = ctx.T, model.transformer.width, ctx.desc
        M, rows = pk.rows, pk.sel
        model._attach_grads()
        G = model._gview
        _check_stream(ctx, model)
        # dxn: [n, D] gradient at the EOT rows (dx_sel of the pruned tower: fp32)
        dxn, gs = _tower_top_backward(model, desc, _f32(dfeat), xN, hfin, mean_f, rstd_f, "ln_final", "text_projection")
        dx = _empty((M, D), xN.dtype, dev)
        stop = _tower_backward(model, desc, "text", n, M, pk.cu, x0, lease, dx, rows, dxn)
        lease.release()
        if stop > 0:      # as in EncodeImageFn.backward: no stream cast, no positional sum, no token-embedding scatter
            return _tower_backward_done(ctx, "text", 4)
        if gs is not None:            # the embedding gradients below take the fp32 gradient in true units
            dx = ops.cast_scaled(dx, torch.float32, gs, divide=True)
        native = T == model.native_context_length
        if not native and not model._pmap["positional_embedding"].requires_grad:
            dpos = None                                        # a frozen table has no reader for either step
        elif native:
            dpos = G("positional_embedding")
        else:
            # the tower ran on the run-length table: reduce into a scratch of that length, then the transpose of the stretch adds
            # into the parameter's gradient
            dpos = _empty((T, D), torch.float32, dev)
        if dpos is None:
            pass
        elif pk.cu is None:
            check(cl.ce_batch_reduce(ptr(dx), ptr(dpos), n, T * D, T * D, 1 if native else 0, s), "ce_batch_reduce(text pos)")
        else:
            if not native:
                dpos.zero_()
            check(cl.ce_pos_embed_bwd_packed(ptr(dx), ptr(pk.cu), ptr(dpos), n, T, D, s),
                  "ce_pos_embed_bwd_packed")
        if dpos is not None and not native:
            posembed.stretch_backward(dpos, model.native_context_length, ctx.keep, accumulate=True, out=G("positional_embedding"))
        check(cl.ce_token_embed_bwd(ptr(text), ptr(pk.src), ptr(dx), ptr(G("token_embedding.weight")), M, D, model.vocab_size, s),
              "ce_token_embed_bwd")
        return _tower_backward_done(ctx, "text", 4)


def _sgemm(A, sam, sak, Bm, sbk, sbn, C, M, N, K, alpha_ptr=None, alpha=1.0, alpha_exp=0, beta=0.0):
    check(lib().ce_sgemm(ptr(A), sam, sak, ptr(Bm), sbk, sbn, ptr(C), C.stride(0), M, N, K, ptr(alpha_ptr), alpha, alpha_exp,
                         beta, stream()), "ce_sgemm")


def _l2norm(f):
    """(f / |f| row by row, 1 / |f|) of a contiguous fp32 matrix (``ce_l2norm_fwd``)."""
    n, E = f.shape
    y, inv = torch.empty_like(f), _empty((n,), torch.float32, f.device)
    check(lib().ce_l2norm_fwd(ptr(f), E, ptr(y), E, ptr(inv), n, E, stream()), "ce_l2norm_fwd")
    return y, inv


def _l2norm_bwd(dy, y, inv):
    """Gradient w.r.t. f of ``y, inv = _l2norm(f)`` for the gradient ``dy`` w.r.t. y (``ce_l2norm_bwd``)."""
    n, E = y.shape
    df = torch.empty_like(y)
    check(lib().ce_l2norm_bwd(ptr(dy), E, ptr(y), E, ptr(inv), ptr(df), E, n, E, 0, stream()), "ce_l2norm_bwd")
    return df


def _index64(t, dev):
    """Labels / ``index_pos`` rows as the kernels read them: contiguous int64 on ``dev`` (None stays None)."""
    return None if t is None else t.to(device=dev, dtype=torch.int64).contiguous()


def _infonce_workspace(nq: int, dev):
    return _empty((lib().ce_infonce_workspace_bytes(nq),), torch.uint8, dev)


def _small_head_workspace(nI: int, nT: int, nsel: int, E: int, dev):
    """(workspace of ``ce_head_small_fwd``, index of its four result scalars)."""
    cl = lib()
    return (_empty((cl.ce_head_small_workspace_floats(nI, nT, nsel, E),), torch.float32, dev),
            cl.ce_head_small_scalars_offset(nI, nT, nsel, E))


class LogitsFn(torch.autograd.Function):
    """Feature normalisation + logits (model_clip.py:496-521).  ``text_all`` / ``image_all`` may be
    larger than the local features (all-gathered global batch): logits_per_image =
    s * I_local @ T_all^T, logits_per_text = s * T_local @ I_all^T."""

    @staticmethod
    def forward(ctx, fi, ft, logit_scale, overbatch: bool, want: str = "both"):
        cl, s = lib(), stream()
        dev = fi.device
        ctx.set_materialize_grads(False)
        fi, ft = _f32(fi), _f32(ft)
        B, E = fi.shape
        N = ft.shape[0]
        In, inv_i = _l2norm(fi)
        Tn, inv_t = _l2norm(ft)
        ls = logit_scale.detach().reshape(1)
        lpt = None
        # both matrices over the batch from the same features: logits_per_text IS logits_per_image^T (the same products summed in
        # the same order), so one GEMM + a transposed copy instead of two GEMMs; the backward folds the two gradients likewise
        ctx.twin = want == "both" and overbatch and os.environ.get("CE_HEAD_TWIN", "1") != "0"
        if want in ("both", "text") and not ctx.twin:
            lpt = _empty((N, B), torch.float32, dev)
            _sgemm(Tn, E, 1, In, 1, E, lpt, N, B, E, alpha_ptr=ls, alpha_exp=1)      # s * T I^T
        if want == "text":
            lpi = None
        elif overbatch:
            lpi = _empty((B, N), torch.float32, dev)
            _sgemm(In, E, 1, Tn, 1, E, lpi, B, N, E, alpha_ptr=ls, alpha_exp=1)      # s * I T^T
            if ctx.twin:
                lpt = lpi.t().contiguous()
        else:
            if N % B != 0:
                raise RuntimeError("per-instance logits need the same number of descriptions per image")
            K = N // B
            lpi = _empty((B, K), torch.float32, dev)
            check(cl.ce_instance_logits(ptr(In), ptr(Tn), ptr(ls), ptr(lpi), B, K, E, s), "ce_instance_logits")
        # the logits are this node's OUTPUTS: keeping the tensors themselves on ctx would close a cycle through their
        # grad_fn (= ctx) that Python's collector cannot see, and every step's whole graph (both towers' activation
        # stashes) would stay alive; detached aliases share the storage without the back edge
        ctx.saved = (In, Tn, inv_i, inv_t, ls, None if lpi is None else lpi.detach(), None if lpt is None else lpt.detach())
        ctx.overbatch = overbatch
        return lpi, lpt

    @staticmethod
    def backward(ctx, dlpi, dlpt):
        cl, s = lib(), stream()
        In, Tn, inv_i, inv_t, ls, lpi, lpt = ctx.saved
        dev = In.device
        B, E = In.shape
        N = Tn.shape[0]
        twin = ctx.twin and dlpi is not None and dlpt is not None
        dIn = torch.empty_like(In) if twin else torch.zeros_like(In)      # (twin: written, not accumulated)
        dTn = torch.empty_like(Tn) if twin else torch.zeros_like(Tn)
        dls = torch.zeros(1, dtype=torch.float32, device=dev)
        if twin:
            # lpt = lpi^T: dI = s (dlpi + dlpt^T) T, dT = s (dlpi + dlpt^T)^T I, ds = <dlpi + dlpt^T, lpi> / s-scaled as below
            G = torch.add(_f32(dlpi), _f32(dlpt).t())
            _sgemm(G, N, 1, Tn, E, 1, dIn, B, E, N, alpha_ptr=ls, alpha_exp=1)
            _sgemm(G, 1, N, In, E, 1, dTn, N, E, B, alpha_ptr=ls, alpha_exp=1)
            check(cl.ce_dot(ptr(G), ptr(lpi), G.numel(), ptr(dls), s), "ce_dot")
            dlpi = dlpt = None
        if dlpt is not None:
            dlpt = _f32(dlpt)
            # lpt = s T I^T : dT += s dlpt I ; dI += s dlpt^T T
            _sgemm(dlpt, B, 1, In, E, 1, dTn, N, E, B, alpha_ptr=ls, alpha_exp=1, beta=1.0)
            _sgemm(dlpt, 1, B, Tn, E, 1, dIn, B, E, N, alpha_ptr=ls, alpha_exp=1, beta=1.0)
            check(cl.ce_dot(ptr(dlpt), ptr(lpt), N * B, ptr(dls), s), "ce_dot")
        if dlpi is not None:
            dlpi = _f32(dlpi)
            if ctx.overbatch:
                _sgemm(dlpi, N, 1, Tn, E, 1, dIn, B, E, N, alpha_ptr=ls, alpha_exp=1, beta=1.0)
                _sgemm(dlpi, 1, N, In, E, 1, dTn, N, E, B, alpha_ptr=ls, alpha_exp=1, beta=1.0)
            else:
                check(cl.ce_instance_logits_bwd(ptr(dlpi), ptr(In), ptr(Tn), ptr(ls), ptr(dIn), ptr(dTn), B, N // B, E, s),
                      "ce_instance_logits_bwd")
            check(cl.ce_dot(ptr(dlpi), ptr(lpi), dlpi.numel(), ptr(dls), s), "ce_dot")
        return _l2norm_bwd(dIn, In, inv_i), _l2norm_bwd(dTn, Tn, inv_t), dls.reshape(()), None, None


def logits_from_features(image_features, text_features, logit_scale, overbatch: bool = True, want: str = "both"):
    """``want`` in {"both", "image", "text"}: skip the logits matrix that is not needed (global-batch
    path: each rank needs only its own row blocks)."""
    return LogitsFn.apply(image_features, text_features, logit_scale, bool(overbatch), want)


# ---- the fused loss heads: one autograd node per loss, one or two directions over a pair of feature matrices ---------------
# A node takes two raw feature matrices a, b.  Direction 0 scores query rows of a (the rows ``sel``, or all) against every row of
# b; direction 1, when asked for, rows of b against every row of a (one process: the keys of one direction are the queries of the
# other).  Each matrix is normalised once however many directions read it, every backward call adds into one gradient buffer per
# matrix, and one ``ce_l2norm_bwd`` per matrix follows.  A node returns one loss per direction (a bare tensor when there is one).
# The helpers below are that frame; what a loss calls in its forward and backward stays written out in its node.

def _head_normalise(a, b):
    """((a^, b^), (1 / |a|, 1 / |b|)): both matrices fp32 and L2-normalised row by row."""
    a, b = _f32(a), _f32(b)
    an, inv_a = _l2norm(a)
    bn, inv_b = _l2norm(b)
    return (an, bn), (inv_a, inv_b)


def _head_directions(mats, *given):
    """The directions of a node as its library calls read them, [(iq, nq, labels, sel)]: direction t takes its queries from
    ``mats[iq]`` (iq = t) and its keys from ``mats[1 - iq]``; ``given`` holds one (labels, sel) per direction."""
    dev = mats[0].device
    dirs = []
    for iq, (labels, sel) in enumerate(given):
        sel = _index64(sel, dev)
        dirs.append((iq, mats[iq].shape[0] if sel is None else sel.shape[0], _index64(labels, dev), sel))
    return dirs


def _head_upstream(gs, dev):
    """The upstream gradients of a node's losses as one fp32 tensor [directions] (a loss nobody used: 0)."""
    if len(gs) == 1:
        return gs[0].contiguous().float().reshape(1)
    zero = torch.zeros(len(gs), dtype=torch.float32, device=dev)
    return torch.stack([zero[t] if g is None else g.float().reshape(()) for t, g in enumerate(gs)])


def _head_grad_buffers(mats):
    """((da^, db^), four scalar slots): the accumulation targets of a backward, zeroed in ONE fill."""
    na, nb = mats[0].numel(), mats[1].numel()
    acc = torch.zeros(na + nb + 4, dtype=torch.float32, device=mats[0].device)
    return (acc[:na].view_as(mats[0]), acc[na:na + nb].view_as(mats[1])), acc[na + nb:]


def _head_result(losses):
    return losses[0] if losses.shape[0] == 1 else (losses[0], losses[1])


class InfoNCEFn(torch.autograd.Function):
    """mean_r CE(s q^_r . k^_c, label_r) over the query rows ``sel_ab`` (index_pos) of ``a`` against all rows of ``b`` --
    model_clip.py:496-521 + :633-662 for one direction -- without the [nq, nk] logits matrix (``ce_infonce_fwd/bwd``:
    similarity tiles on the fp32 matrix instruction, online log-sum-exp, backward from the saved log-sum-exp).  With
    ``labels_ba`` also the other direction on the same pair of matrices, the rows ``sel_ba`` of ``b`` against all rows of ``a``:
    the same kernels and arithmetic as two nodes, 14 launches instead of 26 on the stretch between the towers' forward and
    backward, where nothing else can run.  Across ranks, where queries and keys are different tensors: one direction per node."""

    @staticmethod
    def forward(ctx, a, b, logit_scale, labels_ab, sel_ab, labels_ba=None, sel_ba=None):
        cl, s = lib(), stream()
        dev = a.device
        mats, invs = _head_normalise(a, b)
        E = mats[0].shape[1]
        dirs = _head_directions(mats, (labels_ab, sel_ab), *([] if labels_ba is None else [(labels_ba, sel_ba)]))
        ls = logit_scale.detach().reshape(1)
        losses = torch.zeros(len(dirs), dtype=torch.float32, device=dev)                   # the merge kernel adds the rows' terms
        ws = _infonce_workspace(max(nq for _, nq, _, _ in dirs), dev)
        lses = []
        for t, (iq, nq, labels, sel) in enumerate(dirs):
            q, k = mats[iq], mats[1 - iq]
            lses.append(_empty((nq,), torch.float32, dev))
            check(cl.ce_infonce_fwd(ptr(q), E, ptr(sel), nq, ptr(k), E, k.shape[0], E, ptr(ls), ptr(labels), ptr(lses[t]),
                                    ptr(losses[t:t + 1]), ptr(ws), s), "ce_infonce_fwd")
        ctx.saved = (mats, invs, ls, dirs, lses)
        return _head_result(losses)

    @staticmethod
    def backward(ctx, *gs):
        cl, s = lib(), stream()
        mats, invs, ls, dirs, lses = ctx.saved
        E = mats[0].shape[1]
        g = _head_upstream(gs, mats[0].device)
        grads, scalars = _head_grad_buffers(mats)                                           # da^ | db^ | dlogit_scale
        for t, (iq, nq, labels, sel) in enumerate(dirs):
            q, k = mats[iq], mats[1 - iq]
            check(cl.ce_infonce_bwd(ptr(q), E, ptr(sel), nq, ptr(k), E, k.shape[0], E, ptr(ls), ptr(labels), ptr(lses[t]),
                                    ptr(g[t:t + 1]), ptr(grads[iq]), ptr(grads[1 - iq]), ptr(scalars[0:1]), s), "ce_infonce_bwd")
        return (_l2norm_bwd(grads[0], mats[0], invs[0]), _l2norm_bwd(grads[1], mats[1], invs[1]), scalars[0].reshape(()),
                None, None, None, None)


def fused_head_ok(embed_dim: int) -> bool:
    return embed_dim % 128 == 0 and 128 <= embed_dim <= 1024


def small_head_ok(fi, ft, index_pos) -> bool:
    """Shapes the three-launch head (csrc/head_small.hip) takes."""
    nI, E = fi.shape
    nT = ft.shape[0]
    nsel = nT if index_pos is None else int(index_pos.shape[0])
    return (fi.dim() == 2 and ft.dim() == 2 and ft.shape[1] == E and 1 <= nI <= 1024 and 1 <= nT <= 1024 and 1 <= nsel <= nT
            and E % 4 == 0 and E <= 1024)


class SmallHeadFn(torch.autograd.Function):
    """Normalisation + logits over the batch + CriterionContrastive('ce') (model_clip.py:496-521, :633-662) as ONE node of three
    launches -- two in the forward, one in the backward -- for batches whose logits matrix is small (config 2: 256 x 256):
    between the towers' forward and backward nothing else runs, and the general head is 21 launches / 200 us there."""

    @staticmethod
    def forward(ctx, fi, ft, logit_scale, labels_i, labels_t, sel):
        dev = fi.device
        fi, ft = _f32(fi), _f32(ft)
        nI, E = fi.shape
        nT = ft.shape[0]
        labels_i, labels_t, sel = _index64(labels_i, dev), _index64(labels_t, dev), _index64(sel, dev)
        nsel = nT if sel is None else int(sel.shape[0])
        ws, off = _small_head_workspace(nI, nT, nsel, E, dev)
        ls = logit_scale.detach().reshape(1)
        check(lib().ce_head_small_fwd(ptr(fi), ptr(ft), nI, nT, E, ptr(ls), ptr(labels_i), ptr(labels_t), ptr(sel), nsel, ptr(ws),
                                      stream()), "ce_head_small_fwd")
        ctx.saved = (ws, ls, sel, (nI, nT, nsel, E))
        return ws[off], ws[off + 1]

    @staticmethod
    def backward(ctx, g_i, g_t):
        ws, ls, sel, (nI, nT, nsel, E) = ctx.saved
        dev = ws.device
        g_i = None if g_i is None else g_i.float()
        g_t = None if g_t is None else g_t.float()
        dfi, dft = _empty((nI, E), torch.float32, dev), _empty((nT, E), torch.float32, dev)
        dls = _empty((1,), torch.float32, dev)
        check(lib().ce_head_small_bwd(nI, nT, nsel, E, ptr(ls), ptr(g_i), ptr(g_t), ptr(sel), ptr(ws), ptr(dfi), ptr(dft), ptr(dls),
                                      stream()), "ce_head_small_bwd")
        return dfi, dft, dls.reshape(()), None, None, None


def small_contrastive_losses(fi, ft, logit_scale, labels_per_image, labels_per_text, index_pos):
    loss_i, loss_t = SmallHeadFn.apply(fi, ft, logit_scale, labels_per_image, labels_per_text, index_pos)
    return {"loss_i": loss_i, "loss_t": loss_t}


def fused_contrastive_losses(fi, ft, fi_all, ft_all, logit_scale, labels_per_image, labels_per_text, index_pos):
    """``CriterionContrastive('ce')`` over the batch on raw features: loss_i = CE(s I^ T_all^T, labels_per_image),
    loss_t = CE over the ``index_pos`` rows of s T^ I_all^T (model_clip.py:633-662), the logits never materialised."""
    if fi_all is fi and ft_all is ft:          # one process: one node for both directions
        loss_i, loss_t = InfoNCEFn.apply(fi, ft, logit_scale, labels_per_image, None, labels_per_text, index_pos)
        return {"loss_i": loss_i, "loss_t": loss_t}
    return {"loss_i": InfoNCEFn.apply(fi, ft_all, logit_scale, labels_per_image, None),
            "loss_t": InfoNCEFn.apply(ft, fi_all, logit_scale, labels_per_text, index_pos)}


class MultiPosHeadFn(torch.autograd.Function):
    """Softmax cross entropy against the uniform distribution over each query's SET of positives (UniCL's supervised contrastive
    loss; with one positive per row ``InfoNCEFn``): key c is a positive of query r when ``groups_b[c] == groups_a[src(r)]`` and
    the id is not negative.  mean over the query rows ``sel_ab`` of ``a`` (rows without a positive add nothing, the divisor
    stays the row count) against all rows of ``b``, without the logits matrix (``ce_multipos_head_fwd/bwd``: the positives are
    counted and their logits summed in the sweep that takes the log-sum-exp).  ``both``: also the rows ``sel_ba`` of ``b`` against
    all rows of ``a`` -- the same two id vectors, read the other way round.  Across ranks, where the keys are gathered: one direction
    per node, ``groups_b`` the ids of the gathered rows."""

    @staticmethod
    def forward(ctx, a, b, logit_scale, groups_a, groups_b, sel_ab, both=False, sel_ba=None):
        cl, s = lib(), stream()
        dev = a.device
        mats, invs = _head_normalise(a, b)
        E = mats[0].shape[1]
        groups = (_index64(groups_a, dev), _index64(groups_b, dev))
        if groups[0].shape[0] != mats[0].shape[0] or groups[1].shape[0] != mats[1].shape[0]:
            raise RuntimeError(f"multi-positive head: {groups[0].shape[0]} / {groups[1].shape[0]} group ids for "
                               f"{mats[0].shape[0]} / {mats[1].shape[0]} feature rows")
        dirs = _head_directions(mats, (None, sel_ab), *([(None, sel_ba)] if both else []))
        ls = logit_scale.detach().reshape(1)
        losses = torch.zeros(len(dirs), dtype=torch.float32, device=dev)                   # the merge kernel adds the rows' terms
        ws = _empty((cl.ce_multipos_head_workspace_bytes(max(nq for _, nq, _, _ in dirs)),), torch.uint8, dev)
        stats = []
        for t, (iq, nq, _, sel) in enumerate(dirs):
            q, k = mats[iq], mats[1 - iq]
            stats.append(_empty((2, nq), torch.float32, dev))                              # lse | 1 / positives
            check(cl.ce_multipos_head_fwd(ptr(q), E, ptr(sel), nq, ptr(k), E, k.shape[0], E, ptr(ls), ptr(groups[iq]),
                                          ptr(groups[1 - iq]), ptr(stats[t][0]), ptr(stats[t][1]), ptr(losses[t:t + 1]), ptr(ws), s),
                  "ce_multipos_head_fwd")
        ctx.saved = (mats, invs, ls, groups, dirs, stats)
        return _head_result(losses)

    @staticmethod
    def backward(ctx, *gs):
        cl, s = lib(), stream()
        mats, invs, ls, groups, dirs, stats = ctx.saved
        E = mats[0].shape[1]
        g = _head_upstream(gs, mats[0].device)
        grads, scalars = _head_grad_buffers(mats)                                           # da^ | db^ | dlogit_scale
        for t, (iq, nq, _, sel) in enumerate(dirs):
            q, k = mats[iq], mats[1 - iq]
            check(cl.ce_multipos_head_bwd(ptr(q), E, ptr(sel), nq, ptr(k), E, k.shape[0], E, ptr(ls), ptr(groups[iq]),
                                          ptr(groups[1 - iq]), ptr(stats[t][0]), ptr(stats[t][1]), ptr(g[t:t + 1]), ptr(grads[iq]),
                                          ptr(grads[1 - iq]), ptr(scalars[0:1]), s), "ce_multipos_head_bwd")
        return (_l2norm_bwd(grads[0], mats[0], invs[0]), _l2norm_bwd(grads[1], mats[1], invs[1]), scalars[0].reshape(()),
                None, None, None, None, None)


def multipos_contrastive_losses(fi, ft, fi_all, ft_all, logit_scale, groups_per_image, groups_per_text, groups_per_image_all,
                                groups_per_text_all, index_pos):
    """``CriterionMultiPositive`` over the batch on raw features: loss_i = the local images against all texts, loss_t = the
    ``index_pos`` rows of the local texts against all images, the logits never materialised."""
    if fi_all is fi and ft_all is ft:          # one process: one node for both directions
        loss_i, loss_t = MultiPosHeadFn.apply(fi, ft, logit_scale, groups_per_image, groups_per_text, None, True, index_pos)
        return {"loss_i": loss_i, "loss_t": loss_t}
    return {"loss_i": MultiPosHeadFn.apply(fi, ft_all, logit_scale, groups_per_image, groups_per_text_all, None),
            "loss_t": MultiPosHeadFn.apply(ft, fi_all, logit_scale, groups_per_text, groups_per_image_all, index_pos)}


class SigmoidHeadFn(torch.autograd.Function):
    """The sigmoid pairwise loss of SigLIP, -(1/nq) sum_r sum_c log sigma(z (s q^_r . k^_c + b)) with z = +1 where c is the label
    of query r and -1 elsewhere, over the query rows ``sel_ab`` of ``a`` against all rows of ``b`` -- without the [nq, nk] logits
    matrix (``ce_sigmoid_head_fwd/bwd``: three sweeps, nothing saved but the normalised features); with ``labels_ba`` also over the
    rows ``sel_ba`` of ``b`` against all rows of ``a``.  Gradients for both raw feature matrices, ``logit_scale`` and
    ``logit_bias``.

    ``groups`` = (ids of the rows of ``a``, ids of the rows of ``b``): the multi-positive form.  z = +1 wherever the key's id equals
    the query's and is not negative (``ce_sigmoid_head_group_fwd/bwd``); ``labels_ab`` / ``labels_ba`` are then not read, and the
    second direction is asked for with ``labels_ba`` not None (any value) or ``sel_ba``."""

    @staticmethod
    def forward(ctx, a, b, logit_scale, logit_bias, labels_ab, sel_ab, labels_ba=None, sel_ba=None, groups=None):
        if groups is not None:
            return SigmoidHeadFn._forward_groups(ctx, a, b, logit_scale, logit_bias, sel_ab, labels_ba is not None or sel_ba is not None,
                                                 sel_ba, groups)
        ctx.groups = None
        cl, s = lib(), stream()
        dev = a.device
        mats, invs = _head_normalise(a, b)
        E = mats[0].shape[1]
        dirs = _head_directions(mats, (labels_ab, sel_ab), *([] if labels_ba is None else [(labels_ba, sel_ba)]))
        ls, lb = logit_scale.detach().reshape(1), logit_bias.detach().float().reshape(1)
        losses = _empty((len(dirs),), torch.float32, dev)
        for t, (iq, nq, labels, sel) in enumerate(dirs):
            q, k = mats[iq], mats[1 - iq]
            ws = _empty((cl.ce_sigmoid_head_workspace_bytes(nq, k.shape[0]),), torch.uint8, dev)
            check(cl.ce_sigmoid_head_fwd(ptr(q), E, ptr(sel), nq, ptr(k), E, k.shape[0], E, ptr(ls), ptr(lb), ptr(labels),
                                         ptr(losses[t:t + 1]), ptr(ws), s), "ce_sigmoid_head_fwd")
        ctx.saved = (mats, invs, ls, lb, dirs)
        return _head_result(losses)

    @staticmethod
    def _forward_groups(ctx, a, b, logit_scale, logit_bias, sel_ab, both, sel_ba, groups):
        cl, s = lib(), stream()
        dev = a.device
        mats, invs = _head_normalise(a, b)
        E = mats[0].shape[1]
        ctx.groups = (_index64(groups[0], dev), _index64(groups[1], dev))
        if ctx.groups[0].shape[0] != mats[0].shape[0] or ctx.groups[1].shape[0] != mats[1].shape[0]:
            raise RuntimeError(f"sigmoid head: {ctx.groups[0].shape[0]} / {ctx.groups[1].shape[0]} group ids for "
                               f"{mats[0].shape[0]} / {mats[1].shape[0]} feature rows")
        dirs = _head_directions(mats, (None, sel_ab), *([(None, sel_ba)] if both else []))
        ls, lb = logit_scale.detach().reshape(1), logit_bias.detach().float().reshape(1)
        losses = _empty((len(dirs),), torch.float32, dev)
        for t, (iq, nq, _, sel) in enumerate(dirs):
            q, k = mats[iq], mats[1 - iq]
            ws = _empty((cl.ce_sigmoid_head_workspace_bytes(nq, k.shape[0]),), torch.uint8, dev)
            check(cl.ce_sigmoid_head_group_fwd(ptr(q), E, ptr(sel), nq, ptr(k), E, k.shape[0], E, ptr(ls), ptr(lb),
                                               ptr(ctx.groups[iq]), ptr(ctx.groups[1 - iq]), ptr(losses[t:t + 1]), ptr(ws), s),
                  "ce_sigmoid_head_group_fwd")
        ctx.saved = (mats, invs, ls, lb, dirs)
        return _head_result(losses)

    @staticmethod
    def backward(ctx, *gs):
        cl, s = lib(), stream()
        mats, invs, ls, lb, dirs = ctx.saved
        E = mats[0].shape[1]
        g = _head_upstream(gs, mats[0].device)
        grads, scalars = _head_grad_buffers(mats)                                           # da^ | db^ | dscale, dbias
        for t, (iq, nq, labels, sel) in enumerate(dirs):
            q, k = mats[iq], mats[1 - iq]
            if ctx.groups is not None:
                check(cl.ce_sigmoid_head_group_bwd(ptr(q), E, ptr(sel), nq, ptr(k), E, k.shape[0], E, ptr(ls), ptr(lb),
                                                   ptr(ctx.groups[iq]), ptr(ctx.groups[1 - iq]), ptr(g[t:t + 1]), ptr(grads[iq]),
                                                   ptr(grads[1 - iq]), ptr(scalars[0:1]), ptr(scalars[1:2]), s),
                      "ce_sigmoid_head_group_bwd")
                continue
            check(cl.ce_sigmoid_head_bwd(ptr(q), E, ptr(sel), nq, ptr(k), E, k.shape[0], E, ptr(ls), ptr(lb), ptr(labels),
                                         ptr(g[t:t + 1]), ptr(grads[iq]), ptr(grads[1 - iq]), ptr(scalars[0:1]), ptr(scalars[1:2]), s),
                  "ce_sigmoid_head_bwd")
        return (_l2norm_bwd(grads[0], mats[0], invs[0]), _l2norm_bwd(grads[1], mats[1], invs[1]), scalars[0].reshape(()),
                scalars[1].reshape(()), None, None, None, None, None)


def sigmoid_contrastive_losses(fi, ft_all, logit_scale, logit_bias, labels_per_image, groups=None):
    """``CriterionSigmoid`` over the batch on raw features: the local images against all (gathered) texts, one direction.
    ``groups`` = (ids of the images, ids of all texts): ``CriterionSigmoid(multi_positive=True)``."""
    if groups is not None:
        return {"loss_sig": SigmoidHeadFn.apply(fi, ft_all, logit_scale, logit_bias, None, None, None, None, groups)}
    return {"loss_sig": SigmoidHeadFn.apply(fi, ft_all, logit_scale, logit_bias, labels_per_image, None)}


def _teacher_norm(t):
    """A teacher's features as the distillation head reads them: fp32, L2-normalised, no gradient."""
    return _l2norm(_f32(t.detach()))[0]


def _rowdot_sum(x, y, out):
    check(lib().ce_rowdot_sum(ptr(x), x.shape[1], ptr(y), y.shape[1], x.shape[0], x.shape[1], ptr(out), stream()), "ce_rowdot_sum")


def _check_teacher(what, s, t):
    if t.dim() != 2 or t.shape[0] != s.shape[0]:
        raise RuntimeError(f"distillation: teacher {what} features {tuple(t.shape)} do not match the student's {tuple(s.shape)} row for row")


class DistillHeadFn(torch.autograd.Function):
    """Distillation loss (open_clip's ``DistillClipLoss.dist_loss``),
    -(softmax(st ta^ tb^T) * log_softmax(s a^ b^T)).sum(1).mean() over the query rows ``sel_ab`` of ``a`` against all rows of ``b``,
    without either logits matrix (``ce_distill_head_fwd/bwd``).  ``ta`` / ``tb`` are the teacher's features for the same rows as
    ``a`` / ``b`` (any width the head takes) and ``teacher_logit_scale`` its log scale: constants.  ``both``: also the other
    direction on the same matrices, the rows ``sel_ba`` of ``b`` against all rows of ``a`` (one process); one direction is the form
    for keys gathered across ranks.  Gradients for ``a``, ``b`` and ``logit_scale``; the latter is sum_r <a^_r, da^_r>
    (``ce_rowdot_sum`` over the accumulated gradient buffer this node owns: the queries of one direction, the keys of the other)."""

    @staticmethod
    def forward(ctx, a, b, logit_scale, ta, tb, teacher_logit_scale, sel_ab, both=False, sel_ba=None):
        cl, s = lib(), stream()
        dev = a.device
        _check_teacher("first", a, ta)
        _check_teacher("second", b, tb)
        mats, invs = _head_normalise(a, b)
        tmats = (_teacher_norm(ta), _teacher_norm(tb))
        Es, Et = mats[0].shape[1], tmats[0].shape[1]
        dirs = _head_directions(mats, (None, sel_ab), *([(None, sel_ba)] if both else []))
        ls, tls = logit_scale.detach().reshape(1), teacher_logit_scale.detach().float().reshape(1).to(dev)
        losses = _empty((len(dirs),), torch.float32, dev)
        ws = _empty((cl.ce_distill_head_workspace_bytes(max(nq for _, nq, _, _ in dirs)),), torch.uint8, dev)
        kept = []
        for t, (iq, nq, _, sel) in enumerate(dirs):
            q, k, tq, tk = mats[iq], mats[1 - iq], tmats[iq], tmats[1 - iq]
            stats = _empty((2, nq, 2), torch.float32, dev)                                 # lse_s | lse_t, each (max, log sum) per row
            v = torch.zeros((nq, Es), dtype=torch.float32, device=dev)                     # an accumulation target
            check(cl.ce_distill_head_fwd(ptr(q), Es, ptr(sel), nq, ptr(k), Es, k.shape[0], Es, ptr(ls), ptr(tq), Et, ptr(tk), Et, Et,
                                         ptr(tls), ptr(stats[0]), ptr(stats[1]), ptr(v), ptr(losses[t:t + 1]), ptr(ws), s),
                  "ce_distill_head_fwd")
            kept.append((stats, v))
        ctx.saved = (mats, invs, tmats, ls, tls, dirs, kept)
        return _head_result(losses)

    @staticmethod
    def backward(ctx, *gs):
        cl, s = lib(), stream()
        mats, invs, tmats, ls, tls, dirs, kept = ctx.saved
        Es, Et = mats[0].shape[1], tmats[0].shape[1]
        g = _head_upstream(gs, mats[0].device)
        grads, scalars = _head_grad_buffers(mats)                                           # da^ | db^ | dlogit_scale
        for t, (iq, nq, _, sel) in enumerate(dirs):
            q, k, tq, tk = mats[iq], mats[1 - iq], tmats[iq], tmats[1 - iq]
            stats, v = kept[t]
            check(cl.ce_distill_head_bwd(ptr(q), Es, ptr(sel), nq, ptr(k), Es, k.shape[0], Es, ptr(ls), ptr(tq), Et, ptr(tk), Et, Et,
                                         ptr(tls), ptr(stats[0]), ptr(stats[1]), ptr(v), ptr(g[t:t + 1]), ptr(grads[iq]),
                                         ptr(grads[1 - iq]), s), "ce_distill_head_bwd")
        _rowdot_sum(mats[0], grads[0], scalars)
        return (_l2norm_bwd(grads[0], mats[0], invs[0]), _l2norm_bwd(grads[1], mats[1], invs[1]), scalars[0].reshape(()),
                None, None, None, None, None, None)


def distill_losses(fi, ft, fi_all, ft_all, logit_scale, tfi, tft, tfi_all, tft_all, teacher_logit_scale, index_pos):
    """The two distillation terms on raw features, the logits never materialised: the local images against all texts and the
    ``index_pos`` rows of the local texts against all images, student and teacher alike."""
    if fi_all is fi and ft_all is ft:          # one process: one node for both directions
        li, lt = DistillHeadFn.apply(fi, ft, logit_scale, tfi, tft, teacher_logit_scale, None, True, index_pos)
        return {"loss_dist_i": li, "loss_dist_t": lt}
    return {"loss_dist_i": DistillHeadFn.apply(fi, ft_all, logit_scale, tfi, tft_all, teacher_logit_scale, None),
            "loss_dist_t": DistillHeadFn.apply(ft, fi_all, logit_scale, tft, tfi_all, teacher_logit_scale, index_pos)}
