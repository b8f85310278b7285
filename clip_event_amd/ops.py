"""Op-level Python wrappers over the C ABI (used by the tower runner's tests and by the
loss-head / optimizer code).  Each wrapper only marshals pointers and sizes; all math runs in
the HIP library.  bf16 tensors are torch.bfloat16, residual/grad streams torch.float32 (or torch.float16 through the
``_t`` wrappers, model.stream16)."""
from __future__ import annotations

from typing import Optional

import torch

from . import _lib as L
from ._lib import check, lib, ptr, stream


def _rows(t: torch.Tensor) -> int:
    return t.shape[0]


def _nt_tail(epilogue, bias, resid, out, out2, ldo2, aux):
    """The arguments ``ce_gemm_nt``, ``ce_gemm_nt_fp8`` and ``ce_gemm_nt_mx8`` share, from ``epilogue`` on."""
    return (epilogue, ptr(bias), ptr(resid), resid.stride(0) if resid is not None else 0, ptr(out), out.stride(0), ptr(out2),
            ldo2, ptr(aux), aux.stride(0) if aux is not None else 0, stream())


def gemm_nt(a: torch.Tensor, b: torch.Tensor, epilogue: int, *, bias=None, resid=None, out=None, out2=None,
            aux=None, M: Optional[int] = None) -> torch.Tensor:
    """out[M,N] = a[M,K] @ b[N,K]^T with a fused epilogue (include/clip_event_hip.h)."""
    assert a.dtype == torch.bfloat16 and b.dtype == torch.bfloat16 and a.is_cuda and b.is_cuda
    M = a.shape[0] if M is None else M
    K = a.shape[1]
    N = b.shape[0]
    assert b.shape[1] == K
    f32_out = epilogue in (L.EPI_F32, L.EPI_BIAS_F32, L.EPI_BIAS_RESID_F32)
    if epilogue == L.EPI_BIAS_RESID_F16:
        assert resid is not None and resid.dtype == torch.float16
    if out is None:
        out = torch.empty(a.shape[0], N, device=a.device,
                          dtype=torch.float16 if epilogue == L.EPI_BIAS_RESID_F16 else (torch.float32 if f32_out else torch.bfloat16))
    if epilogue == L.EPI_BIAS_GELU and out2 is None:
        out2 = torch.empty_like(out)
    ldo2 = 0 if out2 is None else (N if out2.dim() == 1 else out2.stride(0))        # 1-D: GELUGRAD column sums
    check(lib().ce_gemm_nt(ptr(a), a.stride(0), ptr(b), b.stride(0), M, N, K,
                           *_nt_tail(epilogue, bias, resid, out, out2, ldo2, aux)), "ce_gemm_nt")
    return (out, out2) if epilogue == L.EPI_BIAS_GELU else out


def gemm_tn(p: torch.Tensor, q: torch.Tensor, out: torch.Tensor, splits: int = 0, M: Optional[int] = None,
            ldo: Optional[int] = None):
    """out[Nn,Kk] += p[M,Nn]^T @ q[M,Kk] (fp32 atomic accumulation); ``ldo``: the row pitch of ``out`` when it is not
    ``out.stride(0)`` (a 4-D convolution weight written as [Nn, Kk])."""
    assert p.dtype == torch.bfloat16 and q.dtype == torch.bfloat16 and out.dtype == torch.float32
    M = p.shape[0] if M is None else M
    check(lib().ce_gemm_tn(ptr(p), p.stride(0), ptr(q), q.stride(0), M, p.shape[1], q.shape[1], ptr(out),
                           out.stride(0) if ldo is None else ldo, splits, stream()), "ce_gemm_tn")
    return out


def layernorm_fwd(x: torch.Tensor, w, b, *, rows=None, out_f32=False, eps=1e-5, M=None):
    """y = LN(x[rows]) ; returns (y, mean, rstd)."""
    assert x.dtype == torch.float32
    M = (rows.shape[0] if rows is not None else x.shape[0]) if M is None else M
    D = x.shape[-1]
    y = torch.empty(M, D, device=x.device, dtype=torch.float32 if out_f32 else torch.bfloat16)
    mean = torch.empty(M, device=x.device, dtype=torch.float32)
    rstd = torch.empty(M, device=x.device, dtype=torch.float32)
    check(lib().ce_layernorm_fwd(ptr(x), x.stride(0), ptr(rows), ptr(w), ptr(b), ptr(y), y.stride(0),
                                 1 if out_f32 else 0, ptr(mean), ptr(rstd), M, D, eps,
                                 stream()), "ce_layernorm_fwd")
    return y, mean, rstd


def layernorm_bwd(dy, x, mean, rstd, w, dw, db, *, rows=None, dx_in=None, dx_out=None, dxb=None, dxsum=None):
    """dx_out = dx_in + LN'(dy); dxb = bf16(dx_out); dw += ..., db += ... (atomic)."""
    M = dy.shape[0]
    D = dy.shape[1]
    if dx_out is None:
        dx_out = torch.zeros_like(x) if rows is not None else torch.empty_like(x)
    check(lib().ce_layernorm_bwd(ptr(dy), dy.stride(0), 1 if dy.dtype == torch.float32 else 0, ptr(x),
                                 x.stride(0), ptr(rows), ptr(mean), ptr(rstd), ptr(w), ptr(dx_in), ptr(dx_out),
                                 dx_out.stride(0), ptr(dxb), dxb.stride(0) if dxb is not None else 0,
                                 ptr(dw), ptr(db), ptr(dxsum), M, D, stream()), "ce_layernorm_bwd")
    return dx_out


_TYPE = {torch.float32: L.T_F32, torch.bfloat16: L.T_BF16, torch.float16: L.T_F16}


def layernorm_fwd_t(x: torch.Tensor, w, b, out_dtype=torch.bfloat16, *, rows=None, eps=1e-5):
    """``layernorm_fwd`` with typed operands (ce_layernorm_fwd_t): x fp32 / fp16, y bf16 / fp32 / fp16."""
    M = rows.shape[0] if rows is not None else x.shape[0]
    D = x.shape[-1]
    y = torch.empty(M, D, device=x.device, dtype=out_dtype)
    mean = torch.empty(M, device=x.device, dtype=torch.float32)
    rstd = torch.empty(M, device=x.device, dtype=torch.float32)
    check(lib().ce_layernorm_fwd_t(ptr(x), _TYPE[x.dtype], x.stride(0), ptr(rows), ptr(w), ptr(b), ptr(y),
                                   _TYPE[out_dtype], y.stride(0), ptr(mean), ptr(rstd), M, D,
                                   eps, stream()), "ce_layernorm_fwd_t")
    return y, mean, rstd


def layernorm_bwd_t(dy, x, mean, rstd, w, dw, db, dx_out, *, gscale=None, rows=None, dx_in=None, dxb=None, dxsum=None):
    """``layernorm_bwd`` with typed operands (ce_layernorm_bwd_t); fp16 gradient operands hold gradient * gscale[0]
    (``gscale``: a 1-element fp32 DEVICE tensor, see ``grad_scale``)."""
    M, D = dy.shape
    check(lib().ce_layernorm_bwd_t(ptr(dy), _TYPE[dy.dtype], dy.stride(0), ptr(x), _TYPE[x.dtype],
                                   x.stride(0), ptr(rows), ptr(mean), ptr(rstd), ptr(w), ptr(dx_in),
                                   _TYPE[dx_in.dtype] if dx_in is not None else L.T_F32, ptr(dx_out),
                                   _TYPE[dx_out.dtype], dx_out.stride(0), ptr(dxb),
                                   dxb.stride(0) if dxb is not None else 0, ptr(dw), ptr(db), ptr(dxsum),
                                   ptr(gscale), M, D, stream()), "ce_layernorm_bwd_t")
    return dx_out


def grad_scale(x: torch.Tensor, target: float = 1024.0) -> torch.Tensor:
    """1-element device tensor: the power of two s with s * max|x| in (target / 2, target] (ce_grad_scale)."""
    assert x.dtype == torch.float32 and x.is_contiguous()
    buf = torch.empty(257, device=x.device, dtype=torch.float32)
    check(lib().ce_grad_scale(ptr(x), x.numel(), target, buf.data_ptr() + 4, ptr(buf), stream()),
          "ce_grad_scale")
    return buf[:1]


def cast_scaled(x: torch.Tensor, dtype, scale: torch.Tensor, divide: bool = False):
    y = torch.empty_like(x, dtype=dtype)
    check(lib().ce_cast_scaled(ptr(x), _TYPE[x.dtype], ptr(y), _TYPE[dtype], ptr(scale), 1 if divide else 0,
                               x.numel(), stream()), "ce_cast_scaled")
    return y


def cast_t(x: torch.Tensor, dtype, mul: float = 1.0):
    y = torch.empty_like(x, dtype=dtype)
    check(lib().ce_cast_t(ptr(x), _TYPE[x.dtype], ptr(y), _TYPE[dtype], mul, x.numel(), stream()),
          "ce_cast_t")
    return y


def attention_fwd(qkv: torch.Tensor, B: int, L: int, H: int, causal: bool, cu_seqlens=None):
    """o, lse = attention(qkv[B*L, 3*H*64]); ``cu_seqlens`` (int32 [B+1]) = packed variable-length batch."""
    assert qkv.dtype == torch.bfloat16
    o = torch.empty(qkv.shape[0], H * 64, device=qkv.device, dtype=torch.bfloat16)
    lse = torch.empty(B * H * L, device=qkv.device, dtype=torch.float32)
    check(lib().ce_attention_fwd(ptr(qkv), qkv.stride(0), ptr(o), o.stride(0), ptr(lse),
                                 ptr(cu_seqlens), B, L, H, 1 if causal else 0, stream()),
          "ce_attention_fwd")
    return o, lse


def attention_bwd(qkv, o, dout, lse, B: int, L: int, H: int, causal: bool, bias_grad=None, cu_seqlens=None):
    dqkv = torch.empty_like(qkv)
    check(lib().ce_attention_bwd(ptr(qkv), qkv.stride(0), ptr(o), o.stride(0), ptr(dout),
                                 dout.stride(0), ptr(lse), ptr(dqkv), dqkv.stride(0), ptr(bias_grad),
                                 ptr(cu_seqlens), B, L, H, 1 if causal else 0, stream()),
          "ce_attention_bwd")
    return dqkv


def probe_mfma(shape: int, a_frags: torch.Tensor, b_frags: torch.Tensor) -> torch.Tensor:
    out = torch.empty(64, 4 if shape == 16 else 16, device=a_frags.device, dtype=torch.float32)
    check(lib().ce_probe_mfma(shape, ptr(a_frags), ptr(b_frags), ptr(out), stream()), "ce_probe_mfma")
    return out


def probe_tr16(image: torch.Tensor, byte_off: torch.Tensor) -> torch.Tensor:
    out = torch.empty(64, 4, device=image.device, dtype=torch.int16)
    check(lib().ce_probe_tr16(ptr(image), image.numel(), ptr(byte_off), ptr(out), stream()), "ce_probe_tr16")
    return out


def quant_rows_fp8(x: torch.Tensor):
    """(q uint8 [M,K] of e4m3 bytes, scale f32 [M]) = per-row quantisation of a bf16 matrix (ce_quant_rows_fp8)."""
    assert x.dtype == torch.bfloat16 and x.is_cuda and x.stride(1) == 1
    M, K = x.shape
    q = torch.empty(M, K, dtype=torch.uint8, device=x.device)
    scale = torch.empty(M, dtype=torch.float32, device=x.device)
    check(lib().ce_quant_rows_fp8(ptr(x), x.stride(0), ptr(q), K, ptr(scale), M, K, stream()),
          "ce_quant_rows_fp8")
    return q, scale


def gemm_nt_fp8(a8, sa, b8, sb, epilogue: int, *, bias=None, resid=None, aux=None, colsum=None):
    """out[M,N] = sa[m] sb[n] (a8[M,K] @ b8[N,K]^T) with a fused epilogue (ce_gemm_nt_fp8)."""
    M, K = a8.shape
    N = b8.shape[0]
    f32_out = epilogue == L.EPI_BIAS_RESID_F32
    out = torch.empty(M, N, device=a8.device, dtype=torch.float32 if f32_out else torch.bfloat16)
    out2 = torch.empty_like(out) if epilogue == L.EPI_BIAS_GELU else colsum
    ldo2 = out2.stride(0) if epilogue == L.EPI_BIAS_GELU else 0
    check(lib().ce_gemm_nt_fp8(ptr(a8), a8.stride(0), ptr(sa), ptr(b8), b8.stride(0), ptr(sb), M, N, K,
                               *_nt_tail(epilogue, bias, resid, out, out2, ldo2, aux)), "ce_gemm_nt_fp8")
    return (out, out2) if epilogue == L.EPI_BIAS_GELU else out


def quant_mx_fp8(x: torch.Tensor):
    """(q uint8 [M,K] of e4m3 bytes, scale8 uint8 [M, K/32] of E8M0 bytes) = MX block quantisation of a bf16 matrix."""
    assert x.dtype == torch.bfloat16 and x.is_cuda and x.stride(1) == 1 and x.shape[1] % 32 == 0
    M, K = x.shape
    q = torch.empty(M, K, dtype=torch.uint8, device=x.device)
    s8 = torch.empty(M, K // 32, dtype=torch.uint8, device=x.device)
    check(lib().ce_quant_mx_fp8(ptr(x), x.stride(0), ptr(q), K, ptr(s8), K // 32, M, K, stream()),
          "ce_quant_mx_fp8")
    return q, s8


def gemm_nt_mx8(a8, sa8, b8, sb8, epilogue: int, *, bias=None, resid=None, aux=None, colsum=None):
    """out[M,N] = sum over 32-blocks of 2^(sa8-127) 2^(sb8-127) (a8 . b8) with a fused epilogue (ce_gemm_nt_mx8)."""
    M, K = a8.shape
    N = b8.shape[0]
    dt = torch.float32 if epilogue == L.EPI_BIAS_RESID_F32 else (torch.float16 if epilogue == L.EPI_BIAS_RESID_F16 else torch.bfloat16)
    out = torch.empty(M, N, device=a8.device, dtype=dt)
    out2 = torch.empty_like(out) if epilogue == L.EPI_BIAS_GELU else colsum
    ldo2 = out2.stride(0) if epilogue == L.EPI_BIAS_GELU else 0
    check(lib().ce_gemm_nt_mx8(ptr(a8), a8.stride(0), ptr(sa8), ptr(b8), b8.stride(0), ptr(sb8), M, N, K,
                               *_nt_tail(epilogue, bias, resid, out, out2, ldo2, aux)), "ce_gemm_nt_mx8")
    return (out, out2) if epilogue == L.EPI_BIAS_GELU else out


def score_topk(q: torch.Tensor, keys: torch.Tensor, k: int, logit_scale=None, target=None, splits: int = 0):
    """Best ``k`` keys of every query without the [nq, nk] matrix (``ce_score_topk``): ``(values [nq,k] f32, indices [nq,k]
    int64, lse [nq] f32, rank [nq] int64 or None)``.  ``q`` / ``keys`` are used as given (normalise them first);
    ``logit_scale`` a device scalar (the score is exp(logit_scale) <q, key>) or None; ``target`` int64 [nq] or None."""
    assert q.dtype == torch.float32 and keys.dtype == torch.float32 and q.is_cuda and keys.is_cuda
    assert q.dim() == 2 and keys.dim() == 2 and q.stride(1) == 1 and keys.stride(1) == 1 and q.shape[1] == keys.shape[1]
    nq, E = q.shape
    nk = keys.shape[0]
    if target is not None:
        assert target.dtype == torch.int64 and target.is_cuda and target.is_contiguous() and target.numel() == nq
    if logit_scale is not None:
        assert logit_scale.dtype == torch.float32 and logit_scale.is_cuda and logit_scale.numel() == 1
    cl = lib()
    nbytes = int(cl.ce_score_topk_workspace_bytes(nq, nk, k, splits))
    ws = torch.empty(max(nbytes, 4), dtype=torch.uint8, device=q.device)
    top_val = torch.empty(nq, max(k, 0), dtype=torch.float32, device=q.device)
    top_idx = torch.empty(nq, max(k, 0), dtype=torch.int64, device=q.device)
    lse = torch.empty(nq, dtype=torch.float32, device=q.device)
    rank = None if target is None else torch.empty(nq, dtype=torch.int64, device=q.device)
    check(cl.ce_score_topk(ptr(q), q.stride(0), nq, ptr(keys), keys.stride(0), nk, E,
                           ptr(logit_scale), ptr(target), k, splits, ptr(top_val), ptr(top_idx), ptr(lse), ptr(rank),
                           ptr(ws), stream()), "ce_score_topk")
    return top_val, top_idx, lse, rank
