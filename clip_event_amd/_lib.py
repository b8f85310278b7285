"""ctypes binding of libclip_event_hip.so (the C ABI in include/clip_event_hip.h).

The product path has no CPU fallback: if the library is missing, or a call fails, this
raises.  Tensors are passed as raw device pointers (`tensor.data_ptr()`), the stream as
`torch.cuda.current_stream().cuda_stream`.
"""
from __future__ import annotations

import ctypes
import os
import re
from ctypes import c_char_p, c_void_p

import torch

from .build import HEADER

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libclip_event_hip.so")
_lib = None

(EPI_BF16, EPI_F32, EPI_BIAS_BF16, EPI_BIAS_F32, EPI_BIAS_RESID_F32, EPI_BIAS_GELU, EPI_GELUGRAD_BF16, EPI_BIAS_RESID_F16,
 EPI_BIAS_QGELU_BF16) = range(9)
T_F32, T_BF16, T_F16 = 0, 1, 2          # element types of stream operands (CE_T_* of include/clip_event_hip.h)


class HipExtensionMissing(RuntimeError):
    pass


class QuantJob(ctypes.Structure):
    """``ce_quant_job`` of include/clip_event_hip.h."""
    _fields_ = [("src", c_void_p), ("dst", c_void_p), ("scale", c_void_p), ("lds_", ctypes.c_long), ("ldd", ctypes.c_long),
                ("rows", ctypes.c_int), ("cols", ctypes.c_int), ("group_start", ctypes.c_int), ("pad_", ctypes.c_int)]


class TransposeJob(ctypes.Structure):
    """``ce_transpose_job`` of include/clip_event_hip.h."""
    _fields_ = [("src", c_void_p), ("dst", c_void_p), ("rows", ctypes.c_int), ("cols", ctypes.c_int),
                ("tile_start", ctypes.c_int), ("pad_", ctypes.c_int)]


class LoraJob(ctypes.Structure):
    """``ce_lora_job`` of include/clip_event_hip.h."""
    _fields_ = ([(n, c_void_p) for n in ("w0", "w16", "wt", "a", "b", "gw", "ga", "gb")] +
                [("rows", ctypes.c_int), ("cols", ctypes.c_int), ("rank", ctypes.c_int), ("scale", ctypes.c_float),
                 ("tile_start", ctypes.c_int), ("strip_start", ctypes.c_int), ("ws_start", ctypes.c_long)])


def lora_job_table(specs):
    """``(host array, tiles, strips)`` of ``ce_lora_job``s from ``specs`` = [(w0, w16, wt, a, b, gw, ga, gb, rows, cols, rank, scale)]
    (addresses as integers, ``wt`` may be 0 / None) with the running ``tile_start`` / ``strip_start`` / ``ws_start`` filled in."""
    jobs = (LoraJob * len(specs))()
    tiles = strips = ws = 0
    for job, (w0, w16, wt, a, b, gw, ga, gb, rows, cols, rank, scale) in zip(jobs, specs):
        job.w0, job.w16, job.wt, job.a, job.b, job.gw, job.ga, job.gb = w0, w16, wt or None, a, b, gw, ga, gb
        job.rows, job.cols, job.rank, job.scale = rows, cols, rank, scale
        job.tile_start, job.strip_start, job.ws_start = tiles, strips, ws
        n = (rows + 63) // 64
        tiles += n * ((cols + 63) // 64)
        strips += n
        ws += n * rank * cols
    return jobs, tiles, strips


class NTPlan(ctypes.Structure):
    """``ce_nt_plan`` of include/clip_event_hip.h; ``kernel`` indexes ``NT_KERNELS``."""
    _fields_ = [(name, ctypes.c_int) for name in ("kernel", "tm", "ts", "tall_panels", "tiles_m", "tiles_n", "tile_chunk",
                                                   "workgroups", "block", "lds_bytes", "wants_tile_queue", "taken")]


NT_KERNELS = ("NT128", "NT256x2", "NT256x4", "NT32", "NT160_RING", "LW", "PERSIST", "SKINNY")


def gemm_nt_plan(M: int, N: int, K: int, epilogue: int, fp8: bool = False, *, lda=None, ldb=None, ldo=None, ldo2=None,
                 ldaux=None, ldr=None) -> NTPlan:
    """The launch ``ce_gemm_nt`` (``fp8``: the loader-wave path of ``ce_gemm_nt_fp8``) would make under the process's current
    knobs (``ce_gemm_nt_plan``: host arithmetic, no GPU).  Leading dimensions default to those of contiguous operands; an
    operand the epilogue does not have has 0."""
    has_out2 = epilogue in (EPI_BIAS_GELU, EPI_GELUGRAD_BF16)
    has_resid = epilogue in (EPI_BIAS_RESID_F32, EPI_BIAS_RESID_F16)
    lds = [K if lda is None else lda, K if ldb is None else ldb, N if ldo is None else ldo,
           (N if has_out2 else 0) if ldo2 is None else ldo2, (N if epilogue == EPI_GELUGRAD_BF16 else 0) if ldaux is None else ldaux,
           (N if has_resid else 0) if ldr is None else ldr]
    plan = NTPlan()
    check(lib().ce_gemm_nt_plan(M, N, K, epilogue, int(fp8), *lds, ctypes.byref(plan)), "ce_gemm_nt_plan")
    return plan


TN_MAX_GROUP = 36                       # CE_TN_MAX_GROUP
TN_FORMS = ("v1", "v2", "v3", "v3")     # ce_tn_plan.form -> the policy's name for it
_TN_KERNELS = ("gemm_tn_kernel", "gemm_tn2_kernel", "gemm_tn3_kernel<{rows},{stages}>", "gemm_tn3lw_kernel<{rows},{stages}>")


class TNKnobs(ctypes.Structure):
    """``ce_tn_knobs`` of include/clip_event_hip.h: the weight-gradient GEMM's environment switches as values."""
    _fields_ = [(name, ctypes.c_int) for name in ("variant", "force_splits", "depth", "rows", "loader_waves")]

    def __init__(self, variant=3, force_splits=0, depth=3, rows=48, loader_waves=1):
        super().__init__(variant, force_splits, depth, rows, loader_waves)


class TNPlan(ctypes.Structure):
    """``ce_tn_plan`` of include/clip_event_hip.h; ``form`` indexes ``TN_FORMS``."""
    _fields_ = ([(name, ctypes.c_int) for name in ("form", "rows", "stages", "block", "lds_bytes", "workgroups", "splits",
                                                    "m_per_split", "depth", "kernel_overwrites", "zero_fill_first", "tiles",
                                                    "prof_class")] +
                [(name, ctypes.c_int * TN_MAX_GROUP) for name in ("tiles_n", "tiles_k", "tile_end")])

    @property
    def kernel(self) -> str:
        return _TN_KERNELS[self.form].format(rows=self.rows, stages=self.stages)


def gemm_tn_plan(shapes, M: int, splits: int = 0, overwrite: bool = False, knobs: TNKnobs = None) -> TNPlan:
    """The launch ``ce_gemm_tn_grouped_ex`` would make of the problems ``shapes`` = [(Nn, Kk), ...] under ``knobs`` (None:
    the process's, from the environment) -- ``ce_gemm_tn_plan``: host arithmetic, no GPU."""
    n = len(shapes)
    Nn, Kk = (ctypes.c_int * n)(*[s[0] for s in shapes]), (ctypes.c_int * n)(*[s[1] for s in shapes])
    plan = TNPlan()
    check(lib().ce_gemm_tn_plan(n, Nn, Kk, M, splits, int(overwrite), ctypes.byref(knobs) if knobs is not None else None,
                                ctypes.byref(plan)), "ce_gemm_tn_plan")
    return plan


def tower_wgrad_cuts(n_blocks: int, width: int, M: int, extra_tiles: int = 0, force_group: int = 0):
    """Blocks per grouped weight-gradient launch of ``ce_tower_backward``, top-down (``ce_tower_wgrad_cuts``; no GPU)."""
    sizes = (ctypes.c_int * max(n_blocks, 1))()
    groups = lib().ce_tower_wgrad_cuts(n_blocks, width, M, extra_tiles, force_group, sizes)
    if groups < 0:
        check(groups, "ce_tower_wgrad_cuts")
    return list(sizes[:groups])


_SCALARS = {"int": ctypes.c_int, "long": ctypes.c_long, "float": ctypes.c_float, "double": ctypes.c_double,
            "size_t": ctypes.c_size_t}
_DECL = re.compile(r"((?:\w+\s+)*\w+\s*\*?)\s*\b(ce_[a-z0-9_]+)\s*\(([^()]*)\)\s*;")


def signatures(header_text: str) -> dict:
    """{name: (restype, [argtypes])} of every function ``header_text`` (include/clip_event_hip.h) declares.  Scalars map to
    the ctypes scalar of the same name, every pointer to ``c_void_p``, a ``void`` return to None and a ``const char*`` return
    to ``c_char_p``; any other type raises and names the declaration."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", header_text, flags=re.S)
    text = "\n".join(line for line in text.split("\n") if not line.lstrip().startswith("#"))
    out = {}
    for ret, name, params in _DECL.findall(text):
        ret = " ".join(ret.replace("*", " * ").split())
        if ret not in _SCALARS and ret not in ("void", "const char *"):
            raise TypeError(f"{name}: return type '{ret}' has no ctypes mapping")
        restype = c_char_p if "*" in ret else _SCALARS.get(ret)
        argtypes = []
        for param in ([] if params.strip() in ("", "void") else params.split(",")):
            ctype = " ".join(w for w in param.split()[:-1] if w != "const")         # the last word is the parameter's name
            if "*" not in param and ctype not in _SCALARS:
                raise TypeError(f"{name}: parameter '{' '.join(param.split())}' has no ctypes mapping")
            argtypes.append(c_void_p if "*" in param else _SCALARS[ctype])
        out[name] = (restype, argtypes)
    return out


def lib() -> ctypes.CDLL:
    """Load the shared library once and give every function the header declares its ``restype`` / ``argtypes``: a wrong
    width or a wrong argument count then raises in Python, before the call.  Fails loudly when the library has not been
    built or the header is not where ``build.HEADER`` says."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise HipExtensionMissing(
                f"{LIB_PATH} not found: build it with `python -m clip_event_amd.build` "
                "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
        with open(HEADER) as f:
            declared = signatures(f.read())
        cdll = ctypes.CDLL(LIB_PATH)
        for name, (restype, argtypes) in declared.items():
            fn = getattr(cdll, name)
            fn.restype, fn.argtypes = restype, argtypes
        _lib = cdll
    return _lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        raise RuntimeError(f"{what} failed ({rc}): {lib().ce_last_error().decode()}")


def ptr(t) -> c_void_p:
    if t is None:
        return c_void_p(0)
    return c_void_p(t.data_ptr())


def stream() -> c_void_p:
    return c_void_p(torch.cuda.current_stream().cuda_stream)


_SAT = {}


def sat_counters(device) -> torch.Tensor:
    """The process-wide device buffer of the fp16-stream saturation counters (``ce_stream16_set_counters``): int32
    [forward stream, gradient stream].  One process drives one GPU, so one buffer, registered once and never freed (the
    library keeps the raw pointer)."""
    key = str(device)
    t = _SAT.get(key)
    if t is None:
        t = _SAT[key] = torch.zeros(2, dtype=torch.int32, device=device)
        check(lib().ce_stream16_set_counters(ptr(t)), "ce_stream16_set_counters")
    return t
