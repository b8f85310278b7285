"""Grouped weight-gradient GEMM (``ce_gemm_tn_grouped_ex``, ``ce_gemm_tn_bias``) against an fp64 reference: the element-wise
checker, the operand / output layouts and the case table, shared by tests/test_wgrad_ops.py and the child process it starts
per environment form (tests/wgrad_child.py).

Checker.  The kernels add exact bf16 x bf16 products in fp32, so an element's error is a small multiple of
eps_fp32 * sum_m |P[m,n]| |Q[m,k]|, i.e. of (|P|^T |Q|)[n,k].  The bound is 2^-12 of that sum: 4096 x the fp32 unit
roundoff, so no summation order comes near it, while a tile that is skipped, doubled, transposed or handed the wrong problem
is off by about |ref| = 1.5 / sqrt(M) of it (>= 1.3e-2 for M <= 12800) and a 64-row contraction tile counted twice by about
8 / (0.64 M) of it (>= 1e-3).  On top of that the relative-L2 bound of the existing TN tests (2e-5)."""
import math
import os
from ctypes import c_double, c_int, c_long, c_void_p

import torch

TN_ELEM_BOUND = 2.0 ** -12
TN_REL_L2 = 2e-5
SENTINEL = -1.25e9          # guard value around every output (finite, exact in fp32, far from any result)
PROF_TN3, PROF_TN2 = 64, 71  # CE_PROF_GEMM_TN (256x256 kernels) / CE_PROF_GEMM_TN2 (128x128 kernels, v1 and v2)


def tn_check(got, ref, mag):
    """(elements over the bound, largest |got - ref| / mag, relative L2) for fp64 [Nn, Kk] tensors; NaN counts as over."""
    diff = got - ref
    err = diff.abs()
    over = int((~(err <= TN_ELEM_BOUND * mag)).sum())
    worst = float((err / mag.clamp_min(1e-300)).nan_to_num(float("inf")).max())
    rel = float(diff.norm() / ref.norm().clamp_min(1e-300))
    return over, worst, rel


def tn_ok(res):
    over, _, rel = res
    return over == 0 and rel < TN_REL_L2


def block(d):
    """(Nn, Kk) of one residual block's weight gradients in the tower's order: qkv, out-projection, c_fc, c_proj."""
    return [(3 * d, d), (d, d), (4 * d, d), (d, 4 * d)]


def alternate_wide(shapes):
    """Every second problem in the wide layout (see Problem)."""
    return [(n, k, i % 2 == 1) for i, (n, k) in enumerate(shapes)]


class Case:
    def __init__(self, name, shapes, Ms, splits, policy):
        self.name, self.shapes, self.Ms, self.splits, self.policy = name, alternate_wide(shapes), Ms, splits, policy


# policy = the kernel the default launcher must pick: "v3" (256x256 ring kernels: every problem a multiple of 256 both ways,
# M >= 2048) or "v2" (128x128 tiles).  splits "rows" = ceil(M / 64): one 64-row contraction tile per split, the last one
# holding M % 64 rows.
CASES = [
    Case("vitb_block", block(768), (2048, 2049, 10837, 12800), (0, 1, 3), "v3"),
    Case("vitb_block_row_splits", block(768), (2049,), ("rows",), "v3"),
    Case("eight_blocks_plus_qkv", block(768) * 8 + [(3 * 768, 768)], (2048,), (0, 3), "v3"),
    Case("thirty_six_problems", block(768) * 9, (2048,), (0,), "v3"),
    Case("text_width_512", block(512), (10837,), (0, 1), "v3"),
    Case("width_1024", block(1024), (2049,), (0, 3), "v3"),
    Case("width_1280", block(1280), (2048,), (0,), "v3"),            # 5 tiles per 1280 columns: odd tiles_n and tiles_k
    Case("single_tile_rows_or_cols", [(256, 4096), (4096, 256), (256, 256), (768, 256)], (2048, 12800), (0, 1, 3), "v3"),
    Case("short_M", block(768), (1, 63, 256), (0, 1, 3), "v2"),     # 256 rows: the pruned last block's Bn
    Case("short_M_row_splits", block(768), (65,), ("rows",), "v2"),
    Case("widths_not_multiples_of_128", [(520, 264), (72, 200), (8, 8), (136, 1032)], (63, 2048, 10837), (0, 1, 3), "v2"),
    Case("mixed_group_goes_to_v2", [(768, 768), (520, 264), (3072, 768)], (2049, 12800), (0, 3), "v2"),
]

# the environment forms run a smaller table each (one child process per form)
CHILD_CASES = [
    Case("vitb_block", block(768), (2049, 10837), (0, 3), "v3"),
    Case("vitb_block_row_splits", block(768), (2049,), ("rows",), "v3"),
    Case("width_1280", block(1280), (2048,), (0,), "v3"),
    Case("single_tile_rows_or_cols", [(256, 4096), (4096, 256), (256, 256), (768, 256)], (2048,), (0, 1), "v3"),
    Case("short_M", block(768), (63,), (0,), "v2"),
    Case("widths_not_multiples_of_128", [(520, 264), (72, 200), (8, 8)], (2048,), (0, 3), "v2"),
    Case("mixed_group_goes_to_v2", [(768, 768), (520, 264)], (2049,), (0,), "v2"),
]


class Problem:
    """One weight-gradient problem with its own random bf16 operands and fp64 reference.

    Dense layout: P [M, Nn], Q [M, Kk] contiguous, ldo = Kk.  Wide layout: P and Q are column slices of wider buffers
    (ldp = Nn + 24 at column 8, ldq = Kk + 40 at column 16) and ldo = Kk + 8.  Either way the output buffer has three rows
    more than Nn; every element outside [Nn, Kk] holds SENTINEL and must come back unchanged."""

    def __init__(self, M, Nn, Kk, wide, gen, dev):
        self.M, self.Nn, self.Kk, self.wide = M, Nn, Kk, wide
        pc, qc = (8, 16) if wide else (0, 0)
        ldp, ldq = (Nn + 24, Kk + 40) if wide else (Nn, Kk)
        self.ldo = Kk + 8 if wide else Kk
        # (one spare row behind a column slice: the 128x128 kernels' bounds-checked loads may reach `column offset` bytes
        # past the last row of the slice, which must still be inside the allocation)
        extra = 1 if wide else 0
        self.P = torch.randn(M + extra, ldp, generator=gen, device=dev).to(torch.bfloat16)[:M, pc:pc + Nn]
        self.Q = torch.randn(M + extra, ldq, generator=gen, device=dev).to(torch.bfloat16)[:M, qc:qc + Kk]
        Pd, Qd = self.P.double(), self.Q.double()
        self.ref = Pd.t() @ Qd
        self.mag = Pd.abs().t() @ Qd.abs()
        self.colsum, self.colmag = Pd.sum(0), Pd.abs().sum(0)
        del Pd, Qd
        self.base = torch.randn(Nn, Kk, generator=gen, device=dev) * math.sqrt(M)     # of the size of the product

    def fresh_out(self, overwrite):
        """Output buffer: SENTINEL guards, the [Nn, Kk] block NaN (overwrite: every element must be written) or the base."""
        out = torch.full((self.Nn + 3, self.ldo), SENTINEL, device=self.P.device)
        if overwrite:
            out[:self.Nn, :self.Kk] = float("nan")
        else:
            out[:self.Nn, :self.Kk] = self.base
        return out

    def check(self, out, overwrite):
        """Added into the base, the fp32 sums also round against the start value: the magnitude is then |P|^T|Q| + |base|
        (|base| ~ sqrt(M) is far below |P|^T|Q| ~ 0.64 M except for the shortest M)."""
        inner = out[:self.Nn, :self.Kk].double()
        if overwrite:
            res = tn_check(inner, self.ref, self.mag)
        else:
            base = self.base.double()
            res = tn_check(inner - base, self.ref, self.mag + base.abs())
        guards = bool((out[self.Nn:] == SENTINEL).all()) and bool((out[:self.Nn, self.Kk:] == SENTINEL).all())
        return res, guards


def _arr(ctype, vals):
    return (ctype * len(vals))(*vals)


def grouped_call(probs, outs, M, splits, overwrite, count=None):
    """ce_gemm_tn_grouped_ex over `probs`; returns the C return code."""
    from clip_event_amd._lib import lib, stream
    n = len(probs) if count is None else count
    return lib().ce_gemm_tn_grouped_ex(c_int(n), _arr(c_void_p, [p.P.data_ptr() for p in probs]),
                                       _arr(c_long, [p.P.stride(0) for p in probs]),
                                       _arr(c_void_p, [p.Q.data_ptr() for p in probs]),
                                       _arr(c_long, [p.Q.stride(0) for p in probs]), c_int(M),
                                       _arr(c_int, [p.Nn for p in probs]), _arr(c_int, [p.Kk for p in probs]),
                                       _arr(c_void_p, [o.data_ptr() for o in outs]), _arr(c_long, [p.ldo for p in probs]),
                                       c_int(splits), c_int(overwrite), stream())


def launched():
    """{profiler class: launches} of the TN kernel classes since the last call (the library's event profiler)."""
    from clip_event_amd._lib import lib
    cl = lib()
    n = cl.ce_profile_num_classes()
    buf = (c_double * (4 * n))()
    cl.ce_profile_collect(buf, c_int(n))
    return {c: int(buf[4 * c]) for c in (PROF_TN3, PROF_TN2) if buf[4 * c] > 0}


def ran_form(counts, plan):
    """The form that ran, from the profiler classes alone; v1 and v2 share a class, there the plan tells which."""
    from clip_event_amd._lib import TN_FORMS
    if counts.get(PROF_TN3):
        return "v3"
    if counts.get(PROF_TN2):
        return "v1" if TN_FORMS[plan.form] == "v1" else "v2"
    return "none"


def expected_form(policy):
    """The case table's policy, or the form CE_GEMM_TN forces.  Only the plain spellings "1" and "2" count here (the library
    parses with atoi, so "01" would force v1 there and fail the case here, not pass it)."""
    return {"1": "v1", "2": "v2"}.get(os.environ.get("CE_GEMM_TN", "").strip(), policy)


def run_case(case, seed=0, dev="cuda:0", log=print):
    """Every (M, splits, overwrite) of a case: one launch each, checked against fp64.  Returns one record per launch."""
    from clip_event_amd._lib import TN_FORMS, gemm_tn_plan, lib
    recs = []
    lib().ce_profile_enable(1)
    launched()
    try:
        for M in case.Ms:
            gen = torch.Generator(device=dev)
            gen.manual_seed(seed * 1000003 + M * 7 + len(case.shapes))
            probs = [Problem(M, n, k, w, gen, dev) for n, k, w in case.shapes]
            for sp in case.splits:
                splits = (M + 63) // 64 if sp == "rows" else sp
                for overwrite in (0, 1):
                    outs = [p.fresh_out(overwrite) for p in probs]
                    rc = grouped_call(probs, outs, M, splits, overwrite)
                    torch.cuda.synchronize()
                    plan = gemm_tn_plan([(p.Nn, p.Kk) for p in probs], M, splits, overwrite)      # under the process's knobs
                    form, kernel = ran_form(launched(), plan), plan.kernel
                    rec = dict(case=case.name, M=M, splits=splits, overwrite=overwrite, problems=len(probs), rc=rc, form=form,
                               kernel=kernel, workgroups=plan.workgroups, expect=expected_form(case.policy))
                    over, worst, rel, guards = 0, 0.0, 0.0, True
                    if rc == 0:
                        for p, o in zip(probs, outs):
                            (ov, wo, re_), g = p.check(o, overwrite)
                            over, worst, rel, guards = over + ov, max(worst, wo), max(rel, re_), guards and g
                    rec.update(over=over, worst=worst, rel=rel, guards=guards,
                               ok=(rc == 0 and over == 0 and rel < TN_REL_L2 and guards and
                                   form == rec["expect"] == TN_FORMS[plan.form]))
                    log(f"[tn {case.name} M={M} splits={splits} overwrite={overwrite}] {kernel} ({form}, want {rec['expect']}): "
                        f"{over} elements over 2^-12 |P|^T|Q|, worst ratio {worst:.2e}, rel_l2 {rel:.2e}, "
                        f"guards {'untouched' if guards else 'WRITTEN'}" + ("" if rc == 0 else f", rc {rc}"))
                    recs.append(rec)
                    del outs
            del probs
    finally:
        launched()
        lib().ce_profile_enable(0)
    return recs
