"""The NT GEMMs at the op level: ``ce_gemm_nt`` (bf16 operands), ``ce_gemm_nt_fp8`` (e4m3, per-row scales) and ``ce_gemm_nt_mx8``
(e4m3, E8M0 block scales) against an fp64 reference of the same operand bits, element by element (tests/nt_cases.py states
the bounds), in a dense and a padded layout, with sentinel guards around every output, NaN in every overwritten output and
NaN behind every operand's edge, for every kernel form the dispatch table of csrc/gemm.hip holds, at the smallest shapes that
reach each form; the forms behind CE_NT_* / CE_GEMM_CUS in one child process per form."""
import json
import math
import os
import re
import subprocess
import sys

import pytest
import torch

from tests import nt_cases as C
from tests.nt_cases import (BF16, BIAS_BF16, BIAS_F32, BIAS_GELU, BIAS_QGELU_BF16, BIAS_RESID_F16, BIAS_RESID_F32, F32,
                            GELUGRAD_BF16, CASES, REL_L2, Launch, Values)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


@pytest.fixture(scope="module")
def lib():
    from clip_event_amd import _lib as L, build
    build.build()
    return L.lib()


# ---------------------------------------------------------------------------------------------------------------
# CPU: the checker against faithful emulations and against corrupted results

def _bf16_ulp_up(t):
    """Every bf16 element one unit in the last place up (towards +inf)."""
    bits = t.contiguous().view(torch.int16)
    return torch.where(t >= 0, bits + 1, bits - 1).view(torch.bfloat16)


def _quick_gelu_both_f32(h):
    """fp32 emulation of the kernels' QuickGELU pair: exp2 of the scaled argument, then a reciprocal."""
    t = torch.exp2(h * (-1.702 * 1.4426950408889634))
    s = 1.0 / (1.0 + t)
    return s + 1.702 * h * s * (1.0 - s), h * s


def test_nt_checker_passes_faithful_results_and_flags_corrupted_ones():
    """fp32 products of the same operands in two summation orders, rounded to each output type, and an fp32 emulation of the
    QuickGELU epilogue pass every check.  Twelve corruptions each fail theirs; the printout shows which of them the relative-L2
    limits of the older tests (1e-5 fp32, 3e-3 bf16) let through."""
    M, N, K = 1100, 520, 192
    v = Values(M, N, K, special="clamp")
    a, b, bias = v.a.float(), v.b.float(), v.bias
    orders = [a @ b.t(), a[:, :96] @ b[:, :96].t() + a[:, 96:] @ b[:, 96:].t()]
    aux = v.aux.float()
    for acc in orders:
        assert C.passes(C.check_f32(acc, *v.x_and_B(F32)), REL_L2[F32])
        assert C.passes(C.check_f32(acc + bias + v.resid, *v.x_and_B(BIAS_RESID_F32)), REL_L2[BIAS_RESID_F32])
        assert C.passes(C.check_rounded(acc.bfloat16(), *v.x_and_B(BF16), torch.bfloat16), REL_L2[BF16])
        assert C.passes(C.check_rounded((acc + bias).bfloat16(), *v.x_and_B(BIAS_BF16), torch.bfloat16), REL_L2[BIAS_BF16])
        f16 = (acc + bias + v.resid16.float()).clamp(-65504.0, 65504.0).half()
        assert C.passes(C.check_rounded(f16, *v.x_and_B(BIAS_RESID_F16), torch.float16), REL_L2[BIAS_RESID_F16])
        x, B = v.x_and_B(GELUGRAD_BF16)
        assert C.passes(C.check_gelugrad((acc * aux).bfloat16(), x, B, v.aux.double()), REL_L2[GELUGRAD_BF16])
        sums = v.colbase + (acc * aux).sum(0)
        assert C.passes(C.check_colsum(sums, v.colbase, x, B, v.aux.double()), C.REL_L2_COLSUM)
        assert torch.equal(sums[8:16], v.colbase[8:16])
        der, act = _quick_gelu_both_f32(acc + bias)
        x, B = v.x_and_B(BIAS_GELU)
        rd, ra = C.check_gelu(der.bfloat16(), x, B, True), C.check_gelu(act.bfloat16(), x, B, False)
        print(f"[checker] fp32 QuickGELU emulation: derivative ratio {rd[1]:.3f}, activation ratio {ra[1]:.3f}")
        assert C.passes(rd, REL_L2[BIAS_GELU]) and C.passes(ra, REL_L2[BIAS_GELU])

    acc = orders[0]
    x, B = v.x_and_B(BIAS_BF16)
    good = acc + bias
    rows, cols = slice(96, 192), slice(256, 512)
    other = Values(M, N, K, seed=1)

    def tile(fn):
        bad = good.clone()
        bad[rows, cols] = fn()
        return bad.bfloat16()

    one = good.bfloat16()
    one[700, 300] = one[700, 300] + 5 * 2.0 ** (math.floor(math.log2(abs(float(one[700, 300])))) - 7)
    last_row = good.clone()
    last_row[-1] = last_row[-2]
    no_bias = good.clone()
    no_bias[:, -8:] = acc[:, -8:]
    sq = good.clone()
    sq[128:256, 256:384] = good[128:256, 256:384].t()
    bf16_cases = {
        "one element off by five bf16 ulps": one,
        "every element one bf16 ulp up": _bf16_ulp_up(good.bfloat16()),
        "a 96 x 256 tile without its last 64-wide K tile": tile(lambda: a[rows, :128] @ b[cols, :128].t() + bias[cols]),
        "a tile without one 16-wide k-step": tile(lambda: acc[rows, cols] - a[rows, 64:80] @ b[cols, 64:80].t() + bias[cols]),
        "the last row equal to the row before it": last_row.bfloat16(),
        "bias dropped in the last 8 columns": no_bias.bfloat16(),
        "a tile transposed": sq.bfloat16(),
        "a tile taken from another problem": tile(lambda: other.a.float()[rows] @ other.b.float()[cols].t() + bias[cols]),
    }
    results = {name: C.check_rounded(bad, x, B, torch.bfloat16) + (REL_L2[BIAS_BF16],) for name, bad in bf16_cases.items()}
    xg, Bg = v.x_and_B(GELUGRAD_BF16)
    prod = acc * aux
    results["column sums missing the last row"] = C.check_colsum(v.colbase + prod[:-1].sum(0), v.colbase, xg, Bg, v.aux.double()) + (C.REL_L2_COLSUM,)
    results["column sums counting one row twice"] = C.check_colsum(v.colbase + prod.sum(0) + prod[500], v.colbase, xg, Bg, v.aux.double()) + (C.REL_L2_COLSUM,)
    der, act = _quick_gelu_both_f32(good)
    xb, Bb = v.x_and_B(BIAS_GELU)
    results["a GELU derivative computed as the activation"] = C.check_gelu(act.bfloat16(), xb, Bb, True) + (REL_L2[BIAS_GELU],)
    x16, B16 = v.x_and_B(BIAS_RESID_F16)
    results["an fp16 output not clamped"] = C.check_rounded((good + v.resid16.float()).half(), x16, B16, torch.float16) + (REL_L2[BIAS_RESID_F16],)
    assert len(results) == 12
    for name, (over, worst, rel, limit) in results.items():
        print(f"[checker] {name}: {over} elements flagged, rel_l2 {rel:.2e} "
              f"({'passes' if rel < limit else 'fails'} the older limit {limit:g})")
        assert over > 0, name


def test_nt_reference_is_finite_and_blind_to_the_poison():
    """The reference holds no NaN, and the NaN around the operands changes none of its values: recomputed from the slices of the
    poisoned buffers of both layouts it is the same bits."""
    for kind, shape in (("bf16", (130, 136, 72)), ("e4m3", (130, 136, 128)), ("mx", (130, 136, 128))):
        v = Values(*shape, kind=kind, seed=2)
        M, N, K = shape
        for epi in range(9):
            x, B = v.x_and_B(epi)
            assert bool(x.isfinite().all()) and bool(B.isfinite().all()) and bool((B >= 0).all())
        for layout in ("dense", "wide"):
            ln = Launch(v, layout, BIAS_RESID_F32)
            A, Bm = ln.A[:M, ln.a_off:ln.a_off + K], ln.B[:N, ln.a_off:ln.a_off + K]
            if kind == "bf16":
                assert bool(ln.A.isnan().sum() == ln.A.numel() - M * K)
                Ad, Bd = A.double(), Bm.double()
            else:
                assert int((ln.A == 0x7F).sum()) >= ln.A.numel() - M * K
                Ad, Bd = C._e4m3_values(A.contiguous()), C._e4m3_values(Bm.contiguous())
            if kind == "mx":
                Ad = Ad * torch.exp2(ln.sa[:M].double() - 127).repeat_interleave(32, dim=1)
                Bd = Bd * torch.exp2(ln.sb[:N].double() - 127).repeat_interleave(32, dim=1)
            ref = Ad @ Bd.t()
            if kind == "e4m3":
                ref = ref * (ln.sa[:M].double()[:, None] * ln.sb[:N].double()[None, :])
                assert bool(ln.sa[M:].isnan().all()) and bool(ln.sb[N:].isnan().all())
            assert torch.equal(ref, v.ref)
            assert bool(ln.bias[N:].isnan().all()) and bool(ln.resid[M:].isnan().all()) and bool(ln.out[:M, :N].isnan().all())
            assert torch.equal(ln.resid[:M, :N], v.resid)


def _dispatch_table():
    """{(kernel, tm, ts)} of the bf16 and of the e4m3 switch in csrc/gemm.hip's dispatch()."""
    with open(os.path.join(ROOT, "clip_event_amd", "csrc", "gemm.hip")) as f:
        src = f.read()
    body = src[src.index("bool dispatch(const NTPlan& p"):src.index("#undef CE_NT_CASE")]
    f8_part, bf16_part = body.split("} else {")
    forms = []
    for part in (bf16_part, f8_part):
        plain = {(k, int(tm), 0) for k, tm in re.findall(r"CE_NT_CASE\(NT_(\w+), (\d),", part)}
        two = {(k, int(tm), int(ts)) for k, tm, ts in re.findall(r"CE_NT_CASE_IF\(two, NT_(\w+), (\d), (\d),", part)}
        forms.append(plain | two)
    return forms


def test_case_table_reaches_the_whole_dispatch_table(lib):
    """Every row's plan is the intended one (the planner, no GPU), and the (kernel, tm, ts) the table reaches are all of
    dispatch()'s cases, bf16 and e4m3, minus the named remainder (empty)."""
    reached = {False: set(), True: set()}
    nt8 = 0
    for case in CASES:
        if case.kind == "mx":
            continue
        with C.knobs(case):
            for layout in case.layouts:
                for epi in case.epis:
                    form, queue, _ = C.planned(case, epi, C.plan_lds(case.shape[1], case.shape[2], case.kind, layout, epi))
                    assert form == case.expected(epi) and queue == case.queue, (case.name, layout, C.EPI_NAMES[epi], form, queue)
                    if form == C.NT8:
                        nt8 += 1
                    else:
                        reached[case.kind == "e4m3"].add(form)
    bf16_table, f8_table = _dispatch_table()
    assert len(bf16_table) == 23 and len(f8_table) == 8
    assert reached[False] == bf16_table - C.UNREACHED_BF16, (bf16_table - reached[False], reached[False] - bf16_table)
    assert reached[True] == f8_table - C.UNREACHED_E4M3, (f8_table - reached[True], reached[True] - f8_table)
    assert nt8 > 0 and not C.UNREACHED_BF16 and not C.UNREACHED_E4M3
    # one row per kernel family runs every epilogue the family is built for: nine (bf16), seven (e4m3 and MX)
    for kernel in ("NT128", "SKINNY", "LW", "PERSIST", "NT256x4", "NT256x2", "NT32", "NT160_RING"):
        assert any(c.kind == "bf16" and c.expect[0] == kernel and c.epis == C.ALL9 for c in CASES), kernel
    for kind, kernel in (("e4m3", "LW"), ("e4m3", "PERSIST"), ("e4m3", "NT8"), ("mx", "NT8")):
        assert any(c.kind == kind and c.expect[0] == kernel and c.epis == C.SEVEN for c in CASES), (kind, kernel)


# ---------------------------------------------------------------------------------------------------------------
# GPU

@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[f"{c.kind}-{c.name}" for c in CASES])
def test_nt_against_fp64(case):
    """Every (layout, epilogue) launch of the row: zero elements over their bounds, guards intact, no NaN in any output, the
    planned kernel form under the profiler class it reports."""
    bad = [r for r in C.run_case(case) if not r["ok"]]
    assert not bad, bad[:4]


REFUSALS = [
    ("K % 8", BF16, dict(K=60)), ("N % 4", BF16, dict(N=62)), ("lda % 8", BF16, dict(lda=68)), ("ldb % 8", BF16, dict(ldb=68)),
    ("ldo % 4", BF16, dict(ldo=66)), ("lda < K", BF16, dict(lda=56)), ("ldb < K", BF16, dict(ldb=56)), ("ldo < N", BF16, dict(ldo=60)),
    ("no bias", BIAS_BF16, dict(bias=0)), ("no bias", BIAS_F32, dict(bias=0)), ("no resid", BIAS_RESID_F32, dict(resid=0)),
    ("no resid", BIAS_RESID_F16, dict(resid=0)), ("no out2", BIAS_GELU, dict(out2=0)), ("no aux", GELUGRAD_BF16, dict(aux=0)),
    ("no bias", BIAS_QGELU_BF16, dict(bias=0)), ("epilogue 9", BF16, dict(epi=9)),
]
REFUSALS_F8 = [
    ("K % 128", BF16, dict(K=64)), ("N % 8", BF16, dict(N=60)), ("lda % 16", BF16, dict(lda=136)), ("no sa", BF16, dict(sa=0)),
    ("no sb", BIAS_GELU, dict(sb=0)), ("F32 not built", F32, {}), ("BIAS_F32 not built", BIAS_F32, {}),
    ("no resid", BIAS_RESID_F32, dict(resid=0)), ("no aux", GELUGRAD_BF16, dict(aux=0)),
]


@pytest.mark.gpu
def test_nt_refusals_write_nothing():
    """Each refused call returns non-zero, leaves ce_last_error naming the entry point, and writes nothing: guards, the NaN
    block and the column-sum base come back as they were."""
    from clip_event_amd._lib import lib
    cl = lib()
    for kind, table, name in (("bf16", REFUSALS, b"ce_gemm_nt"), ("e4m3", REFUSALS_F8, b"ce_gemm_nt_fp8"),
                              ("mx", REFUSALS_F8, b"ce_gemm_nt_")):
        v = Values(64, 64, 64 if kind == "bf16" else 128, kind=kind, seed=3, dev=DEV)
        for what, epi, override in table:
            ln = Launch(v, "dense", epi)
            rc = ln.call(**override)
            torch.cuda.synchronize()
            err = cl.ce_last_error()
            assert rc != 0 and name in err, (kind, what, rc, err)
            assert ln.untouched(), (kind, what)
    # GELUGRAD column sums on the 128 x 128 kernel are a second launch that takes N % 8 == 0 only: refused before the first
    for shape in ((1, 4, 8), (130, 132, 72)):
        ln = Launch(Values(*shape, seed=3, dev=DEV), "dense", GELUGRAD_BF16)
        rc = ln.call()
        torch.cuda.synchronize()
        assert rc != 0 and b"ce_gemm_nt" in cl.ce_last_error() and ln.untouched(), (shape, rc, cl.ce_last_error())
    assert cl.ce_gemm_set_cu_budget(7) != 0 and b"ce_gemm_set_cu_budget" in cl.ce_last_error()
    assert cl.ce_gemm_set_cu_budget(0) == 0


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


@pytest.mark.gpu
def test_nt_persistent_tile_queue_on_a_side_stream():
    """Three consecutive persistent launches with the tile queue on a non-default stream (the queue ring is per stream)."""
    case = C.Case("side_stream", C.P192, ("PERSIST", 5, 2), budget=32, dynamic=1, queue=True)
    v = Values(*case.shape, seed=4, dev=DEV)
    side = torch.cuda.Stream()
    with C.knobs(case), torch.cuda.stream(side):
        assert C.planned(case, BIAS_GELU)[:2] == (case.expect, True)
        launches = [Launch(v, "wide", BIAS_GELU) for _ in range(3)]
        rcs = [ln.call() for ln in launches]
        side.synchronize()
        assert rcs == [0, 0, 0]
        for ln in launches:
            res = ln.check()
            assert ln.guards_intact() and all(C.passes(r[:3], r[3]) for r in res.values()), res
            assert torch.equal(_bits(ln.out), _bits(launches[0].out)) and torch.equal(_bits(ln.out2), _bits(launches[0].out2))
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("case", [c for c in CASES if c.epis in (C.ALL9, C.SEVEN)] +
                         [c for c in CASES if c.queue], ids=lambda c: f"{c.kind}-{c.name}")
def test_nt_same_launch_twice_gives_the_same_bits(case):
    """out and out2 of two identical launches are bit-identical, tile queue or not (the column sums are float atomics: exempt)."""
    v = Values(*case.shape, kind=case.kind, seed=5, dev=DEV)
    with C.knobs(case):
        for epi in (BIAS_GELU, BIAS_RESID_F32, GELUGRAD_BF16):
            no_sums = case.shape[1] % 8 != 0            # (the 128 x 128 kernel's column-sum pass takes N % 8 == 0 only)
            first, second = Launch(v, "wide", epi, out2_null=no_sums), Launch(v, "wide", epi, out2_null=no_sums)
            assert first.call() == 0 and second.call() == 0
            torch.cuda.synchronize()
            assert torch.equal(_bits(first.out), _bits(second.out)), C.EPI_NAMES[epi]
            if epi == BIAS_GELU:
                assert torch.equal(_bits(first.out2), _bits(second.out2))


# ---------------------------------------------------------------------------------------------------------------
# environment forms: the launcher reads CE_NT_* / CE_GEMM_CUS once per process, so each form runs in a fresh child process
# (tests/nt_child.py, a reduced case table) under its own time limit, one at a time.  A child that ends by a signal or on its
# time limit stops the sequence: no further child is started.

ENV_FORMS = [{"CE_NT_MIXED": "0"}, {"CE_NT_PGRID": "64"}, {"CE_NT_PGRID": "24", "CE_NT_CHUNK": "2"}, {"CE_NT_CHUNK": "-1"},
             {"CE_NT_CHUNK": "3"}, {"CE_NT_DYNAMIC": "1", "CE_GEMM_CUS": "32"}, {"CE_GEMM_CUS": "40"}]
CHILD_TIMEOUT_S = 300
_stopped = []


def _form_id(env):
    return ",".join(f"{k}={v}" for k, v in env.items())


@pytest.mark.gpu
@pytest.mark.parametrize("form", ENV_FORMS, ids=[_form_id(e) for e in ENV_FORMS])
def test_nt_environment_form(form):
    if _stopped:
        pytest.fail(f"not started: the child of {_stopped[0]} ended by a signal or its time limit")
    env = {k: v for k, v in os.environ.items() if k != "CE_GEMM_CUS" and not k.startswith("CE_NT_")}
    env.update(form)
    try:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "nt_child.py")], env=env, cwd=ROOT,
                           capture_output=True, text=True, timeout=CHILD_TIMEOUT_S)
    except subprocess.TimeoutExpired as e:
        _stopped.append(_form_id(form))
        pytest.fail(f"{_form_id(form)}: no verdict within {CHILD_TIMEOUT_S} s\n{(e.stderr or '')[-2000:] if isinstance(e.stderr, str) else ''}")
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
        _stopped.append(_form_id(form))
        pytest.fail(f"{_form_id(form)}: child ended with {r.returncode}\n{r.stderr[-3000:]}")
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert lines, f"{_form_id(form)}: no verdict (rc {r.returncode})\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}"
    verdict = json.loads(lines[-1])
    print(f"[{_form_id(form)}] {verdict['launches']} launches in {verdict['seconds']:.1f} s, forms {verdict['forms']}, "
          f"worst ratio {verdict['worst']:.3f}")
    for rec in verdict["failed"]:
        print("   FAILED", rec)
    assert r.returncode == 0 and verdict["ok"], verdict["failed"][:4]
