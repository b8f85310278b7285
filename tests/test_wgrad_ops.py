"""The block weight-gradient GEMM at the op level: ``ce_gemm_tn_grouped_ex`` (1..36 problems per launch, first-touch
overwrite or accumulate) and ``ce_gemm_tn_bias`` against an fp64 reference of the same bf16 operands, element by element
(tests/wgrad_cases.py states the bound), with guard rows / columns around every output, for every kernel form the launcher
can pick: the default policy here, the forms behind CE_GEMM_TN / CE_TN3_* in one child process per form."""
import json
import os
import subprocess
import sys

import pytest
import torch

from tests.wgrad_cases import CASES, SENTINEL, TN_ELEM_BOUND, TN_REL_L2, Problem, grouped_call, tn_check, tn_ok

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


def test_tn_checker_flags_corrupted_tiles():
    """CPU self-test of the checker: fp32 sums of the products in two different orders pass; a reference with one
    256 x 256 tile zeroed, doubled, transposed, taken from another problem, or with one M-split boundary (a 64-row
    contraction tile, or a single row) counted twice fails."""
    g = torch.Generator().manual_seed(3)
    M, Nn, Kk = 2049, 512, 768
    P = torch.randn(M, Nn, generator=g).to(torch.bfloat16).double()
    Q = torch.randn(M, Kk, generator=g).to(torch.bfloat16).double()
    Q2 = torch.randn(M, Kk, generator=g).to(torch.bfloat16).double()
    ref, mag = P.t() @ Q, P.abs().t() @ Q.abs()
    assert tn_ok(tn_check((P.float().t() @ Q.float()).double(), ref, mag))
    halves = (P[:1024].t() @ Q[:1024]).float().double() + (P[1024:].t() @ Q[1024:]).float().double()
    assert tn_ok(tn_check(halves, ref, mag))
    n, k = slice(256, 512), slice(256, 512)

    def corrupt(fn):
        bad = ref.clone()
        bad[n, k] = fn(bad[n, k].clone())
        return bad

    cases = {
        "zeroed": corrupt(lambda t: t * 0),
        "doubled": corrupt(lambda t: t * 2),
        "transposed": corrupt(lambda t: t.t()),
        "another problem's tile": corrupt(lambda t: (P.t() @ Q2)[n, k]),
        "64-row split boundary twice": corrupt(lambda t: t + P[1024:1088, n].t() @ Q[1024:1088, k]),
        "one boundary row twice": corrupt(lambda t: t + P[1024:1025, n].t() @ Q[1024:1025, k]),
    }
    for name, bad in cases.items():
        over, worst, rel = tn_check(bad, ref, mag)
        print(f"[checker] {name}: {over} elements over the bound, worst ratio {worst:.2e}, rel_l2 {rel:.2e}")
        assert over > 0 and not tn_ok((over, worst, rel)), name


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_grouped_wgrad_against_fp64(case):
    """One launch per (M, splits, overwrite): overwrite = 0 adds into a random base (checked as out - base), overwrite = 1
    writes into a NaN-poisoned output (every element must be written: plain stores from unsplit 256 x 256 tiles, zero-fill +
    atomics when the launch is split or runs on the 128 x 128 kernel).  The profiler's kernel class must be the one the
    launch policy promises: 256 x 256 for all-multiples-of-256 groups with M >= 2048, 128 x 128 otherwise."""
    from tests.wgrad_cases import run_case
    recs = run_case(case)
    bad = [r for r in recs if not r["ok"]]
    assert not bad, bad[:4]


@pytest.mark.gpu
@pytest.mark.parametrize("M,Nn,Kk,wide", [(2048, 768, 768, True), (10837, 3072, 768, False), (12800, 768, 3072, True),
                                          (63, 520, 264, True), (1, 8, 8, False), (2049, 136, 1032, False)])
def test_gemm_tn_bias_against_fp64(M, Nn, Kk, wide):
    """``ce_gemm_tn_bias``: dW += P^T Q (the checker's bound) and the bias gradient db += sum_m P[m, :], both into non-zero
    starting values; db within 2^-12 of sum_m |P[m, n]| + |start| (fp32 column sums) and 2e-5 relative L2; guards untouched."""
    from ctypes import c_int, c_long
    from clip_event_amd._lib import lib, ptr, stream
    gen = torch.Generator(device=DEV)
    gen.manual_seed(M + Nn + Kk)
    p = Problem(M, Nn, Kk, wide, gen, DEV)
    out = p.fresh_out(0)
    bias = torch.full((Nn + 8,), SENTINEL, device=DEV)
    bias_base = torch.randn(Nn, generator=gen, device=DEV) * M ** 0.5
    bias[:Nn] = bias_base
    rc = lib().ce_gemm_tn_bias(ptr(p.P), c_long(p.P.stride(0)), ptr(p.Q), c_long(p.Q.stride(0)), c_int(M), c_int(Nn), c_int(Kk),
                               ptr(out), c_long(p.ldo), ptr(bias), c_int(0), stream())
    torch.cuda.synchronize()
    assert rc == 0, lib().ce_last_error()
    res, guards = p.check(out, 0)
    print(f"[tn+bias {M}x{Nn}x{Kk} wide={wide}] dW: {res[0]} over, worst ratio {res[1]:.2e}, rel_l2 {res[2]:.2e}")
    assert tn_ok(res) and guards
    db = bias[:Nn].double() - bias_base.double()
    err = (db - p.colsum).abs()
    rel = float((db - p.colsum).norm() / p.colsum.norm())
    print(f"   db: worst ratio {float((err / p.colmag).max()):.2e}, rel_l2 {rel:.2e}")
    assert bool((err <= TN_ELEM_BOUND * (p.colmag + bias_base.double().abs())).all()) and rel < TN_REL_L2
    assert bool((bias[Nn:] == SENTINEL).all())


@pytest.mark.gpu
def test_grouped_wgrad_refuses_37_problems():
    """CE_TN_MAX_GROUP = 36: a 37-problem call (and an empty one) is refused with rc != 0 and writes nothing."""
    gen = torch.Generator(device=DEV)
    gen.manual_seed(37)
    probs = [Problem(2048, 256, 256, False, gen, DEV) for _ in range(37)]
    outs = [p.fresh_out(0) for p in probs]
    assert grouped_call(probs, outs, 2048, 0, 1) != 0
    assert grouped_call(probs, outs, 2048, 0, 1, count=0) != 0
    torch.cuda.synchronize()
    for p, o in zip(probs, outs):
        assert torch.equal(o[:256, :256], p.base) and bool((o[256:] == SENTINEL).all())


# ---------------------------------------------------------------------------------------------------------------
# environment forms: the launcher reads CE_GEMM_TN / CE_TN3_* once per process, so each form runs in a fresh child process
# (tests/wgrad_child.py, a reduced case table) under its own time limit, one at a time.  A child that ends by a signal or on
# its time limit stops the sequence: no further child is started.

ENV_FORMS = [{"CE_GEMM_TN": "1"}, {"CE_GEMM_TN": "2"}, {"CE_TN3_LW": "0"}, {"CE_TN3_ROWS": "32", "CE_TN3_LW": "1"},
             {"CE_TN3_ROWS": "32", "CE_TN3_LW": "0"}, {"CE_TN3_DEPTH": "1"}, {"CE_TN3_DEPTH": "2"}, {"CE_TN3_SPLITS": "5"}]
CHILD_TIMEOUT_S = 300
_stopped = []


def _form_id(env):
    return ",".join(f"{k}={v}" for k, v in env.items())


@pytest.mark.gpu
@pytest.mark.parametrize("form", ENV_FORMS, ids=[_form_id(e) for e in ENV_FORMS])
def test_grouped_wgrad_environment_form(form):
    if _stopped:
        pytest.fail(f"not started: the child of {_stopped[0]} ended by a signal or its time limit")
    env = {k: v for k, v in os.environ.items() if k != "CE_GEMM_TN" and not k.startswith("CE_TN3_")}
    env.update(form)
    try:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "wgrad_child.py")], env=env, cwd=ROOT,
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
    print(f"[{_form_id(form)}] {verdict['launches']} launches, kernels {verdict['kernels']}")
    for rec in verdict["failed"]:
        print("   FAILED", rec)
    assert r.returncode == 0 and verdict["ok"], verdict["failed"][:4]
