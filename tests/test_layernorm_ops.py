"""The LayerNorm family at the op level (csrc/layernorm.hip: ``ce_layernorm_fwd`` / ``_fwd_t`` / ``_fwd_q8`` / ``_bwd`` / ``_bwd_t`` /
``_bwd_q8`` / ``_bwd_partials`` / ``_fold``) against an fp64 reference of the same operand bits, element by element
(tests/ln_cases.py states the bounds), in dense, padded, gathered / scattered, in-place, no-dxb and no-dx_in layouts, with
sentinel guards around every output, NaN in every overwritten output and NaN behind every operand's edge, for every built type
combination and every LN_DISPATCH bucket, the row loop at default settings included; the forms behind CE_LN_FWD_RPW /
CE_LN_BWD_BLOCKS in one child process per form.  The relative-L2 tests of tests/test_hip_ops.py stay as the coarser layer."""
import json
import os
import subprocess
import sys

import pytest
import torch

from tests import ln_cases as C
from tests.ln_cases import (BWD8, CASES, FWD6, T_BF16, T_F16, T_F32, BwdLaunch, FwdLaunch, Values, passes)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
ORDERS = (("lanes", C.rowsum_lanes), ("serial", C.rowsum_serial))
CLASSES = (("plain", ("limit",)), ("offset", ()), ("mixed", ()), ("plain", ("sat",)))


# ---------------------------------------------------------------------------------------------------------------
# CPU: the checker against faithful emulations, a wrong algorithm and corrupted results

def _bf16_ulp_up(t):
    bits = t.contiguous().view(torch.int16)
    return torch.where(t >= 0, bits + 1, bits - 1).view(torch.bfloat16)


@pytest.mark.parametrize("D", [4, 260, 768, 2048])
def test_ln_checker_passes_faithful_emulations(D):
    """fp32 emulations of the forward and the backward in two summation orders (the kernels' lane order; plain serial), written
    into the guarded buffers of every layout, pass every check for every value class and every built type combination."""
    worst = {}
    for cls, special in CLASSES:
        v = Values(37, D, cls, seed=1, special=special)
        for oname, rowsum in ORDERS:
            for n, (xt, yt) in enumerate(FWD6):
                ln = FwdLaunch(v, C.FWD_LAYOUTS[n % 3], xt, yt, q8=yt == T_BF16, entry="q8").emulate(rowsum)
                res = ln.check()
                assert ln.guards_intact() and all(passes(r) for r in res.values()), (cls, oname, ln.describe(), res)
                key = ("fwd", cls, oname)
                worst[key] = max(worst.get(key, 0.0), max(r[1] for r in res.values()))
            for n, combo in enumerate(BWD8):
                layouts = [l for l in C.BWD_LAYOUTS if l != "inplace" or combo[2] == combo[3]]
                for layout in (layouts[n % len(layouts)], layouts[(n + 3) % len(layouts)]):
                    ln = BwdLaunch(v, layout, combo, gs=65536.0 if n % 2 == 0 else 1024.0, dxsum=True, q8=layout != "nodxb").emulate(rowsum)
                    res = ln.check()
                    assert ln.guards_intact() and all(passes(r) for r in res.values()), (cls, oname, ln.describe(), res)
                    key = ("bwd", cls, oname)
                    worst[key] = max(worst.get(key, 0.0), max(r[1] for k, r in res.items() if k == "dx"))
                    key = ("sums", cls, oname)
                    worst[key] = max(worst.get(key, 0.0), max(r[1] for k, r in res.items() if k in ("dgamma", "dbeta", "dxsum")))
    for (kind, cls, oname), w in sorted(worst.items()):
        print(f"[checker D={D}] {kind} {cls} {oname}: worst err / bound {w:.3f}")
    assert max(worst.values()) < 1.0


@pytest.mark.parametrize("D", [4, 260, 768, 2048])
def test_ln_offset_class_separates_one_pass_from_two_pass_variance(D):
    """Rows with mean 30 and spread 0.05: the bound on xhat stays below 0.05 on every such row (it still means something), the two-pass emulation
    passes in both orders, an fp32 one-pass variance E[x^2] - mu^2 is flagged."""
    v = Values(37, D, "offset", seed=2)
    f = v.fwd(T_F32)
    live = [r for r in range(37) if r not in (1, 2)]        # (the constant edge row, rstd = eps^-1/2 = 316: rstd d_mu = 0.073 around xhat = 0)
    assert float(f["dxh"][live].max()) < 0.05
    assert float(f["dxh"].max()) < 0.08
    for oname, rowsum in ORDERS:
        good = FwdLaunch(v, "dense", T_F32, T_F32).emulate(rowsum).check()
        assert all(passes(r) for r in good.values()), (oname, good)
        bad = FwdLaunch(v, "dense", T_F32, T_F32).emulate(rowsum, one_pass=True).check()
        print(f"[checker D={D} {oname}] two-pass y ratio {good['y'][1]:.3f}; one-pass: y {bad['y'][0]} over, ratio {bad['y'][1]:.1f}, "
              f"rstd {bad['rstd'][0]} over, ratio {bad['rstd'][1]:.1f}, rel_l2 {bad['y'][2]:.2e}")
        assert bad["y"][0] > 0 and bad["rstd"][0] > 0


def test_ln_checker_flags_corrupted_results():
    """Eleven corruptions of a faithful result each fail their check; the printout says which of them the relative-L2 limits of
    the older tests alone would have let through."""
    M, D, GS = 37, 768, 65536.0
    v = Values(M, D, "plain", seed=3)
    vs = Values(M, D, "plain", seed=3, special=("sat",))
    f = v.fwd(T_F32)
    x, w, b = v.x[T_F32], v.w, v.b
    mu, rs, y = C.emulate_fwd(x, w, b)
    results = {}

    def fwd(name, bad, yt=T_F32):
        if yt == T_F32:
            results[name] = C.check_abs(bad, f["y"], f["By"]) + (C.fwd_rel_limit(yt, f),)
        else:
            results[name] = C.check_rounded(bad, f["y"], f["By"], C.DT[yt]) + (C.fwd_rel_limit(yt, f),)

    bad = y.clone()
    bad[7, -4:] = y[6, -4:]
    fwd("the last 4 columns of a row taken from the row above", bad)
    bad = y.clone()
    bad[9] = (x[9] - mu[10]) * rs[9] * w + b
    fwd("one row normalised with the next row's mean", bad)
    fwd("every bf16 output one ulp up", _bf16_ulp_up(y.bfloat16()), T_BF16)
    bad = y.clone()
    bad[:, -4:] -= b[-4:]
    fwd("gamma applied but beta dropped in the last 4 columns", bad)
    _, rs_out, y_out = C.emulate_fwd(x, w, b, eps_outside=True)
    results["rstd computed with eps outside the square root"] = C.check_abs(rs_out, f["rstd"], f["rho"] * f["rstd"]) + (C.fwd_rel_limit(T_F32, f),)
    rel_y = float((y_out.double() - f["y"]).norm() / f["y"].norm())

    combo = (T_BF16, T_F32, T_F32, T_F32)
    r = v.bwd(*combo[:3], GS)
    mean, rstd = v.stats(T_F32)
    d, din = v.grad("dy", T_BF16, GS).float(), v.din32
    o, dw, db, dxs = C.emulate_bwd(d, x, mean, rstd, w, din)
    xh = (x - mean[:, None]) * rstd[:, None]
    bad = o.clone()
    bad[5] = o[5] - din[5]
    results["one row's dx without its dx_in"] = C.check_abs(bad, r["dx"], r["Bdx"]) + (C.REL_DX,)
    sums = lambda k, got: C.check_colsum(v.base[k] + got, v.base[k], *((r["tw"], r["dtw"]), (r["tb"], r["dtb"]), (r["dx"], r["Bdx"]))[k])
    assert passes(sums(0, dw) + (C.REL_DW,)) and passes(sums(2, dxs) + (C.REL_DXSUM,))
    results["dgamma missing the last row"] = sums(0, dw - d[-1] * xh[-1]) + (C.REL_DW,)
    results["dgamma counting one row twice"] = sums(0, dw + d[20] * xh[20]) + (C.REL_DW,)
    results["dxsum computed from dLN without dx_in"] = sums(2, dxs - din.sum(0)) + (C.REL_DXSUM,)

    combo16 = (T_BF16, T_F16, T_F16, T_F16)
    r16 = vs.bwd(*combo16[:3], GS)
    mean16, rstd16 = vs.stats(T_F16)
    o16 = C.emulate_bwd(vs.grad("dy", T_BF16, GS).float(), vs.x[T_F16], mean16, rstd16, w, vs.grad("din", T_F16, GS).float() / GS)[0]
    assert passes(C.check_rounded(C.store(o16, T_F16, GS), r16["dx"] * GS, r16["Bdx"] * GS, torch.float16) + (C.REL_DX16,))
    assert float((r16["dx"] * GS).abs().max()) > 65504.0
    results["an fp16 output not clamped"] = C.check_rounded((o16 * GS).half(), r16["dx"] * GS, r16["Bdx"] * GS, torch.float16) + (C.REL_DX16,)
    assert passes(C.check_rounded(o16.bfloat16(), r16["dx"], r16["Bdx"], torch.bfloat16) + (C.REL_DXB,))
    results["dxb rounded from the scaled instead of the true-unit value"] = \
        C.check_rounded((o16 * GS).bfloat16(), r16["dx"], r16["Bdx"], torch.bfloat16) + (C.REL_DXB,)

    assert len(results) == 11
    for name, (over, worst, rel, limit) in results.items():
        if name.startswith("rstd"):
            rel = rel_y             # (what the older tests look at: y)
        print(f"[checker] {name}: {over} elements flagged, rel_l2 {rel:.2e} "
              f"({'passes' if rel < limit else 'fails'} the older limit {limit:g})")
        assert over > 0, name


def test_ln_reference_is_finite_and_blind_to_the_poison():
    """The reference holds no NaN, and the NaN around the operands changes none of its values: recomputed from the slices of the
    poisoned buffers of every layout it is the same bits."""
    M, D = 5, 260
    v = Values(M, D, "plain", seed=4, special=("limit",))
    for xt in (T_F32, T_F16):
        f = v.fwd(xt)
        assert all(bool(t.isfinite().all()) for t in f.values() if isinstance(t, torch.Tensor))
        for layout in C.FWD_LAYOUTS:
            ln = FwdLaunch(v, layout, xt, T_BF16, q8=True, entry="q8")
            assert int(ln.x.buf.isnan().sum()) == ln.x.buf.numel() - M * D
            assert bool(ln.w[D:].isnan().all()) and bool(ln.b[D:].isnan().all()) and bool(ln.y.get(M=M).isnan().all())
            again = C.fwd_reference(ln.x.get(ln.rows, M), ln.w[:D], ln.b[:D])
            assert torch.equal(again["y"], f["y"]) and torch.equal(again["By"], f["By"]) and torch.equal(again["mu"], f["mu"])
    for combo in BWD8:
        dyt, xt, dit, dot = combo
        r = v.bwd(dyt, xt, dit, 65536.0)
        assert all(bool(t.isfinite().all()) for t in r.values())
        for layout in ("dense", "wide", "rows"):
            ln = BwdLaunch(v, layout, combo)
            idx = ln._idx()
            for m in (ln.dy, ln.x, ln.din):
                assert int(m.buf.isnan().sum()) == m.buf.numel() - M * D
            assert bool(ln.w[D:].isnan().all()) and bool(ln.mean[M:].isnan().all()) and bool(ln.rstd[M:].isnan().all())
            un = lambda m, t, i=None: m.get(i, M).double() / (65536.0 if t == T_F16 else 1.0)
            again = C.bwd_reference(un(ln.dy, dyt), ln.x.get(idx), ln.mean[:M], ln.rstd[:M], ln.w[:D], un(ln.din, dit, idx))
            assert torch.equal(again["dx"], r["dx"]) and torch.equal(again["Bdx"], r["Bdx"]) and torch.equal(again["tw"], r["tw"])


def test_ln_case_table_covers_what_it_claims():
    """Every LN_DISPATCH bucket at its ragged start and exact end, every NW with a loop case M = 2 * 256 * NW + 5, all six forward
    and all eight backward type combinations with / without dxsum in both forms at D = 768 and a ragged D, every backward layout."""
    ds = {c.D for c in CASES}
    assert {4, 64, 256, 260, 512, 516, 768, 1000, 1024, 1028, 2048} <= ds and {1, 3, 5, 37} <= {c.M for c in CASES}
    for M, D in ((8197, 256), (4101, 768), (2053, 1028)):
        assert M == 2 * 256 * C.form_of(D)[1] + 5 and any(c.M == M and c.D == D and c.bwd for c in CASES)
    for D in (768, 260):
        specs = [s for c in CASES if c.D == D for s in c.bwd]
        for combo in BWD8:
            for dxsum in (True, False):
                for form in ("atomic", "partials"):
                    assert any(s["combo"] == combo and s["dxsum"] == dxsum and s["form"] == form for s in specs), (D, combo, dxsum, form)
        assert {(xt, yt) for c in CASES if c.D == D for _, xt, yt, _, _ in c.fwd} == set(FWD6)
        assert {1024.0, 65536.0} <= {s["gs"] for s in specs}
    for D in ds:
        specs = [s for c in CASES if c.D == D for s in c.bwd]
        assert {s["layout"] for s in specs if s["combo"] in C.TOWER_BWD} >= {"dense", "inplace"}, D
    assert {s["layout"] for c in CASES for s in c.bwd} == set(C.BWD_LAYOUTS)
    assert any(s["q8"] for c in CASES for s in c.bwd) and any(q for c in CASES for _, _, _, q, _ in c.fwd)
    assert {e for c in CASES for _, _, _, _, e in c.fwd} == {"t", "q8", "plain"}


# ---------------------------------------------------------------------------------------------------------------
# GPU

@pytest.fixture(scope="module")
def lib():
    from clip_event_amd import _lib as L, build
    build.build()
    return L.lib()


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_ln_against_fp64(lib, case):
    """Every forward and backward launch of the row: zero elements over their bounds, guards intact, no NaN in any output, the
    saturation counters as the values demand."""
    recs = C.run_case(case)
    bad = [r for r in recs if not r["ok"]]
    worst = {}
    for r in recs:
        for k, w in r["worst"].items():
            key = (r["form"].split()[0], k)
            worst[key] = max(worst.get(key, 0.0), w)
    print(f"[ln {case.name}] {len(recs)} launches, worst err / bound: " + ", ".join(f"{a} {k} {w:.3f}" for (a, k), w in sorted(worst.items())))
    assert recs and not bad, bad[:4]


@pytest.mark.gpu
def test_ln_fold_of_65_jobs(lib):
    """One fold call of 65 jobs (two chunks of CE_LN_FOLD_MAX) mixing D = 4, 260, 768 and blocks = 1, 3, 7, each into its own
    non-zero destinations with 8 guard floats behind; jobs with a null dxsum leave theirs bit-identical."""
    assert C.FOLD_MAX == 64
    rc, recs = C.run_fold(DEV, 65)
    bad = [r for r in recs if not r["ok"]]
    print(f"[ln fold] 65 jobs, worst err / bound {max(r['worst'] for r in recs):.3f}")
    assert rc == 0 and len(recs) == 65 and not bad, (rc, bad[:4])
    assert any(r["null_dxsum"] for r in recs) and {r["blocks"] for r in recs} == {1, 3, 7} and {r["D"] for r in recs} == {4, 260, 768}


FWD_REFUSALS = [("D = 2052", dict(D=2052)), ("D = 6", dict(D=6)), ("M = 0", dict(M=0)), ("ldx % 4", dict(ldx=66)), ("ldy % 4", dict(ldy=66)),
                ("q8 with an fp32 y", dict(y_type=T_F32)), ("q8 without scales", dict(qscale=0)), ("ldq % 4", dict(ldq=66)),
                ("bf16 x is not built", dict(x_type=T_BF16))]
BWD_REFUSALS = [("D = 2052", dict(D=2052)), ("D = 6", dict(D=6)), ("M = 0", dict(M=0)), ("lddy % 4", dict(lddy=66)), ("ldx % 4", dict(ldx=66)),
                ("lddx % 4", dict(lddx=66)), ("lddxb % 4", dict(lddxb=66)), ("q8 without dxb", dict(dxb=0)), ("q8 without scales", dict(qscale=0)),
                ("an fp16 gradient operand without gscale", dict(gscale=0)), ("bf16 dx_out is not built", dict(dx_type=T_BF16)),
                ("fp32 dy on an fp16 x is not built", dict(dy_type=T_F32))]


@pytest.mark.gpu
def test_ln_refusals_write_nothing(lib):
    """Each refused call returns non-zero, names the family in ce_last_error and writes nothing (host argument checks: no launch)."""
    v = Values(5, 64, "plain", seed=5, dev=DEV)
    for what, override in FWD_REFUSALS:
        ln = FwdLaunch(v, "dense", T_F32, T_BF16, q8=True, entry="q8")
        rc = ln.call(**override)
        torch.cuda.synchronize()
        assert rc != 0 and b"ce_layernorm" in lib.ce_last_error() and ln.untouched(), ("fwd", what, rc, lib.ce_last_error())
    for form in ("atomic", "partials"):
        for what, override in BWD_REFUSALS + ([("null partials", dict(partials=0))] if form == "partials" else []):
            ln = BwdLaunch(v, "dense", (T_BF16, T_F16, T_F16, T_F16), form=form, q8=True, entry="q8")
            rc = ln.call(**override)
            torch.cuda.synchronize()
            assert rc != 0 and b"ce_layernorm" in lib.ce_last_error() and ln.untouched(), (form, what, rc, lib.ce_last_error())
    # fold: a job without dgamma, and no jobs at all
    p, dst = torch.ones(2, 3, 64, device=DEV), torch.full((3, 64), 0.5, device=DEV)
    for job, n in ((C.Job(p.data_ptr(), None, dst[1].data_ptr(), dst[2].data_ptr(), 2, 64), 1),
                   (C.Job(p.data_ptr(), dst[0].data_ptr(), dst[1].data_ptr(), None, 0, 64), 1),
                   (C.Job(p.data_ptr(), dst[0].data_ptr(), dst[1].data_ptr(), None, 2, 64), 0)):
        from clip_event_amd._lib import stream
        rc = lib.ce_layernorm_fold((C.Job * 1)(job), n, stream())
        torch.cuda.synchronize()
        assert rc != 0 and b"ce_layernorm_fold" in lib.ce_last_error() and bool((dst == 0.5).all())


# ---------------------------------------------------------------------------------------------------------------
# environment forms: the launchers read CE_LN_FWD_RPW / CE_LN_BWD_BLOCKS once per process, so each form runs in a fresh child
# process (tests/ln_child.py, CHILD_CASES) under its own time limit, one at a time.  A child that ends by a signal or on its
# time limit stops the sequence: no further child is started.

ENV_FORMS = [{"CE_LN_FWD_RPW": "2"}, {"CE_LN_BWD_BLOCKS": "3"}, {"CE_LN_BWD_BLOCKS": "1"}]
CHILD_TIMEOUT_S = 240
_stopped = []


def _form_id(env):
    return ",".join(f"{k}={v}" for k, v in env.items())


@pytest.mark.gpu
@pytest.mark.parametrize("form", ENV_FORMS, ids=[_form_id(e) for e in ENV_FORMS])
def test_ln_environment_form(lib, form):
    if _stopped:
        pytest.fail(f"not started: the child of {_stopped[0]} ended by a signal or its time limit")
    env = {k: v for k, v in os.environ.items() if not k.startswith("CE_LN_")}
    env.update(form)
    try:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "ln_child.py")], env=env, cwd=ROOT,
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
    print(f"[{_form_id(form)}] {verdict['launches']} launches in {verdict['seconds']:.1f} s, blocks {verdict['blocks']}, "
          f"worst ratio {verdict['worst']:.3f}")
    for rec in verdict["failed"]:
        print("   FAILED", rec)
    assert verdict["env"] == form and verdict["blocks_ok"]
    if "CE_LN_BWD_BLOCKS" in form:
        assert set(verdict["blocks"].values()) <= {1, int(form["CE_LN_BWD_BLOCKS"])}
    assert r.returncode == 0 and verdict["ok"], verdict["failed"][:4]
