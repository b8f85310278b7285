"""The five attention kernels at the op level: ``ce_attention_fwd`` / ``ce_attention_bwd`` against an fp64 reference of the same
bf16 operands, element by element against the magnitude each element's rounding errors scale with, with an fp64 emulation of the
kernels' bf16 roundings as the noise floor (tests/attn_cases.py states reference, emulation and bounds), sentinel guards around
every operand and output, every short bucket edge, the long kernels in both block orders, packed batches with empty samples,
refusals, a side stream, and the forms behind CE_ATTN_NS_FWD / CE_ATTN_NS / CE_ATTN_NK / CE_ATTN_XCD in one child process each."""
import json
import os
import subprocess
import sys

import pytest
import torch

from tests import attn_cases as A
from tests.attn_cases import BITS_CASES, LONG_CASES, PACKED_CASES, SHORT_CASES, Case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


# ---------------------------------------------------------------------------------------------------------------
# CPU: the checker itself

def _ops(L, kind, heads=1, seed=5):
    q, k, v, do = A.make_inputs([L], heads, kind, seed + L)[0]
    return [t.double().permute(1, 0, 2) for t in (q, k, v, do)]


def test_emulation_passes_at_every_table_shape():
    """The emulated reference passes E (and, trivially, M and R) against the exact one at every (L, causal, input kind) of the
    case tables, and so does an fp32 evaluation of the emulation's formulas: another summation order, another faithful kernel."""
    worst = {name: 0.0 for name in A.OUTPUTS}
    worst32 = {name: [0.0, 0.0, 0.0] for name in A.OUTPUTS}
    for L, causal, kind in A.self_test_keys():
        ops = _ops(L, kind, heads=2)
        ex, em = A.exact(*ops, causal), A.emulate(*ops, causal)
        em32 = {n: t.double() for n, t in A.emulate(*ops, causal, dtype=torch.float32).items()}
        for rec, rec32 in zip(A.check_all(em, ex, em), A.check_all(em32, ex, em)):
            name = rec["out"]
            assert rec["ok"], (L, causal, kind, rec)
            assert rec32["ok"], (L, causal, kind, "fp32", rec32)
            worst[name] = max(worst[name], rec["worst"] / A.E_BOUND[name])
            for i, f in enumerate(("worst", "mean_ratio", "row_ratio")):
                worst32[name][i] = max(worst32[name][i], rec32[f])
        assert A.check_lse(em["lse"], ex)[0] and A.check_lse(em32["lse"], ex)[0], (L, causal, kind)
    for name in A.OUTPUTS:
        w = worst32[name]
        print(f"[emulation] {name}: worst rho {worst[name]:.2f} of the element bound; fp32 evaluation: worst rho {w[0]:.3e}, "
              f"mean rho / emulation's {w[1]:.2f}, worst row / emulation's {w[2]:.2f}")


def test_checker_flags_corrupted_kernels():
    """Emulated kernels with one defect each, at L = 77 under the causal mask, must fail; what each one trips is printed."""
    L = 77
    ops = _ops(L, "normal")
    q, k, v, do = ops
    ex, em = A.exact(*ops, 1), A.emulate(*ops, 1)
    assert all(r["ok"] for r in A.check_all(em, ex, em))
    keep = A.causal_keep(L, 1)

    def with_(**changed):
        return {**em, **changed}

    no_diag = keep.clone()
    no_diag[L - 1, L - 1] = False
    head = slice(0, L - 1)
    cases = {
        "last query ignores its diagonal key": A.emulate(*ops, 1, keep=no_diag),
        "causal mask shifted by one": A.emulate(*ops, 1, keep=torch.tril(torch.ones(L, L, dtype=torch.bool), diagonal=1)),
        "scale off by 2 %": A.emulate(*ops, 1, scale=0.125 * 1.02),
        "dk, dv without the last query": with_(dk=A.bf(em["ds"][:, head].transpose(1, 2) @ q[:, head]),
                                               dv=A.bf(em["p"][:, head].transpose(1, 2) @ do[:, head])),
        "two rows of o swapped": with_(o=em["o"][:, [*range(10), 11, 10, *range(12, L)]]),
        "truncation instead of rounding": A.emulate(*ops, 1, rnd=A.bf_trunc),
    }
    trips = {}
    for name, got in cases.items():
        recs = A.check_all(got, ex, em)
        trips[name] = A.tripped(recs)
        print(f"[checker] {name}: " + ", ".join(f"{r['out']} {trips[name][r['out']] or 'passes'} (worst rho {r['worst']:.2e}, "
                                                f"mean x{r['mean_ratio']:.1f}, row x{r['row_ratio']:.1f})" for r in recs))
        assert any(trips[name].values()), name
    t = trips["last query ignores its diagonal key"]
    assert "E" in t["o"] and "E" in t["dk"] and "E" in t["dv"] and "R" in t["dq"], t
    assert any("M" in s for s in trips["truncation instead of rounding"].values())
    t = trips["dk, dv without the last query"]
    assert t["dk"] and t["dv"] and not t["o"] and not t["dq"], t
    t = trips["two rows of o swapped"]
    assert t["o"] and not (t["dq"] or t["dk"] or t["dv"]), t

    # one head's output in another head's columns
    ops2 = _ops(L, "normal", heads=2)
    ex2, em2 = A.exact(*ops2, 1), A.emulate(*ops2, 1)
    got = {**em2, "o": em2["o"][[0, 0]]}
    t = A.tripped(A.check_all(got, ex2, em2))
    print(f"[checker] one head's o in another head's columns: {t}")
    assert "E" in t["o"]

    # bias_grad: the fp32 column sums of dqkv pass; without one row's contribution they fail
    x = torch.cat([em["dq"][0], em["dk"][0], em["dv"][0]], dim=1)
    base = torch.randn(3 * A.HD, generator=torch.Generator().manual_seed(1)).double()
    added = lambda rows: (base.float() + rows.float().sum(0)).double() - base
    ok, ratio = A.check_bias(added(x), x, base)
    ok_bad, ratio_bad = A.check_bias(added(x[:L - 1]), x, base)
    print(f"[checker] bias_grad: fp32 column sums {ratio:.3f} of the bound; one row missing {ratio_bad:.1f} of it")
    assert ok and not ok_bad


# ---------------------------------------------------------------------------------------------------------------
# GPU: the default forms

def _run(case):
    rec, bufs = A.run_case(case, DEV)
    assert rec["ok"], {k: v for k, v in rec.items() if k != "outputs"} | {"failed": [w for w in rec["outputs"] if not w["ok"]]}
    return rec, bufs


@pytest.mark.gpu
@pytest.mark.parametrize("case", SHORT_CASES, ids=[c.name for c in SHORT_CASES])
def test_short_attention_against_fp64(case):
    """attn_fwd_kernel / attn_bwd_kernel, one workgroup per (sample, head): every bucket edge (T = 2, 4, 6, 8 tiles), a single
    token, odd lengths, four input kinds; dense and wide leading dimensions alternate over the cases."""
    _run(case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", LONG_CASES, ids=[c.name for c in LONG_CASES])
def test_long_attention_against_fp64(case):
    """attn_fwd_long_kernel / attn_bwd_long_dq_kernel / attn_bwd_long_dkv_kernel in the default forms: the plain block order
    (B H = 3) and the XCD-owned one (B H = 8), with and without the causal mask, lengths around the 64-row blocks (192 and 256
    without the mask: no block takes the masked code) and inputs that move the running maximum at every key block."""
    _run(case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", PACKED_CASES, ids=[c.name for c in PACKED_CASES])
def test_packed_attention_against_fp64(case):
    """cu_seqlens batches with samples of length 0 and 1: every sample against fp64 on its own rows, lse up to its length,
    nothing written for an empty sample, nothing outside [B, H, L]."""
    _run(case)


@pytest.mark.gpu
def test_packed_equal_lengths_give_the_dense_bits():
    packed = Case(3, 64, 2, 1, lens=[64, 64, 64], seed=64)
    dense = Case(3, 64, 2, 1, seed=64)
    _, bp = _run(packed)
    _, bd = _run(dense)
    for name, a, b in zip(("o", "lse", "dqkv"), bp.bits(), bd.bits()):
        assert torch.equal(a, b), name


@pytest.mark.gpu
@pytest.mark.parametrize("case", BITS_CASES, ids=[c.name for c in BITS_CASES])
def test_repeated_and_bias_free_calls_give_the_same_bits(case):
    """No atomics touch o, lse or dqkv: a second call gives the same bits, and so does a backward with bias_grad = NULL (which
    leaves the bias vector alone)."""
    rec, bufs = _run(case)
    first = bufs.bits()
    _run_again = A.run_case(case, DEV, bufs=bufs)[0]
    assert _run_again["ok"]
    for name, a, b in zip(("o", "lse", "dqkv"), first, bufs.bits()):
        assert torch.equal(a, b), name
    bufs.fresh()
    assert bufs.forward() == 0 and bufs.backward(bias=False) == 0
    torch.cuda.synchronize()
    for name, a, b in zip(("o", "lse", "dqkv"), first, bufs.bits()):
        assert torch.equal(a, b), f"{name} without bias_grad"
    assert torch.equal(bufs.bias[:3 * bufs.D], bufs.bias_base) and all(bufs.guards().values())


@pytest.mark.gpu
def test_attention_refusals_write_nothing():
    """A packed batch longer than 128 tokens, a leading dimension that breaks the 16-byte row alignment and an empty batch are
    refused by both entry points: non-zero return, a message in ce_last_error, every buffer as it was."""
    from clip_event_amd._lib import lib
    long_case, short_case = Case(2, 129, 2, 0), Case(2, 77, 2, 1, wide=True)
    cu = torch.tensor([0, 129, 258], dtype=torch.int32, device=DEV)
    refused = [(("packed",), A.Buffers(long_case, DEV), dict(cu=cu)),
               (("ld must", "leading dimension"), A.Buffers(short_case, DEV), dict(ld=3 * 128 + 4)),
               (("empty",), A.Buffers(short_case, DEV), dict(B=0))]
    for words, bufs, how in refused:
        for entry, call in (("ce_attention_fwd", bufs.forward), ("ce_attention_bwd", bufs.backward)):
            rc = call(**how)
            message = lib().ce_last_error().decode()
            torch.cuda.synchronize()
            assert rc != 0 and entry in message and any(w in message for w in words), (how, rc, message)
            assert bufs.untouched(), (how, entry)


@pytest.mark.gpu
def test_long_backward_on_a_side_stream():
    """The per-stream delta scratch of the long backward on a stream of its own: a call, a larger problem that makes the
    scratch grow, and the first call again; all three against fp64, the first and the third bit-identical."""
    small, large = Case(2, 257, 4, 1, wide=True), Case(2, 577, 4, 0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        rec1, bufs = _run(small)
        first = bufs.bits()
        _run(large)
        rec2 = A.run_case(small, DEV, bufs=bufs)[0]
        side.synchronize()
        assert rec2["ok"], rec2
        for name, a, b in zip(("o", "lse", "dqkv"), first, bufs.bits()):
            assert torch.equal(a, b), name
    torch.cuda.current_stream().wait_stream(side)


# ---------------------------------------------------------------------------------------------------------------
# environment forms: the launcher reads CE_ATTN_* once per process, so each form runs in a fresh child process
# (tests/attn_child.py, the long table in both block orders) under its own time limit, one at a time.  A child that ends by a
# signal or on its time limit stops the sequence: no further child is started.

ENV_FORMS = [{"CE_ATTN_NS_FWD": "2"}, {"CE_ATTN_NS": "1"}, {"CE_ATTN_NK": "2"}, {"CE_ATTN_XCD": "0"}]
CHILD_TIMEOUT_S = 300
_stopped = []


def _form_id(env):
    return ",".join(f"{k}={v}" for k, v in env.items())


@pytest.mark.gpu
@pytest.mark.parametrize("form", ENV_FORMS, ids=[_form_id(e) for e in ENV_FORMS])
def test_long_attention_environment_form(form):
    if _stopped:
        pytest.fail(f"not started: the child of {_stopped[0]} ended by a signal or its time limit")
    env = {k: v for k, v in os.environ.items() if not k.startswith("CE_ATTN_")}
    env.update(form)
    try:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "attn_child.py")], env=env, cwd=ROOT,
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
    print(f"[{_form_id(form)}] {verdict['cases']} cases, largest figures {json.dumps(verdict['figures'])}")
    for rec in verdict["failed"]:
        print("   FAILED", rec)
    assert verdict["env"] == form
    assert r.returncode == 0 and verdict["ok"], verdict["failed"][:4]
