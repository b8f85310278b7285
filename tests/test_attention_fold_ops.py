"""The short attention backward's in_proj bias gradient in its partial-row form (``ce_attention_bwd_partials`` +
``ce_layernorm_fold``) and the paired column map of the short kernels' output tiles.

* Op level: the partial form on the buffers of tests/attn_cases.py, after ``run_case`` has checked the atomic form of the same
  inputs against fp64: ``dqkv`` bit-equal to ``ce_attention_bwd``'s, every entry of a NaN-filled ``partials[B][3][H*64]`` written
  (exact zeros for an empty sample), the fold into a non-zero base within ``attn_cases.check_bias`` of the kernel's own dqkv
  (which proves ``+=``), and two runs bit-identical (a workgroup adds its waves' sums in wave order, the fold adds the rows in row
  order: nothing depends on arrival order).
* Column map: q, k, v, dO with a distinct power-of-two-ish scale on every head-dim column, against fp64 per element: a column
  group stored in another group's place is off by the ratio of their scales, far outside the element bound.
* Tower level: a 10-layer model (more layers than ring slots), image tower dense, text tower packed with ``sel_rows``, backward in
  one child process per form (tests/attn_fold_child.py; CE_ATTN_FOLD is read once per process).
* CPU: ``ce_tower_workspace_bytes`` grows by exactly the ring (towers of at most 128 tokens), by nothing above."""
import ctypes
import os
import subprocess
import sys
from ctypes import c_int, c_long

import pytest
import torch

from tests import attn_cases as A
from tests.attn_cases import GUARD, HD, SENTINEL, Case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"

FOLD_CASES = [Case(2, 50, 3, 0), Case(2, 77, 3, 1), Case(2, 1, 3, 0), Case(2, 128, 3, 1),
              Case(8, 77, 3, 1, lens=[77, 10, 0, 33, 1, 64, 77, 17])]


class Job(ctypes.Structure):
    """``ce_ln_fold_job`` of include/clip_event_hip.h."""
    _fields_ = [("partials", ctypes.c_void_p), ("dw", ctypes.c_void_p), ("db", ctypes.c_void_p), ("dxsum", ctypes.c_void_p),
                ("blocks", c_int), ("D", c_int)]


def _backward_partials(bufs, partials):
    """``ce_attention_bwd_partials`` on the buffers' operands (o and lse as the forward left them) into a fresh NaN dqkv."""
    from clip_event_amd._lib import lib, ptr, stream
    c = bufs.case
    bufs.dqkv = bufs._matrix(bufs.rows, bufs.lddq, torch.full((bufs.rows, 3 * bufs.D), float("nan"), dtype=torch.bfloat16), bufs.dev)
    return lib().ce_attention_bwd_partials(ptr(bufs.qkv[GUARD:]), c_long(bufs.ld), ptr(bufs.o[GUARD:]), c_long(bufs.ldo),
                                           ptr(bufs.dout[GUARD:]), c_long(bufs.lddo), ptr(bufs.lse[GUARD:]), ptr(bufs.dqkv[GUARD:]),
                                           c_long(bufs.lddq), ptr(partials), ptr(bufs.cu), c_int(c.B), c_int(c.L), c_int(c.H),
                                           c_int(c.causal), stream())


def _fold(partials, bias, B, D):
    """One ``ce_layernorm_fold`` job in the tower's format: blocks = B, dw | db | dxsum = the three D-column thirds of bias."""
    from clip_event_amd._lib import lib, stream
    p = bias.data_ptr()
    job = Job(partials.data_ptr(), p, p + 4 * D, p + 8 * D, B, D)
    return lib().ce_layernorm_fold((Job * 1)(job), 1, stream())


def _partial_run(bufs):
    """NaN-filled guarded partials -> partial form -> fold into the case's bias base.  Returns (partials incl. guards, bias incl.
    guards, dqkv bits)."""
    c, D = bufs.case, bufs.D
    n = c.B * 3 * D
    partials = torch.full((n + 2 * GUARD,), SENTINEL, device=bufs.dev)
    partials[GUARD:GUARD + n] = float("nan")
    assert _backward_partials(bufs, partials[GUARD:]) == 0
    bias = torch.full((3 * D + 8,), SENTINEL, device=bufs.dev)
    bias[:3 * D] = bufs.bias_base
    assert _fold(partials[GUARD:], bias, c.B, D) == 0
    torch.cuda.current_stream().synchronize()
    return partials, bias, bufs.dqkv.view(torch.int16).clone()


def _check_partial_form(bufs, atomic_dqkv_bits, log=print):
    c, D = bufs.case, bufs.D
    n = c.B * 3 * D
    partials, bias, bits = _partial_run(bufs)
    live = partials[GUARD:GUARD + n].view(c.B, 3, D)
    assert not bool(torch.isnan(live).any()), "an entry of partials was left unwritten"
    assert bool((partials[:GUARD] == SENTINEL).all()) and bool((partials[GUARD + n:] == SENTINEL).all()), "partials: written outside"
    for b, length in enumerate(c.lens):
        if length == 0:
            assert bool((live[b].view(torch.int32) == 0).all()), f"empty sample {b}: not exact zeros"
    assert torch.equal(bits, atomic_dqkv_bits), "dqkv differs from ce_attention_bwd's"
    assert all(bufs.guards().values()), bufs.guards()
    x = bufs.live(bufs.dqkv, 3 * D).cpu().double()
    base = bufs.bias_base.cpu().double()
    ok, ratio = A.check_bias(bias[:3 * D].cpu().double() - base, x, base)
    log(f"[attn fold {c.name}] folded bias_grad {ratio:.3f} of its bound")
    assert ok, ratio
    assert bool((bias[3 * D:] == SENTINEL).all())
    partials2, bias2, bits2 = _partial_run(bufs)
    assert torch.equal(partials2.view(torch.int32), partials.view(torch.int32)), "partials differ between two runs"
    assert torch.equal(bias2.view(torch.int32), bias.view(torch.int32)), "folded gradient differs between two runs"
    assert torch.equal(bits2, bits)


@pytest.mark.gpu
@pytest.mark.parametrize("case", FOLD_CASES, ids=[c.name for c in FOLD_CASES])
def test_partial_form_against_atomic_form_and_fp64(case):
    rec, bufs = A.run_case(case, DEV)                        # forward + ce_attention_bwd against fp64, bias_grad included
    assert rec["ok"], {k: v for k, v in rec.items() if k != "outputs"} | {"failed": [w for w in rec["outputs"] if not w["ok"]]}
    _check_partial_form(bufs, bufs.dqkv.view(torch.int16).clone())


def test_partial_form_refusals():
    """Argument errors are reported before any launch (no GPU needed): long sequences, a null partials buffer."""
    from clip_event_amd._lib import lib
    cl = lib()
    host = (ctypes.c_char * 64)()
    p = ctypes.cast(host, ctypes.c_void_p)
    args = lambda L, part: (p, c_long(192), p, c_long(64), p, c_long(64), p, p, c_long(192), part, None, c_int(1), c_int(L), c_int(1),
                            c_int(0), None)
    assert cl.ce_attention_bwd_partials(*args(129, p)) == -22 and b"128" in cl.ce_last_error()
    assert cl.ce_attention_bwd_partials(*args(50, None)) == -22 and b"partials" in cl.ce_last_error()
    assert cl.ce_attention_bwd_partials(*args(0, p)) == -22 and b"empty" in cl.ce_last_error()


# ---------------------------------------------------------------------------------------------------------------
# the column map of the output tiles: a distinct scale on every head-dim column

def _column_scales():
    """[4][64] scales for q, k, v, dO.  v: 2^((c - 32) / 8), 1/16 .. ~15: neighbouring columns differ by 9 %, columns 4, 8, 16 or
    32 apart -- the distances between the tiles' chunks -- by a factor of 1.4, 2, 4 or 16.  dO: the same set of scales in another
    order.  q: 2^(m / 16) with m a third order of -32 .. 31, and k its reciprocal, so that the scores keep their distribution."""
    c = torch.arange(HD, dtype=torch.float64)
    sv = 2.0 ** ((c - 32) / 8)
    sd = 2.0 ** ((((c * 37) % 64) - 32) / 8)                # 37 is odd: a permutation of the columns
    sq = 2.0 ** ((((c * 11 + 5) % 64) - 32) / 16)
    return sq, 1.0 / sq, sv, sd


@pytest.mark.gpu
@pytest.mark.parametrize("case", [Case(2, 50, 3, 0, wide=True), Case(2, 77, 3, 1, wide=True)], ids=["L50_full", "L77_causal"])
def test_output_column_map_with_a_distinct_scale_per_column(case):
    samples, _ = A.reference(case)
    scales = _column_scales()
    scaled = [tuple((t.double() * s).to(torch.bfloat16) for t, s in zip(smp, scales)) for smp in samples]     # [len, H, 64] each
    D = case.H * HD
    bufs = A.Buffers(case, DEV)
    cat = lambda t: torch.cat([s[t].reshape(-1, D) for s in scaled])
    bufs.qkv[GUARD:GUARD + bufs.rows, :3 * D] = torch.cat([cat(0), cat(1), cat(2)], dim=1).to(DEV)
    bufs.dout[GUARD:GUARD + bufs.rows, :D] = cat(3).to(DEV)
    bufs.inputs = (bufs.qkv.clone(), bufs.dout.clone())
    ops = [torch.cat([s[t].double().permute(1, 0, 2) for s in scaled]) for t in range(4)]                      # [(sample, head), L, 64]
    ex, em = A.exact(*ops, case.causal), A.emulate(*ops, case.causal)
    assert bufs.forward() == 0 and bufs.backward() == 0
    torch.cuda.current_stream().synchronize()
    got = bufs.gather(list(range(case.B)), case.L)
    for r in A.check_all(got, ex, em):
        print(f"[attn columns {case.name}] {r['out']}: worst rho {r['worst']:.3e} (bound {A.E_BOUND[r['out']]:.3e}, emulation "
              f"{r['worst_emul']:.3e}), {r['over']} over, mean x{r['mean_ratio']:.2f}, row x{r['row_ratio']:.2f}")
        assert r["ok"], r
    assert A.check_lse(got["lse"], ex)[0]
    x = bufs.live(bufs.dqkv, 3 * D).cpu().double()
    base = bufs.bias_base.cpu().double()
    ok, ratio = A.check_bias(bufs.bias[:3 * D].cpu().double() - base, x, base)
    print(f"[attn columns {case.name}] atomic bias_grad {ratio:.3f} of its bound")
    assert ok and all(bufs.guards().values()), (ratio, bufs.guards())
    _check_partial_form(bufs, bufs.dqkv.view(torch.int16).clone())


# ---------------------------------------------------------------------------------------------------------------
# tower level: more layers than ring slots, dense and packed + sel_rows, one child process per form

CHILD_TIMEOUT_S = 120
LAYERS = 10         # tests/attn_fold_child.py


def _child(env_form, out):
    env = {k: v for k, v in os.environ.items() if k != "CE_ATTN_FOLD"}
    env.update(env_form)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "attn_fold_child.py"), out], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=CHILD_TIMEOUT_S)
    assert r.returncode == 0, f"{env_form}: child ended with {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}"
    return torch.load(out, weights_only=True)


@pytest.mark.gpu
def test_tower_backward_fold_form_equals_atomic_form_across_a_ring_wrap(tmp_path):
    """Every parameter gradient bit-equal between CE_ATTN_FOLD=0 and the default except the in_proj biases (and the twelve that
    other kernels do not form reproducibly within one form, below); the in_proj biases agree to the reordering part of ``check_bias``'s bound: both forms add the same fp32 column sums (at most T per workgroup, then batch
    rows), each within 2^-18 sum |x| of the exact sum (attn_cases.BIAS_REL's fp32 term), so within 2^-17 sum |x| of each other,
    with sum |x| per column of the bf16 dqkv as the fp32 oracle gives it."""
    atomic = _child({"CE_ATTN_FOLD": "0"}, str(tmp_path / "atomic.pt"))
    fold = _child({}, str(tmp_path / "fold.pt"))
    assert atomic["attn_fold"] == 0 and fold["attn_fold"] == 1
    mags = fold["mags"]
    assert set(atomic["grads"]) == set(fold["grads"])
    biases = sorted(n for n in fold["grads"] if n.endswith("attn.in_proj_bias"))
    assert len(biases) == 20 and set(biases) == set(mags)
    # Gradients that other kernels form with float atomics from three or more writers per element can differ in the last bit
    # between two runs of ONE form (measured: 4 of 254 here, the same four with CE_ATTN_FOLD=0 and without), so bit-equality cannot
    # be asked of them: ln_pre's backward (outside the tower), the pruned last block's ln_1 backward (ce_layernorm_bwd_t over all
    # rows: d gamma, d beta and the c_proj bias of the block below), and the embedding tables below the towers, which add one
    # contribution per sample or per token occurrence (tests/test_image_size_gpu.py, _atomic_slices).  They get the bound
    # tests/test_model_gpu.py holds two runs of one backward to (relative l2 below 1e-6); their inputs are covered by the
    # bit-equal gradients downstream of the same dqkv.
    last = LAYERS - 1
    atomic_order = {"visual.ln_pre.weight", "visual.ln_pre.bias", "visual.class_embedding", "visual.positional_embedding",
                    "positional_embedding", "token_embedding.weight"}
    for prefix in ("visual.transformer.", "transformer."):
        atomic_order |= {f"{prefix}resblocks.{last}.ln_1.weight", f"{prefix}resblocks.{last}.ln_1.bias",
                         f"{prefix}resblocks.{last - 1}.mlp.c_proj.bias"}
    assert atomic_order <= set(fold["grads"])
    worst = 0.0
    for name, g in fold["grads"].items():
        a = atomic["grads"][name]
        if name in atomic_order:
            rel = float((g.double() - a.double()).norm() / a.double().norm())
            assert rel < 1e-6, (name, rel)
        elif name in mags:
            err = (g.double() - a.double()).abs()
            bound = 2.0 ** -17 * mags[name].double()              # (the gradients start from zero: no base term)
            assert bool((g != 0).any()), name
            worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
            assert bool((err <= bound).all()), (name, float((err / bound.clamp_min(1e-300)).max()))
        else:
            assert torch.equal(g.view(torch.int32), a.view(torch.int32)), f"{name} differs between the two forms"
    print(f"[attn fold tower] 20 in_proj bias gradients: worst |fold - atomic| = {worst:.3f} of the reordering bound; "
          f"{len(fold['grads']) - 20 - len(atomic_order)} other gradients bit-equal, {len(atomic_order)} within 1e-6")


# ---------------------------------------------------------------------------------------------------------------
# CPU: the workspace grows by the ring and by nothing else

LNP_RING = 8        # csrc/tower.cpp


@pytest.mark.parametrize("width,heads,tokens,causal", [(768, 12, 50, 0), (512, 8, 77, 1), (128, 2, 17, 0), (128, 2, 128, 1), (128, 2, 129, 0)])
def test_workspace_grows_by_exactly_the_attention_ring(width, heads, tokens, causal):
    from clip_event_amd._lib import lib
    from tests.test_abi_cpu import _training_workspace_bytes
    from tests.test_micro_batch_cpu import _desc
    cl = lib()
    for layers, stream16, fp8, batch in ((12, 0, 0, 256), (10, 1, 3, 3), (3, 0, 0, 5), (1, 0, 0, 1)):
        without = _training_workspace_bytes(cl, layers, width, heads, tokens, stream16, fp8, batch)      # the layout up to the LayerNorm ring
        slot = (batch * 3 * width * 4 + 255) // 256 * 256                                               # [batch][3][width] floats, 256-byte aligned
        ring = min(LNP_RING, layers) * slot if tokens <= 128 else 0
        got = cl.ce_tower_workspace_bytes(ctypes.byref(_desc(layers, width, heads, tokens, causal, stream16, fp8)), batch)
        print(f"width {width} tokens {tokens} layers {layers} batch {batch}: {got} bytes = {without} + ring {ring}")
        assert got == without + ring
