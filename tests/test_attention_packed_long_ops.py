"""``ce_attention_fwd_packed`` / ``ce_attention_bwd_packed``: variable-length batches above 128 tokens on the long kernels with
per-sample lengths.  Reference, emulation, bounds, guards and ``run_case`` are tests/attn_cases.py's, unchanged;
only the two calls differ.  Lengths sit around the 64-row blocks, the 128-token bucket limit and the 64 NS query blocks; B H = 16
takes the XCD-owned block order, B H = 6 the plain one; the non-default forms run in one child process each
(tests/attn_packed_child.py)."""
import json
import os
import subprocess
import sys
from ctypes import c_int, c_long, c_void_p

import pytest
import torch

from tests import attn_cases as A
from tests.attn_cases import GUARD, Case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


class PackedBuffers(A.Buffers):
    """``attn_cases.Buffers`` whose calls go to the packed entry points."""

    def forward(self, ld=None, B=None, cu="own"):
        from clip_event_amd._lib import lib, ptr, stream
        c = self.case
        return lib().ce_attention_fwd_packed(ptr(self.qkv[GUARD:]), c_long(self.ld if ld is None else ld), ptr(self.o[GUARD:]),
                                             c_long(self.ldo), ptr(self.lse[GUARD:]), ptr(self.cu if cu == "own" else cu),
                                             c_int(c.B if B is None else B), c_int(c.L), c_int(c.H), c_int(c.causal), stream())

    def backward(self, bias=True, ld=None, B=None, cu="own"):
        from clip_event_amd._lib import lib, ptr, stream
        c = self.case
        return lib().ce_attention_bwd_packed(ptr(self.qkv[GUARD:]), c_long(self.ld if ld is None else ld), ptr(self.o[GUARD:]),
                                             c_long(self.ldo), ptr(self.dout[GUARD:]), c_long(self.lddo), ptr(self.lse[GUARD:]),
                                             ptr(self.dqkv[GUARD:]), c_long(self.lddq), ptr(self.bias) if bias else c_void_p(0),
                                             ptr(self.cu if cu == "own" else cu), c_int(c.B if B is None else B), c_int(c.L),
                                             c_int(c.H), c_int(c.causal), stream())


SHORT_UNDER_PACKED = Case(9, 128, 2, 1, lens=[1, 128, 0, 33, 32, 97, 16, 5, 0])
PACKED_LONG_CASES = A._alternate([Case(8, 248, 2, 1, lens=[248, 1, 0, 129, 64, 65, 128, 191]),       # B H = 16: the XCD-owned order
                                  Case(3, 200, 2, 1, lens=[200, 193, 7]),                             # the plain order
                                  Case(5, 257, 3, 0, lens=[257, 130, 0, 256, 33])] +
                                 [Case(4, 248, 2, 1, kind, lens=[248, 150, 192, 129]) for kind in ("peaked", "rising", "falling")] +
                                 [Case(4, 248, 2, 1, lens=[77, 10, 128, 33]),                         # nothing long under a long Lmax
                                  SHORT_UNDER_PACKED])
CHILD_CASES = PACKED_LONG_CASES[:2]


def run_packed(case, log=print, dev=DEV):
    return A.run_case(case, dev, log=log, bufs=PackedBuffers(case, dev))


def _run(case):
    rec, bufs = run_packed(case)
    assert rec["ok"], {k: v for k, v in rec.items() if k != "outputs"} | {"failed": [w for w in rec["outputs"] if not w["ok"]]}
    return rec, bufs


@pytest.mark.gpu
@pytest.mark.parametrize("case", PACKED_LONG_CASES, ids=[c.name for c in PACKED_LONG_CASES])
def test_packed_long_attention_against_fp64(case):
    """Every sample against fp64 on its own rows, lse up to its length, nothing written for an empty sample, nothing outside
    [B, H, Lmax] or the samples' rows."""
    _run(case)


@pytest.mark.gpu
def test_packed_entry_points_are_the_short_path_up_to_128_tokens():
    """L <= 128: the same bits as ce_attention_fwd / ce_attention_bwd in o, lse and dqkv."""
    _, packed = _run(SHORT_UNDER_PACKED)
    rec, plain = A.run_case(SHORT_UNDER_PACKED, DEV)
    assert rec["ok"]
    for name, a, b in zip(("o", "lse", "dqkv"), packed.bits(), plain.bits()):
        assert torch.equal(a, b), name


@pytest.mark.gpu
@pytest.mark.parametrize("causal", (0, 1))
def test_full_length_packed_batch_gives_the_dense_bits(causal):
    """Every length equal to Lmax: o, lse and dqkv bit-identical to the dense call (bias_grad, added with atomics in both,
    inside its bound: run_case checks it)."""
    _, bp = _run(Case(2, 192, 4, causal, lens=[192, 192], seed=192 + causal))
    rec, bd = A.run_case(Case(2, 192, 4, causal, seed=192 + causal), DEV)
    assert rec["ok"]
    for name, a, b in zip(("o", "lse", "dqkv"), bp.bits(), bd.bits()):
        assert torch.equal(a, b), name


@pytest.mark.gpu
def test_packed_refusals_write_nothing():
    """A null cu_seqlens and an empty batch are refused by both entry points before any launch."""
    from clip_event_amd._lib import lib
    case = Case(3, 200, 2, 1, lens=[200, 193, 7])
    for words, how in ((("cu_seqlens",), dict(cu=None)), (("empty",), dict(B=0))):
        bufs = PackedBuffers(case, DEV)
        for entry, call in (("ce_attention_fwd_packed", bufs.forward), ("ce_attention_bwd_packed", bufs.backward)):
            rc = call(**how)
            message = lib().ce_last_error().decode()
            torch.cuda.synchronize()
            assert rc != 0 and entry in message and any(w in message for w in words), (how, rc, message)
            assert bufs.untouched(), (how, entry)


# ---------------------------------------------------------------------------------------------------------------
# the non-default forms of the long kernels, one fresh process each (the launcher reads CE_ATTN_* once per process), one at a
# time; a child that ends by a signal or on its time limit stops the sequence

ENV_FORMS = [{"CE_ATTN_NS_FWD": "2"}, {"CE_ATTN_NS": "1"}, {"CE_ATTN_NK": "2"}, {"CE_ATTN_XCD": "0"}]
CHILD_TIMEOUT_S = 120
_stopped = []


def _form_id(env):
    return ",".join(f"{k}={v}" for k, v in env.items())


@pytest.mark.gpu
@pytest.mark.parametrize("form", ENV_FORMS, ids=[_form_id(e) for e in ENV_FORMS])
def test_packed_long_attention_environment_form(form):
    if _stopped:
        pytest.fail(f"not started: the child of {_stopped[0]} ended by a signal or its time limit")
    env = {k: v for k, v in os.environ.items() if not k.startswith("CE_ATTN_")}
    env.update(form)
    try:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "attn_packed_child.py")], env=env, cwd=ROOT,
                           capture_output=True, text=True, timeout=CHILD_TIMEOUT_S)
    except subprocess.TimeoutExpired:
        _stopped.append(_form_id(form))
        pytest.fail(f"{_form_id(form)}: no verdict within {CHILD_TIMEOUT_S} s")
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
        _stopped.append(_form_id(form))
        pytest.fail(f"{_form_id(form)}: child ended with {r.returncode}\n{r.stderr[-3000:]}")
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert lines, f"{_form_id(form)}: no verdict (rc {r.returncode})\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}"
    verdict = json.loads(lines[-1])
    print(f"[{_form_id(form)}] {verdict['cases']} cases, largest figures {json.dumps(verdict['figures'])}")
    assert verdict["env"] == form
    assert r.returncode == 0 and verdict["ok"], verdict["failed"][:4]
