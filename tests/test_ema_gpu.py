"""GPU: the weight EMA through the model -- ``enable_ema`` on FusedAdam / FusedSGD, the ``averaged()`` context, partial
fine-tuning, fp8 operands and the checkpoint entry.  Tiny oracle geometry of tests/test_partial_gpu.py (2 image blocks, 3 text
blocks, width 128), 4 steps.

Two ``train_step`` runs from the same seed do not give the same bits here: the LayerNorm / bias gradient sums are float atomics
(tests/test_partial_gpu.py's spread rule; measured on this geometry: the flat gradient of two twins differs after the first
step already, without any EMA).  Where a test below asks for bit-identity BETWEEN runs, the second run therefore takes the step
gradients the first run recorded (``_train``): both runs go through ``train_step`` -- forward, loss, backward, ``step()`` -- and
the forward is deterministic, so masters, moments and losses are bit-identical exactly when the update, the operand copies it
leaves behind and the bookkeeping around them are.  The gradient norm is a sum of float atomics too, so these runs clip at a
``max_norm`` far above the norm (tests/test_model_gpu.py's device): the norm is still computed and read, and the coefficient
is exactly 1 whatever order the partial sums arrived in."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.test_ema_ops import _ema_bound, ema_ref
from tests.test_partial_gpu import DEV, _batch, _bits_equal, _crit, _mk

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = 4
CHILD_TIMEOUT_S = 240


def _opt(kind, m, **kw):
    from clip_event_amd.optim import FusedAdam, FusedSGD
    if kind == "adam":
        return FusedAdam(m, lr=1e-3, weight_decay=0.01, max_norm=1e9, **kw)
    return FusedSGD(m, lr=1e-2, momentum=0.9, weight_decay=0.01, max_norm=1e9, **kw)


def _train(m, opt, batch, tape, i):
    """One ``train_step`` whose ``step()`` sees the gradient ``tape[i]`` -- recorded from this very call when the tape is that
    short, replayed (copied over what the backward left) otherwise.  Returns the losses as floats."""
    from clip_event_amd.engine import train_step
    inner = opt.step

    def step(closure=None):
        g = m._flat_grad
        if i < len(tape):
            g.copy_(tape[i])
        else:
            tape.append(g.detach().clone())
        return inner(closure)

    opt.step = step
    try:
        ld = train_step(m, _crit(), opt, *batch)
    finally:
        del opt.step
    torch.cuda.synchronize()
    return {k: float(v.detach()) for k, v in ld.items()}


def _state_bits(opt):
    return [b.detach().clone() for b in opt.state_buffers()]


def feedback_check(kind, tiles_expected):
    """Two models from one seed, the same four steps, one of them with ``enable_ema(0.5)``: ``(ok, what differed)``."""
    batch = _batch(4)
    tape, runs = [], []
    for ema in (False, True):
        m, _ = _mk()
        opt = _opt(kind, m)
        if ema:
            opt.enable_ema(0.5)
        losses = [_train(m, opt, batch, tape, i) for i in range(STEPS)]
        tiled = bool(m._adam_tiles_ok) and os.environ.get("CE_ADAM_TILES", "1") != "0"
        runs.append((m._flat.detach().clone(), m._flat16.detach().clone(), _state_bits(opt), losses, tiled, opt))
    (p_a, p16_a, st_a, loss_a, tiled_a, _), (p_b, p16_b, st_b, loss_b, tiled_b, opt_b) = runs
    bad = []
    if tiled_a != tiles_expected or tiled_b != tiles_expected:
        bad.append(f"tile path taken: {tiled_a}, {tiled_b}; expected {tiles_expected}")
    if not _bits_equal(p_a, p_b):
        bad.append("masters")
    if not torch.equal(p16_a.view(torch.int16), p16_b.view(torch.int16)):
        bad.append("mirror")
    if len(st_a) != len(st_b) or not all(_bits_equal(a, b) for a, b in zip(st_a, st_b)):
        bad.append("state")
    if loss_a != loss_b:
        bad.append(f"losses {loss_a} / {loss_b}")
    if opt_b.ema_updates != STEPS or _bits_equal(opt_b.ema, p_b):
        bad.append("the average did not run")
    return not bad, bad


# ---- 1. the average never feeds back -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_the_average_never_feeds_back(kind):
    """FusedAdam / FusedSGD(momentum 0.9): masters, mirror, moments and the returned losses of four steps are bit-identical with
    and without ``enable_ema(0.5)`` (tile + segment path), and the average did move."""
    ok, bad = feedback_check(kind, tiles_expected=True)
    assert ok, bad


def test_the_average_never_feeds_back_on_the_flat_path():
    """The same for FusedAdam with CE_ADAM_TILES=0 (the flat kernel) in a child process (tests/ema_child.py)."""
    env = dict(os.environ, CE_ADAM_TILES="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "ema_child.py")], env=env, cwd=ROOT, capture_output=True, text=True,
                       timeout=CHILD_TIMEOUT_S)
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert lines, f"no verdict (rc {r.returncode})\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}"
    verdict = json.loads(lines[-1])
    print(verdict)
    assert r.returncode == 0 and verdict["ok"] and verdict["env"] == "0", verdict


# ---- 2. the average is the recurrence ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("decay,warmup", [(0.5, False), (0.9, False), (0.9999, True)])
def test_the_average_is_the_recurrence_over_the_masters(decay, warmup):
    """``model._flat`` recorded after every step: the average equals e_k = e_{k-1} + r_k (p_k - e_{k-1}) in fp64 from e_0 = p_0
    within 4 x the op-level bound (four steps, each adding at most one op-level error; an earlier error shrinks by 1 - r_k; the
    bound is the largest of the four per-step ones, element by element), with r_k = ``ema_rate(decay, warmup, k)`` rounded to
    fp32 as the kernel receives it -- with warm-up 0.9, 9/11, 10/12, 11/13 of weight on the new masters' side."""
    from clip_event_amd.optim import ema_rate
    m, _ = _mk()
    opt = _opt("adam", m)
    opt.enable_ema(decay, warmup=warmup)
    e = m._flat.detach().double().clone()
    assert _bits_equal(opt.ema, m._flat) and opt.ema_updates == 0 and opt.ema_enabled
    batch, tape = _batch(4), []
    bound = torch.zeros_like(e)
    rates = []
    for k in range(STEPS):
        _train(m, opt, batch, tape, k)
        r = float(np.float32(ema_rate(decay, warmup, k)))
        rates.append(r)
        p = m._flat.detach()
        ref = ema_ref(e, p, r)
        bound = torch.maximum(bound, _ema_bound(ref, e, p, r))
        e = ref
    if warmup:
        assert rates == [float(np.float32(1 - x)) for x in (1 / 10, 2 / 11, 3 / 12, 4 / 13)]
    err = (opt.ema.double() - e).abs()
    worst = float((err / (4 * bound).clamp_min(1e-300)).max())
    print(f"[ema recurrence decay={decay} warmup={warmup}] rates {rates}; worst |err| / (4 x bound) {worst:.3f}")
    assert opt.ema_updates == STEPS and bool((err <= 4 * bound).all()), worst
    assert not _bits_equal(opt.ema, m._flat)


# ---- 3. partial fine-tuning --------------------------------------------------------------------------------------------------------

def test_the_average_of_a_frozen_parameter_is_the_parameter():
    """Locked image tower, ``text_projection`` frozen by hand, two param groups (``no_decay_groups``): after four steps the
    average of every frozen parameter is the parameter, bit for bit, and that of every trainable one is not.  Then
    ``text_projection`` is unfrozen and one step taken: its average starts from its value -- not from zero, as its moments do --
    and is ema_ref(value before, value after) within the op-level bound."""
    from clip_event_amd.optim import FusedAdam, ema_rate, no_decay_groups
    m, sd = _mk()
    m.lock_image_tower()
    m.text_projection.requires_grad_(False)
    opt = FusedAdam(m, lr=1e-3, max_norm=1.0, groups=no_decay_groups(m, 0.1))
    assert len(opt.param_groups) == 2
    opt.enable_ema(0.9)
    batch, tape = _batch(4), []
    for k in range(STEPS):
        _train(m, opt, batch, tape, k)
    shadow = opt.ema_state_dict()["shadow"]
    frozen = [n for n, p in m.named_parameters() if not p.requires_grad]
    assert "text_projection" in frozen and any(n.startswith("visual.") for n in frozen)
    for n, p in m.named_parameters():
        assert shadow[n].shape == p.shape
        if n in frozen:
            assert _bits_equal(shadow[n], p) and _bits_equal(p, sd[n]), n
        elif n != "logit_scale":
            assert not _bits_equal(shadow[n], p), n
    before = m.text_projection.detach().clone()
    m.text_projection.requires_grad_(True)
    _train(m, opt, batch, tape, STEPS)
    after, avg = m.text_projection.detach(), opt.ema_state_dict()["shadow"]["text_projection"]
    assert not _bits_equal(after, before) and not _bits_equal(avg, before) and not _bits_equal(avg, after)
    r = float(np.float32(ema_rate(0.9, False, STEPS)))
    ref = ema_ref(before, after, r)
    err = (avg.double() - ref).abs()
    assert bool((err <= _ema_bound(ref, before, after, r)).all())


# ---- 4. averaged() -----------------------------------------------------------------------------------------------------------------

def _features(m, batch):
    with torch.no_grad():
        return m.encode_image(batch[0]).clone(), m.encode_text(batch[1]).clone()


def _fresh_from(shadow):
    from clip_event_amd.model import build_model
    return build_model({k: v.detach().cpu().clone() for k, v in shadow.items()}).to(DEV)


def _trained(kind="adam", decay=0.5, tape=None):
    """A model and its optimiser after four steps with EMA on; ``tape``: the step gradients of an earlier run to replay."""
    m, _ = _mk()
    opt = _opt(kind, m)
    opt.enable_ema(decay)
    batch, tape = _batch(4), [] if tape is None else tape
    for k in range(STEPS):
        _train(m, opt, batch, tape, k)
    return m, opt, batch, tape


def test_averaged_context_swaps_the_average_in_and_back():
    """Inside ``averaged()``: the features equal those of a fresh model built from the shadow (``torch.equal``, the suite's rule
    for a forward from the same weights), the mirror is that model's mirror, ``state_dict()`` holds the shadow, ``step()`` /
    ``enable_ema`` / ``disable_ema`` / a nested ``averaged()`` raise.  After exit -- also after an exception inside -- masters,
    average and mirror have their bits back, the features are the training weights' again, and one more ``train_step`` gives the
    masters of a twin that never entered the context."""
    m, opt, batch, tape = _trained()
    twin, topt, _, _ = _trained(tape=tape)
    assert _bits_equal(twin._flat, m._flat) and _bits_equal(topt.ema, opt.ema)     # (same tape: same bits)
    shadow = opt.ema_state_dict()["shadow"]
    fresh = _fresh_from(shadow)
    want = _features(fresh, batch)
    raw = _features(m, batch)
    p0, e0, p16_0 = m._flat.detach().clone(), opt.ema.detach().clone(), m._flat16.detach().clone()
    assert not _bits_equal(p0, e0)
    with opt.averaged() as inside:
        assert inside is m
        got = _features(m, batch)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
        assert not torch.equal(got[0], raw[0]) and not torch.equal(got[1], raw[1])
        assert torch.equal(m._flat16.view(torch.int16), fresh._flat16.view(torch.int16))
        assert _bits_equal(m._flat, e0) and _bits_equal(opt.ema, p0)
        state = m.state_dict()
        assert all(_bits_equal(state[n], shadow[n]) for n in shadow)
        inner = opt.ema_state_dict()["shadow"]
        assert all(_bits_equal(inner[n], shadow[n]) for n in shadow)
        for call in (opt.step, lambda: opt.enable_ema(0.9), opt.disable_ema, lambda: opt.averaged().__enter__()):
            with pytest.raises(RuntimeError, match="averaged"):
                call()
    torch.cuda.synchronize()
    assert _bits_equal(m._flat, p0) and _bits_equal(opt.ema, e0) and torch.equal(m._flat16.view(torch.int16), p16_0.view(torch.int16))
    back = _features(m, batch)
    assert torch.equal(back[0], raw[0]) and torch.equal(back[1], raw[1])
    with pytest.raises(KeyError, match="boom"):
        with opt.averaged():
            raise KeyError("boom")
    torch.cuda.synchronize()
    assert _bits_equal(m._flat, p0) and _bits_equal(opt.ema, e0) and torch.equal(m._flat16.view(torch.int16), p16_0.view(torch.int16))
    la = _train(m, opt, batch, tape, STEPS)
    lb = _train(twin, topt, batch, tape, STEPS)
    assert la == lb and _bits_equal(m._flat, twin._flat) and _bits_equal(opt.ema, topt.ema)
    assert all(_bits_equal(a, b) for a, b in zip(opt.state_buffers(), topt.state_buffers()))
    assert opt.ema_updates == STEPS + 1


def test_averaged_needs_an_average_and_disable_frees_it():
    m, _ = _mk()
    opt = _opt("sgd", m)
    assert not opt.ema_enabled and opt.ema is None
    with pytest.raises(RuntimeError, match="enable_ema"):
        with opt.averaged():
            pass
    opt.enable_ema(0.99, warmup=True)
    assert opt.ema_enabled and opt.ema.shape == m._flat.shape and opt.ema.dtype == torch.float32 and _bits_equal(opt.ema, m._flat)
    assert opt.ema.data_ptr() not in [b.data_ptr() for b in opt.state_buffers()]
    opt.disable_ema()
    assert not opt.ema_enabled and opt.ema is None and opt.ema_updates == 0


# ---- 5. fp8 ------------------------------------------------------------------------------------------------------------------------

def test_fp8_operands_follow_the_swap(monkeypatch):
    """CE_FP8=1 (forward GEMMs on e4m3 copies of the block weights, rebuilt from the bf16 mirror): inside ``averaged()`` the
    features differ from those outside and equal those of a fresh fp8 model built from the shadow; after exit they are the
    training weights' again: the fp8 operands were refreshed both ways."""
    monkeypatch.setenv("CE_FP8", "1")
    m, opt, batch, _ = _trained()
    assert m.fp8 == 1
    raw = _features(m, batch)
    fresh = _fresh_from(opt.ema_state_dict()["shadow"])
    assert fresh.fp8 == 1
    want = _features(fresh, batch)
    with opt.averaged():
        got = _features(m, batch)
    back = _features(m, batch)
    assert not torch.equal(got[0], raw[0]) and not torch.equal(got[1], raw[1])
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert torch.equal(back[0], raw[0]) and torch.equal(back[1], raw[1])


# ---- 6. checkpoint -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_checkpoint_carries_the_average(kind, tmp_path):
    """``checkpoint_dict`` has the ``'ema'`` key with EMA on and exactly CKPT_KEYS with it off; save -> ``load_checkpoint`` +
    ``load_ema`` -> ``load_state_dict`` + ``load_ema_state_dict`` -> one more step gives the masters and the average of the
    uninterrupted run, bit for bit."""
    from clip_event_amd.checkpoint import CKPT_KEYS, checkpoint_dict, load_checkpoint, load_ema, save_model_on_master
    m, opt, batch, tape = _trained(kind, decay=0.9)
    assert set(checkpoint_dict(m, opt, "t", 1, 0.0)) == set(CKPT_KEYS) | {"ema"}
    path = save_model_on_master(m, str(tmp_path), "t", 1, 0.0, optimizer=opt)
    assert path is not None
    _train(m, opt, batch, tape, STEPS)
    m2, opt_state, epoch, _ = load_checkpoint(path, device=DEV)
    ema = load_ema(path)
    assert epoch == 1 and ema["decay"] == 0.9 and ema["updates"] == STEPS and not ema["warmup"]
    assert all(t.device.type == "cpu" for t in ema["shadow"].values())
    opt2 = _opt(kind, m2)
    opt2.load_state_dict(opt_state)
    opt2.load_ema_state_dict(ema)
    assert opt2.ema_enabled and opt2.ema_updates == STEPS and opt2.ema_decay == 0.9
    _train(m2, opt2, batch, tape, STEPS)
    assert _bits_equal(m2._flat, m._flat) and _bits_equal(opt2.ema, opt.ema)
    opt.disable_ema()
    assert set(checkpoint_dict(m, opt, "t", 1, 0.0)) == set(CKPT_KEYS)
    off = save_model_on_master(m, str(tmp_path), "t", 2, 0.0, optimizer=opt)
    assert load_ema(off) is None
    bad = dict(ema, shadow={k: v for k, v in ema["shadow"].items() if k != "logit_scale"})
    with pytest.raises(ValueError, match="logit_scale"):
        opt2.load_ema_state_dict(bad)
