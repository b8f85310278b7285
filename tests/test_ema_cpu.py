"""CPU (no GPU): the host side of the weight EMA -- ``optim.ema_rate``, the argument rules of ``enable_ema`` and of the
``_ema`` entry points (checked before any launch), and the ``'ema'`` checkpoint entry through ``torch.save`` /
``torch.load(weights_only=True)``.  Stand-ins for the model where a device would be needed, as tests/test_sgd_cpu.py."""
from ctypes import c_float, c_int, c_long, c_void_p

import pytest
import torch

from tests.test_sgd_cpu import _Stub


def test_ema_rate_without_and_with_warmup():
    """Without warm-up the rate is 1 - decay whatever the count; with it 1 - min(decay, (1 + k) / (10 + k)): 0.9, 9/11, 10/12,
    ... of weight on the new masters' side until the cap -- for decay 0.99 the ramp reaches it at k = 890 exactly
    ((1 + k) / (10 + k) >= 0.99 <=> k >= 890)."""
    from clip_event_amd.optim import ema_rate
    assert [ema_rate(0.999, False, k) for k in (0, 1, 10, 10 ** 6)] == [1 - 0.999] * 4
    assert ema_rate(0.0, False, 5) == 1.0 and ema_rate(0.0, True, 5) == 1.0
    got = [ema_rate(0.9999, True, k) for k in range(4)]
    want = [1 - 1 / 10, 1 - 2 / 11, 1 - 3 / 12, 1 - 4 / 13]
    assert got == pytest.approx(want, rel=1e-15) and got[0] == pytest.approx(0.9) and got[1] == pytest.approx(9 / 11)
    rates = [ema_rate(0.99, True, k) for k in range(0, 2000)]
    assert all(a >= b for a, b in zip(rates, rates[1:]))                       # never rises
    assert ema_rate(0.99, True, 889) == pytest.approx(1 - 890 / 899) and ema_rate(0.99, True, 889) > 1 - 0.99
    assert ema_rate(0.99, True, 890) == pytest.approx(1 - 0.99, rel=1e-12)
    assert all(r == 1 - 0.99 for r in rates[891:])
    assert isinstance(ema_rate(0.5, True, 3), float)


def test_enable_ema_refuses_a_decay_outside_the_unit_interval():
    """0 <= decay < 1, checked before anything touches a device; a refused call leaves EMA off."""
    from clip_event_amd.optim import FusedAdam, FusedSGD
    for opt in (FusedAdam(_Stub(), lr=0.1), FusedSGD(_Stub(), lr=0.1, momentum=0.9)):
        assert not opt.ema_enabled and opt.ema is None and opt.ema_updates == 0
        for bad in (1.0, 1.5, -0.1, float("nan")):
            with pytest.raises(ValueError, match="decay"):
                opt.enable_ema(bad)
            assert not opt.ema_enabled
        with pytest.raises(RuntimeError, match="enable_ema"):
            with opt.averaged():
                pass
        with pytest.raises(RuntimeError, match="EMA is off"):
            opt.ema_state_dict()
        opt.disable_ema()                                                         # off already: nothing to do


def test_ema_argument_errors_are_reported_without_a_gpu():
    """NULL ``ema`` and a rate outside (0, 1] return -EINVAL from every ``_ema`` entry point with a message that names the
    entry point; validation comes before any launch, so nothing is launched on the fake pointers."""
    from clip_event_amd._lib import lib
    from clip_event_amd.optim import OptimGroup
    cl = lib()
    fake, null = c_void_p(0x1000), c_void_p(0)
    groups = (OptimGroup * 1)(OptimGroup(0.1, 0.0, 0, 0))
    tables = (fake, c_int(1), c_int(1), fake, c_int(1))
    adam, sgd = (c_float(0.9), c_float(0.999), c_float(1e-8)), (c_float(0.9), c_float(0.0))
    heads = {
        "ce_adam_step_ema": (fake, fake, fake, fake, fake, c_long(8), None, c_float(1.0), c_float(0.1), *adam, c_float(0.0), c_int(1)),
        "ce_adam_step_tiles_ema": (fake, fake, fake, fake, fake, *tables, None, c_float(1.0), c_float(0.1), *adam, c_float(0.0), c_int(1)),
        "ce_adam_step_groups_ema": (fake, fake, fake, fake, fake, *tables, None, None, c_float(1.0), groups, c_int(1), *adam, c_int(1)),
        "ce_sgd_step_ema": (fake, fake, fake, fake, c_long(8), None, c_float(1.0), c_float(0.1), *sgd, c_float(0.0), c_int(0), c_int(1)),
        "ce_sgd_step_tiles_ema": (fake, fake, fake, fake, *tables, None, c_float(1.0), c_float(0.1), *sgd, c_float(0.0), c_int(0), c_int(1)),
        "ce_sgd_step_groups_ema": (fake, fake, fake, fake, *tables, None, None, c_float(1.0), groups, c_int(1), *sgd, c_int(0), c_int(1)),
    }
    for name, head in heads.items():
        for ema, rate, msg in ((null, 0.5, b"ema is NULL"), (fake, 0.0, b"ema_rate"), (fake, 1.5, b"ema_rate"), (fake, -1.0, b"ema_rate"),
                               (fake, float("nan"), b"ema_rate")):
            rc = getattr(cl, name)(*head, ema, c_float(rate), None)
            assert rc == -22, (name, rate, rc)
            err = cl.ce_last_error()
            assert msg in err and name.encode() in err, (name, err)
    assert cl.ce_swap_cast_bf16(fake, fake, fake, c_long(8), None) == -22
    assert cl.ce_swap_cast_bf16(fake, c_void_p(0x2000), fake, c_long(0), None) == -22
    assert cl.ce_swap_cast_bf16(fake, c_void_p(0x2004), fake, c_long(8), None) == -22 and b"aligned" in cl.ce_last_error()


class _EmaOpt:
    """What ``checkpoint_dict`` asks of an optimiser, with an average."""

    def __init__(self, model, on=True):
        self.model, self.ema_enabled = model, on

    def state_dict(self):
        return {"state": {}, "param_groups": [{"lr": 0.1, "params": [0, 1]}]}

    def ema_state_dict(self):
        return {"decay": 0.999, "warmup": True, "updates": 7,
                "shadow": {n: p.detach() * 0.5 + 1.0 for n, p in self.model.named_parameters()}}


def test_ema_checkpoint_entry_round_trips(tmp_path):
    """``checkpoint_dict`` adds ``'ema'`` only for an optimiser with EMA on (otherwise exactly CKPT_KEYS: the reference's file);
    the entry survives ``torch.save`` / ``torch.load(weights_only=True)`` -- plain numbers, a bool and tensors -- and
    ``load_ema`` returns it, or None for a file without one or a bare state dict."""
    from clip_event_amd.checkpoint import CKPT_KEYS, checkpoint_dict, load_ema
    m = _Stub()
    with torch.no_grad():
        m.a.copy_(torch.arange(12.0).view(4, 3))
    on, off = checkpoint_dict(m, _EmaOpt(m), "t", 3, 0.5), checkpoint_dict(m, _EmaOpt(m, on=False), "t", 3, 0.5)
    assert tuple(off) == CKPT_KEYS and tuple(on) == CKPT_KEYS + ("ema",)
    assert tuple(checkpoint_dict(m, None, "t", 3, 0.5)) == CKPT_KEYS
    paths = {}
    for name, blob in (("on", on), ("off", off), ("bare", dict(m.state_dict()))):
        paths[name] = str(tmp_path / f"{name}.pth")
        torch.save(blob, paths[name])
    ema = load_ema(paths["on"])
    assert (ema["decay"], ema["warmup"], ema["updates"]) == (0.999, True, 7)
    assert sorted(ema["shadow"]) == ["a", "b"] and torch.equal(ema["shadow"]["a"], m.a.detach() * 0.5 + 1.0)
    assert ema["shadow"]["a"].shape == (4, 3) and ema["shadow"]["b"].shape == (5,)
    assert load_ema(paths["off"]) is None and load_ema(paths["bare"]) is None
    with pytest.raises(FileNotFoundError):
        load_ema(str(tmp_path / "missing.pth"))
