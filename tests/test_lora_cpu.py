"""CPU (no GPU): low-rank adapters on the host side -- the adapters' names and their place in ``trainable_tables``, the argument
checks of ``enable_lora``, config / state-dict round trips on a host model, the host ``merge_lora()`` against fp64, the checkpoint's
``'lora'`` entry, and the ctypes binding of the three new declarations."""
import ctypes
import os

import numpy as np
import pytest
import torch

from oracle import clip_oracle as O

CFG = O.ClipConfig(64, 64, 2, 128, 32, 20, 512, 128, 2, 3)      # 2 image blocks, 3 text blocks, width 128
U = 2.0 ** -24


def _mk(seed=31):
    from clip_event_amd.model import build_model
    sd = O.init_params(CFG, seed)
    return build_model({k: v.clone() for k, v in sd.items()}), sd


def _host_layout(m):
    offsets, off = {}, 0
    for n, p in m.named_parameters():
        offsets[n] = off
        off += (p.numel() + 63) // 64 * 64
    return offsets


def test_names_and_flags():
    m, sd = _mk()
    m.enable_lora(rank=4, alpha=8.0)
    names = m.lora_parameter_names()
    assert len(names) == 2 * 4 * (2 + 3)
    assert "visual.transformer.resblocks.1.attn.in_proj_lora_A" in names and "transformer.resblocks.2.attn.out_proj.lora_B" in names
    assert "transformer.resblocks.0.mlp.c_fc.lora_A" in names and "visual.transformer.resblocks.0.mlp.c_proj.lora_B" in names
    from clip_event_amd.model import _GEMM_SUFFIXES, block_of, tower_of
    pm = dict(m.named_parameters())
    for w, a, b in m._lora["entries"]:
        assert not a.endswith(_GEMM_SUFFIXES) and not b.endswith(_GEMM_SUFFIXES)
        assert block_of(a) == block_of(b) == block_of(w) and tower_of(a) == tower_of(b) == tower_of(w)
        out, inn = pm[w].shape
        assert tuple(pm[a].shape) == (4, inn) and tuple(pm[b].shape) == (out, 4)
        assert not pm[w].requires_grad and pm[a].requires_grad and pm[b].requires_grad
        assert float(pm[b].detach().abs().max()) == 0.0 and float(pm[a].detach().abs().max()) <= 1.0 / np.sqrt(inn)
    assert all(not p.requires_grad for n, p in m.named_parameters() if n not in names)      # freeze_base
    assert set(m.state_dict()) == set(sd) | set(names)


def test_placement_in_the_trainable_tables():
    """Adapters on the top text block and the top image block only: they are in the segments and chunks of their block, the
    backward stops at the lowest adapted block, and an adapted W0 is in no table."""
    from clip_event_amd.model import trainable_tables
    m, _ = _mk()
    m.enable_lora(rank=8, layers=1)
    offsets = _host_layout(m)
    named = list(m.named_parameters())
    shapes = {n: tuple(p.shape) for n, p in named}
    flags = {n: p.requires_grad for n, p in named}
    tile_names = [n for n in shapes if n.endswith(("in_proj_weight", "out_proj.weight", "c_fc.weight", "c_proj.weight"))]
    t = trainable_tables(offsets, shapes, flags, None, tile_names)
    assert t["stop_layer"] == {"visual": 1, "text": 2} and t["locked"] == {"visual": False, "text": False}
    assert t["tiles"] == []
    covered = np.zeros(max(offsets.values()) + 70000, dtype=np.int32)
    for lo, hi in t["segments"]:
        covered[lo:hi] += 1
    chunked = np.zeros_like(covered)
    for lo, hi in t["chunks"]:
        chunked[lo:hi] += 1
    for n, p in named:
        lo, hi = offsets[n], offsets[n] + p.numel()
        want = 1 if n in m.lora_parameter_names() else 0
        assert (covered[lo:hi] == want).all() and (chunked[lo:hi] == want).all(), n
    plan = m.trainable_plan()
    assert plan.stop_layer == {"visual": 1, "text": 2}
    m2, _ = _mk()
    m2.enable_lora(rank=2, towers=("text",))
    assert m2.trainable_plan().locked == {"visual": True, "text": False} and m2.trainable_plan().stop_layer["text"] == 0


@pytest.mark.parametrize("kw,word", [({"rank": 0}, "rank"), ({"rank": 65}, "rank"), ({"rank": 2.0}, "rank"), ({"alpha": 0.0}, "alpha"),
                                     ({"alpha": float("nan")}, "alpha"), ({"targets": ("qkv",)}, "targets"), ({"targets": ()}, "targets"),
                                     ({"towers": ("image",)}, "towers"), ({"layers": 0}, "layers"),
                                     ({"targets": ("c_fc", "c_fc")}, "targets")])
def test_argument_errors(kw, word):
    m, sd = _mk()
    with pytest.raises(ValueError, match=word):
        m.enable_lora(**kw)
    assert set(m.state_dict()) == set(sd) and m.lora_config() is None       # nothing was registered


def test_second_call_raises():
    m, _ = _mk()
    m.enable_lora()
    with pytest.raises(RuntimeError, match="already"):
        m.enable_lora()


def test_seed_and_freeze_base():
    a, _ = _mk()
    b, _ = _mk()
    c, _ = _mk()
    a.enable_lora(seed=5)
    b.enable_lora(seed=5)
    c.enable_lora(seed=6, freeze_base=False, targets=("c_fc",))
    n = "transformer.resblocks.0.mlp.c_fc.lora_A"
    pa, pb, pc = (dict(x.named_parameters()) for x in (a, b, c))
    assert torch.equal(pa[n], pb[n]) and not torch.equal(pa[n], pc[n])
    assert pc["logit_scale"].requires_grad and pc["transformer.resblocks.0.attn.in_proj_weight"].requires_grad
    assert not pc["transformer.resblocks.0.mlp.c_fc.weight"].requires_grad


def test_config_and_state_dict_round_trip():
    m, sd = _mk()
    m.enable_lora(rank=3, alpha=6.0, targets=("out_proj", "c_proj"), towers=("text",), layers=2, seed=9)
    cfg = m.lora_config()
    assert cfg == {"rank": 3, "alpha": 6.0, "targets": ["out_proj", "c_proj"], "towers": ["text"], "layers": 2,
                   "freeze_base": True, "seed": 9}
    with torch.no_grad():
        for n, p in m.named_parameters():
            if n.endswith("lora_B"):
                p.copy_(torch.randn(p.shape, generator=torch.Generator().manual_seed(1)))
    lsd = m.lora_state_dict()
    assert set(lsd["state"]) == set(m.lora_parameter_names()) and len(lsd["state"]) == 2 * 2 * 2
    m2, _ = _mk()
    m2.load_lora_state_dict(lsd)                       # enables them from the config
    assert m2.lora_config() == cfg
    p2 = dict(m2.named_parameters())
    assert all(torch.equal(p2[n], v) for n, v in lsd["state"].items())
    bad = {"config": cfg, "state": dict(list(lsd["state"].items())[1:])}
    with pytest.raises(ValueError, match="missing"):
        m2.load_lora_state_dict(bad)
    # a plain (base) state dict loads under adapters and leaves them alone
    m2.load_state_dict(sd)
    assert all(torch.equal(p2[n], v) for n, v in lsd["state"].items())


def test_host_merge_against_fp64():
    m, sd = _mk()
    flags = {n: p.requires_grad for n, p in m.named_parameters()}
    m.visual.conv1.weight.requires_grad_(False)
    flags["visual.conv1.weight"] = False
    m.enable_lora(rank=5, alpha=10.0)
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if n.endswith("lora_B"):
                p.copy_(torch.randn(p.shape, generator=g) * 0.1)
    pm = {n: p.detach().clone() for n, p in m.named_parameters()}
    entries, s = list(m._lora["entries"]), m.lora_scale()
    m.merge_lora()
    assert m.lora_config() is None and set(m.state_dict()) == set(sd)
    assert {n: p.requires_grad for n, p in m.named_parameters()} == flags
    now = dict(m.named_parameters())
    worst = 0.0
    for w, a, b in entries:
        ref = pm[w].double() + s * (pm[b].double() @ pm[a].double())
        mag = pm[w].double().abs() + s * (pm[b].double().abs() @ pm[a].double().abs())
        err, bound = (now[w].double() - ref).abs(), (5 + 2) * U * mag
        worst = max(worst, float((err / bound).max()))
        assert bool((err <= bound).all()), w
    print(f"[host merge] worst |err| / bound {worst:.3f}")
    untouched = [n for n in sd if n not in {e[0] for e in entries}]
    assert all(torch.equal(now[n], pm[n]) for n in untouched)
    with pytest.raises(RuntimeError, match="no adapters"):
        m.merge_lora()


def test_checkpoint_keys_with_and_without_adapters(tmp_path):
    from clip_event_amd.checkpoint import CKPT_KEYS, checkpoint_dict, load_checkpoint
    from clip_event_amd.model import build_model
    m, sd = _mk()
    plain = checkpoint_dict(m, None, "t", 1, 0.0)
    assert tuple(plain) == CKPT_KEYS and set(plain["state_dict"]) == set(sd)
    m.enable_lora(rank=2, alpha=4.0, layers=1)
    with torch.no_grad():
        dict(m.named_parameters())["transformer.resblocks.2.mlp.c_fc.lora_B"].fill_(0.25)
    ck = checkpoint_dict(m, None, "t", 1, 0.0)
    assert tuple(ck) == CKPT_KEYS + ("lora",) and ck["lora"] == m.lora_config()
    assert set(ck["state_dict"]) == set(sd) | set(m.lora_parameter_names())
    path = os.path.join(tmp_path, "t_1.pth")
    torch.save(ck, path)
    m2, _, _, _ = load_checkpoint(path)
    assert m2.lora_config() == m.lora_config()
    a, b = m.state_dict(), m2.state_dict()
    assert set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a)
    assert {n for n, p in m2.named_parameters() if p.requires_grad} == set(m2.lora_parameter_names())
    with pytest.raises(ValueError, match="no adapter config"):
        build_model({k: v.clone() for k, v in ck["state_dict"].items()})


def test_signatures_bind_the_new_declarations():
    from clip_event_amd._lib import LoraJob, lora_job_table, signatures
    from clip_event_amd.build import HEADER
    with open(HEADER) as f:
        sig = signatures(f.read())
    vp, ci = ctypes.c_void_p, ctypes.c_int
    assert sig["ce_lora_merge"] == (ci, [vp, vp, ci, ci, ci, vp])
    assert sig["ce_lora_grad"] == (ci, [vp, vp, ci, ci, vp, ctypes.c_size_t, vp])
    assert sig["ce_lora_grad_workspace_bytes"] == (ctypes.c_size_t, [vp, ci])
    assert ctypes.sizeof(LoraJob) == 96 and LoraJob.ws_start.offset == 88 and LoraJob.rows.offset == 64
    jobs, tiles, strips = lora_job_table([(16, 32, 0, 48, 64, 80, 96, 112, 72, 40, 3, 0.5), (16, 32, 48, 48, 64, 80, 96, 112, 200, 136, 8, 2.0)])
    assert (tiles, strips) == (2 + 4 * 3, 2 + 4)
    assert (jobs[1].tile_start, jobs[1].strip_start, jobs[1].ws_start) == (2, 2, 2 * 3 * 40) and jobs[0].wt is None


def test_host_table_checks_need_no_gpu():
    """``ce_lora_grad_workspace_bytes`` and the refusals are host arithmetic: fake addresses, nothing is launched."""
    from clip_event_amd import _lib as L
    cl = L.lib()
    jobs, tiles, strips = L.lora_job_table([(4096, 8192, 0, 12288, 16384, 20480, 24576, 28672, 520, 72, 16, 1.0)])
    assert cl.ce_lora_grad_workspace_bytes(jobs, 1) == 4 * 9 * 16 * 72
    jobs[0].rank = 65
    assert cl.ce_lora_grad_workspace_bytes(jobs, 1) == 0 and b"1..64" in cl.ce_last_error()
    assert cl.ce_lora_merge(jobs, ctypes.c_void_p(4096), 1, tiles, 0, None) == -22
    jobs[0].rank, jobs[0].cols = 16, 76
    assert cl.ce_lora_grad(jobs, ctypes.c_void_p(4096), 1, strips, ctypes.c_void_p(4096), 1 << 30, None) == -22
    assert b"multiples of 8" in cl.ce_last_error()
