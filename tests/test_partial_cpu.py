"""CPU (no GPU): partial fine-tuning on the host side -- the trainable plan's tables from a synthetic flat layout
(``model.trainable_tables``: pure arithmetic over names, offsets, shapes and flags), the lock helpers, the group rules of
``FusedAdam`` / ``FusedSGD`` / ``no_decay_groups``, the argument checks of ``ce_sumsq_segments`` / ``ce_*_step_groups`` before any
launch, in tests/test_sgd_cpu.py's fake-pointer manner, and ``GradSync`` with a locked tower on two gloo ranks."""
import ctypes
from ctypes import c_float, c_int, c_void_p

import numpy as np
import pytest
import torch

from oracle import clip_oracle as O

CFG = O.ClipConfig(64, 64, 2, 128, 32, 20, 512, 128, 2, 3)

# a flat layout in miniature: two towers with two blocks each, four "block weights" (the tile form), offsets padded to 64;
# sizes that are no multiple of 4 (7, 21, 1) and one tensor longer than a 65536-element chunk
SHAPES = {
    "logit_scale": (),
    "visual.proj": (8, 4),
    "visual.ln_post.weight": (8,),
    "visual.transformer.resblocks.1.attn.in_proj_weight": (24, 8),
    "visual.transformer.resblocks.1.ln_1.weight": (7,),
    "visual.transformer.resblocks.0.mlp.c_fc.weight": (32, 8),
    "visual.transformer.resblocks.0.ln_1.bias": (8,),
    "visual.positional_embedding": (3, 7),
    "visual.class_embedding": (8,),
    "visual.conv1.weight": (8, 3, 2, 2),
    "visual.ln_pre.weight": (8,),
    "text_projection": (8, 4),
    "ln_final.weight": (8,),
    "transformer.resblocks.1.attn.out_proj.weight": (8, 8),
    "transformer.resblocks.1.ln_2.weight": (8,),
    "transformer.resblocks.0.mlp.c_proj.weight": (8, 32),
    "transformer.resblocks.0.ln_2.bias": (2500,),
    "positional_embedding": (6, 8),
    "token_embedding.weight": (33000, 2),
}
TILE_NAMES = [n for n in SHAPES if n.endswith(("in_proj_weight", "out_proj.weight", "c_fc.weight", "c_proj.weight"))]


def _numel(n):
    return int(np.prod(SHAPES[n])) if SHAPES[n] else 1


def _layout():
    offsets, off = {}, 0
    for n in SHAPES:
        offsets[n] = off
        off += (_numel(n) + 63) // 64 * 64
    return offsets, off


def _covered(total, ranges):
    count = np.zeros(total, dtype=np.int32)
    for lo, hi in ranges:
        count[lo:hi] += 1
    return count


PATTERNS = {
    "none frozen": lambda n: True,
    "some frozen": lambda n: n not in ("visual.conv1.weight", "visual.transformer.resblocks.1.attn.in_proj_weight",
                                       "transformer.resblocks.0.ln_2.bias", "token_embedding.weight", "logit_scale"),
    "image tower frozen": lambda n: not n.startswith("visual."),
    "text: top block only": lambda n: n.startswith("visual.") or n in ("text_projection", "ln_final.weight", "logit_scale") or
    n.startswith("transformer.resblocks.1."),
}


@pytest.mark.parametrize("pattern", list(PATTERNS))
@pytest.mark.parametrize("tiles", [True, False])
def test_plan_tables_cover_exactly_the_trainable_elements(pattern, tiles):
    """Tile jobs and segments together cover every element of every trainable tensor exactly once, the chunk table covers the same
    set, and no element of a frozen tensor (its padding included) is in either.  Beyond the tensors the tables hold nothing but
    the round-up of a trainable tensor's end to a multiple of 4 -- at most three elements of that tensor's own padding, which the
    16-byte kernels need (``logit_scale`` is one element long).  Segments are multiples of 4 of at most 2048 elements, chunks of at
    most 65536; the group of a tile job and of a segment is its name's."""
    from clip_event_amd.model import trainable_tables
    offsets, total = _layout()
    flags = {n: PATTERNS[pattern](n) for n in SHAPES}
    group_of = {n: (1 if len(SHAPES[n]) < 2 else 2 if n.startswith("visual.") else 0) for n in SHAPES}
    t = trainable_tables(offsets, SHAPES, flags, group_of, TILE_NAMES if tiles else [])
    assert [n for n, _ in t["tiles"]] == [n for n in (TILE_NAMES if tiles else []) if flags[n]]
    assert all(g == group_of[n] for n, g in t["tiles"])
    tile_ranges = [(offsets[n], offsets[n] + _numel(n)) for n, _ in t["tiles"]]
    want = np.zeros(total, dtype=np.int32)
    allowed = np.zeros(total, dtype=np.int32)
    for n in SHAPES:
        if flags[n]:
            want[offsets[n]:offsets[n] + _numel(n)] = 1
            allowed[offsets[n]:offsets[n] + (_numel(n) + 3) // 4 * 4] = 1
    for got in (_covered(total, tile_ranges + t["segments"]), _covered(total, t["chunks"])):
        assert got.max() <= 1                                  # once each
        assert bool((got >= want).all())                       # every trainable element
        assert bool((got <= allowed).all())                    # nothing frozen, no padding beyond the round-up to 4
    assert all((hi - lo) % 4 == 0 and lo % 4 == 0 and 0 < hi - lo <= 2048 for lo, hi in t["segments"])
    assert all((hi - lo) % 4 == 0 and 0 < hi - lo <= (1 << 16) for lo, hi in t["chunks"])
    assert len(t["segment_group"]) == len(t["segments"])
    owner = np.full(total, -1)
    for n in SHAPES:
        owner[offsets[n]:offsets[n] + 64 * ((_numel(n) + 63) // 64)] = group_of[n]
    assert all(owner[lo] == g and owner[hi - 1] == g for (lo, hi), g in zip(t["segments"], t["segment_group"]))
    if flags["token_embedding.weight"]:
        assert sum(1 for lo, hi in t["chunks"] if lo >= offsets["token_embedding.weight"]) == 2       # 66000 elements: two chunks


def test_plan_locked_and_stop_layer():
    from clip_event_amd.model import trainable_tables
    offsets, _ = _layout()

    def plan(pred):
        t = trainable_tables(offsets, SHAPES, {n: pred(n) for n in SHAPES}, None, TILE_NAMES)
        return t["locked"], t["stop_layer"]

    assert plan(lambda n: True) == ({"visual": False, "text": False}, {"visual": 0, "text": 0})
    locked, stop = plan(PATTERNS["image tower frozen"])
    assert locked == {"visual": True, "text": False} and stop == {"visual": 2, "text": 0}
    locked, stop = plan(PATTERNS["text: top block only"])
    assert locked == {"visual": False, "text": False} and stop == {"visual": 0, "text": 1}
    # an input-side parameter alone keeps the whole backward: its gradient comes out of block 0
    locked, stop = plan(lambda n: n == "positional_embedding")
    assert locked == {"visual": True, "text": False} and stop["text"] == 0
    locked, stop = plan(lambda n: n == "visual.class_embedding")
    assert not locked["visual"] and stop["visual"] == 0
    # only the output side: no block runs
    locked, stop = plan(lambda n: n in ("text_projection", "visual.ln_post.weight"))
    assert locked == {"visual": False, "text": False} and stop == {"visual": 2, "text": 2}
    # a gain of block 0 alone: the backward runs down to block 0 (0 also stands for "the input side runs": its results go unused)
    assert plan(lambda n: n == "visual.transformer.resblocks.0.ln_1.bias")[1]["visual"] == 0
    locked, stop = plan(lambda n: n == "logit_scale")
    assert locked == {"visual": True, "text": True}


def _clip():
    from clip_event_amd.model import build_model
    return build_model({k: v.clone() for k, v in O.init_params(CFG, 3).items()})


def test_lock_helpers_set_flags_only():
    """open_clip's spelling: the tower frozen except its top ``unlocked_layers`` blocks, with which the output side stays
    trainable; the plan of a model on the host knows the towers."""
    m = _clip()
    m.lock_image_tower()
    live = {n for n, p in m.named_parameters() if p.requires_grad}
    assert not any(n.startswith("visual.") for n in live) and "logit_scale" in live and "text_projection" in live
    plan = m.trainable_plan()
    assert plan.locked == {"visual": True, "text": False} and plan.stop_layer["text"] == 0 and not plan.plain
    m.lock_text_tower(unlocked_layers=1)
    live = {n for n, p in m.named_parameters() if p.requires_grad}
    text = {n for n in live if n != "logit_scale"}
    assert text == {n for n, _ in m.named_parameters() if n.startswith(("transformer.resblocks.2.", "ln_final.")) or n == "text_projection"}
    plan = m.trainable_plan()
    assert plan.locked == {"visual": True, "text": False} and plan.stop_layer == {"visual": 2, "text": 2}
    assert m.trainable_plan() is plan                           # cached until a flag changes
    m.lock_image_tower(unlocked_layers=5)                       # more than there are: the blocks and the output side, not the input side
    assert m.trainable_plan() is not plan
    assert m.trainable_plan().stop_layer["visual"] == 0 and not m.visual.conv1.weight.requires_grad
    assert m.visual.proj.requires_grad and m.visual.transformer.resblocks[0].ln_1.weight.requires_grad
    for p in m.parameters():
        p.requires_grad_(True)
    assert m.trainable_plan().plain


def test_group_rules_and_no_decay_groups():
    from clip_event_amd.optim import FusedAdam, FusedSGD, build_optimizer, no_decay_groups
    m = _clip()
    names = [n for n, _ in m.named_parameters()]
    gains = [n for n in names if "ln_" in n]
    for cls in (FusedAdam, FusedSGD):
        with pytest.raises(ValueError, match="no parameter"):
            cls(m, groups=[{"params": ["visual.nothing"], "lr": 1e-3}])
        with pytest.raises(ValueError, match="in groups 0 and 1"):
            cls(m, groups=[{"params": gains}, {"params": gains[:1]}])
        with pytest.raises(ValueError, match="at most 8"):
            cls(m, groups=[{"params": [n]} for n in names[:9]])
        with pytest.raises(ValueError, match="at most 8"):
            cls(m, groups=[{"params": [n]} for n in names[:8]])         # eight named + the unnamed parameters' group
        with pytest.raises(ValueError, match="shared"):
            cls(m, groups=[{"params": gains, "betas": (0.8, 0.9)}])
        with pytest.raises(ValueError, match="shared"):
            cls(m, groups=[{"params": gains, "momentum": 0.5}])
    with pytest.raises(ValueError, match="shared"):
        FusedSGD(m, groups=[{"params": gains, "decoupled": True}])
    m.visual.conv1.weight.requires_grad_(False)
    with pytest.raises(ValueError, match="frozen"):
        FusedAdam(m, groups=[{"params": ["visual.conv1.weight"], "lr": 1e-3}])
    # groups are real param groups over the trainable parameters; the unnamed ones come first, with the constructor's values
    opt = FusedAdam(m, lr=1e-3, weight_decay=0.1, groups=[{"params": gains, "weight_decay": 0.0},
                                                         {"params": [m.text_projection], "lr": 1e-4, "decoupled": True}])
    assert [len(g["params"]) for g in opt.param_groups] == [len(names) - 1 - len(gains) - 1, len(gains), 1]
    assert [(g["lr"], g["weight_decay"], g["decoupled_weight_decay"]) for g in opt.param_groups] == \
        [(1e-3, 0.1, False), (1e-3, 0.0, False), (1e-4, 0.1, True)]
    assert all(p.requires_grad for g in opt.param_groups for p in g["params"])
    assert all(g["betas"] == (0.9, 0.999) for g in opt.param_groups)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda it: 0.5)
    assert [g["lr"] for g in opt.param_groups] == [5e-4, 5e-4, 5e-5] and sched is not None
    # one group, nothing frozen: the param group is what it was before groups existed
    for p in m.parameters():
        p.requires_grad_(True)
    assert set(FusedAdam(m).param_groups[0]) == {"params", "lr", "betas", "eps", "weight_decay"}
    assert "decoupled_weight_decay" in FusedAdam(m, decoupled=True).param_groups[0]
    # no_decay_groups: everything of one dimension or none, every bias and logit_scale
    m.lock_image_tower()
    decay, no_decay = no_decay_groups(m, 0.2)
    assert (decay["weight_decay"], no_decay["weight_decay"]) == (0.2, 0.0)
    live = {n: p for n, p in m.named_parameters() if p.requires_grad}
    assert set(decay["params"]) | set(no_decay["params"]) == set(live) and not set(decay["params"]) & set(no_decay["params"])
    assert "logit_scale" in no_decay["params"] and "positional_embedding" in decay["params"] and "token_embedding.weight" in decay["params"]
    assert all(live[n].ndim >= 2 for n in decay["params"]) and all(live[n].ndim < 2 for n in no_decay["params"])
    opt = FusedAdam(m, decoupled=True, groups=[decay, no_decay])
    assert len(opt.param_groups) == 2 and all(g["decoupled_weight_decay"] for g in opt.param_groups)
    # a CLIP with frozen parameters keeps the fused step, for both optimisers
    cfg = {"optimizer": "sgd", "lr": 0.1, "momentum": 0.9, "weight_decay": 0.01}
    assert type(build_optimizer(cfg, m)) is FusedSGD and type(build_optimizer(dict(cfg, optimizer="adam"), m)) is FusedAdam
    assert len(build_optimizer(cfg, m).param_groups[0]["params"]) == len(live)


class _Stub(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.a = torch.nn.Parameter(torch.zeros(4, 3))
        self.b = torch.nn.Parameter(torch.zeros(5))


def test_a_model_without_a_plan_is_still_refused():
    """Frozen parameters and groups need ``trainable_plan``: a bare module gets what it got before."""
    from clip_event_amd.optim import FusedAdam, FusedSGD, build_optimizer
    m = _Stub()
    for cls in (FusedAdam, FusedSGD):
        with pytest.raises(NotImplementedError, match="trainable_plan"):
            cls(m, groups=[{"params": ["b"], "weight_decay": 0.0}])
    m.b.requires_grad_(False)
    for cls in (FusedAdam, FusedSGD):
        with pytest.raises(NotImplementedError, match="frozen"):
            cls(m)
    stock = build_optimizer({"optimizer": "sgd", "lr": 0.1, "momentum": 0.9, "weight_decay": 0.01}, m)
    assert type(stock) is torch.optim.SGD and len(stock.param_groups[0]["params"]) == 1


class _Group(ctypes.Structure):
    _fields_ = [("lr", c_float), ("weight_decay", c_float), ("decoupled", c_int), ("pad_", c_int)]


def test_grouped_entry_points_check_arguments_without_a_gpu():
    """-EINVAL with a message of its own before any launch: a call that passed validation would launch on the fake pointers."""
    from clip_event_amd._lib import lib
    from clip_event_amd.optim import OptimGroup
    assert ctypes.sizeof(OptimGroup) == ctypes.sizeof(_Group) == 16
    cl = lib()
    fake, null = c_void_p(0x1000), c_void_p(0)
    groups = (_Group * 9)(*[_Group(0.1, 0.0, 0, 0) for _ in range(9)])
    dec = (_Group * 2)(_Group(0.1, 0.0, 0, 0), _Group(0.1, 0.1, 1, 0))

    def adam(jobs=fake, njobs=1, tiles=1, segs=fake, nseg=1, g=groups, ng=1, step=1, m=fake):
        return cl.ce_adam_step_groups(fake, fake, m, fake, fake, jobs, c_int(njobs), c_int(tiles), segs, c_int(nseg), null, null,
                                      c_float(1.0), g, c_int(ng), c_float(0.9), c_float(0.999), c_float(1e-8), c_int(step), None)

    def sgd(jobs=fake, njobs=1, tiles=1, segs=fake, nseg=1, g=groups, ng=1, mu=0.9, damp=0.0, nesterov=0, buf=fake):
        return cl.ce_sgd_step_groups(fake, fake, buf, fake, jobs, c_int(njobs), c_int(tiles), segs, c_int(nseg), null, null,
                                     c_float(1.0), g, c_int(ng), c_float(mu), c_float(damp), c_int(nesterov), c_int(1), None)

    cases = [
        (lambda: adam(ng=0), b"ce_adam_step_groups", b"groups"),
        (lambda: adam(ng=9), b"ce_adam_step_groups", b"groups"),
        (lambda: adam(g=null), b"ce_adam_step_groups", b"groups"),
        (lambda: adam(njobs=0, tiles=0, nseg=0), b"ce_adam_step_groups", b"nothing to update"),
        (lambda: adam(jobs=null, segs=null), b"ce_adam_step_groups", b"nothing to update"),
        (lambda: adam(step=0), b"ce_adam_step_groups", b"step"),
        (lambda: adam(m=null), b"ce_adam_step_groups", b"null buffer"),
        (lambda: sgd(ng=0), b"ce_sgd_step_groups", b"groups"),
        (lambda: sgd(ng=9), b"ce_sgd_step_groups", b"groups"),
        (lambda: sgd(g=null), b"ce_sgd_step_groups", b"groups"),
        (lambda: sgd(g=dec, ng=2), b"ce_sgd_step_groups", b"decoupled"),
        (lambda: sgd(njobs=0, tiles=0, nseg=0), b"ce_sgd_step_groups", b"nothing to update"),
        (lambda: sgd(jobs=null, segs=null), b"ce_sgd_step_groups", b"nothing to update"),
        (lambda: sgd(mu=-0.5), b"ce_sgd_step_groups", b"invalid momentum"),
        (lambda: sgd(mu=0.0, nesterov=1), b"ce_sgd_step_groups", b"nesterov"),
        (lambda: sgd(buf=null), b"ce_sgd_step_groups", b"momentum buffer"),
        (lambda: cl.ce_sumsq_segments(fake, fake, c_int(0), fake, None), b"ce_sumsq_segments", b"empty"),
        (lambda: cl.ce_sumsq_segments(fake, null, c_int(3), fake, None), b"ce_sumsq_segments", b"empty"),
        (lambda: cl.ce_sumsq_segments(null, fake, c_int(3), fake, None), b"ce_sumsq_segments", b"empty"),
        (lambda: cl.ce_sumsq_segments(fake, fake, c_int(3), null, None), b"ce_sumsq_segments", b"empty"),
    ]
    for i, (call, who, msg) in enumerate(cases):
        rc = call()
        assert rc == -22, (i, rc)
        err = cl.ce_last_error()
        assert who in err and msg in err, (i, err)


# ---- GradSync with a locked tower (two gloo ranks on the host, tests/test_distributed_cpu.py's stand-in) ------------------------

def _locked_gradsync_worker(rank, W, port, out):
    import os
    import types

    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=W)
    from clip_event_amd import distributed as D
    from tests.test_distributed_cpu import _FlatStandIn
    m = _FlatStandIn()
    m.trainable_plan = lambda: types.SimpleNamespace(locked={"visual": True, "text": False})
    sync = D.GradSync(m, pieces_per_tower=3)
    va, vb = m._ranges["visual"]
    ta, tb = m._ranges["text"]
    m._flat_grad[va:vb] = 100.0 + rank                           # whatever a locked tower's range holds: nobody reads it
    m._flat_grad[0] = float(rank + 1)                            # logit_scale
    sync.note_forward("text")                                    # a locked tower announces no forward (CLIP._note_pass)
    m.backward_pass("text", torch.arange(tb - ta, dtype=torch.float32) * (rank + 1))
    sync.finish()
    assert not sync.pending and not sync.dirty
    gathered = [None] * W
    dist.all_gather_object(gathered, m._flat_grad.clone())
    if rank == 0:
        torch.save(gathered, out)
    dist.destroy_process_group()


@pytest.mark.timeout(120)
def test_gradsync_leaves_a_locked_towers_range_alone(tmp_path):
    """``finish()`` neither waits for nor exchanges the range of a tower the model's plan calls locked: it keeps every rank's own
    values, while the other tower's range and the head are averaged as before."""
    import torch.multiprocessing as mp
    from tests.test_distributed_cpu import _FlatStandIn, _free_port
    W = 2
    out = str(tmp_path / "g.pt")
    mp.spawn(_locked_gradsync_worker, args=(W, _free_port(), out), nprocs=W, join=True)
    gathered = torch.load(out, weights_only=False)               # written by this test
    m = _FlatStandIn()
    va, vb = m._ranges["visual"]
    ta, tb = m._ranges["text"]
    for r in range(W):
        assert bool((gathered[r][va:vb] == 100.0 + r).all()), r
        assert torch.allclose(gathered[r][ta:tb], torch.arange(tb - ta, dtype=torch.float32) * 1.5), r
        assert float(gathered[r][0]) == 1.5
