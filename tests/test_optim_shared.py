"""What the fused optimisers share, whatever the update rule (csrc/optim.hip: one flat, one tile and one segment traversal
instantiated per rule; optim._FusedFlatOptimizer: one ``step()``): the three kernel forms give the same bits at op level, and
``step()`` polls the fp16-stream saturation counters on its sharded exit too."""
import types
from ctypes import c_float, c_int, c_long, c_void_p

import pytest
import torch

from tests.test_embed_optim_ops import (ADAM_GRID, B1, B2, DEV, EPS, LR, MAX_NORM, TILE_MATS, TILE_N, TILE_SEGS, _adam_state, _dev,
                                        _lib)
from tests.test_sgd_ops import SGD_GRID, _call_flat, _call_tiles, _job_table

gpu = pytest.mark.gpu


def _null(t):
    return c_void_p(t.data_ptr()) if t is not None else c_void_p(0)


class _Sgd:
    """clip + SGD at op level; ``state`` is [buf], which momentum 0 leaves alone (the kernel gets NULL)."""
    names = ("momentum_buffer",)

    def __init__(self, momentum):
        self.cases = [(clip, wd, step, var) for clip, wd, step, var in SGD_GRID if (var[1] != 0) == momentum]

    def state0(self, n, case, seed):
        clip, _, step, _ = case
        p, g, buf, _, sumsq = _adam_state(n, step, clip, seed)
        return p, g, [buf], sumsq

    def flat(self, cl, ptr, stream, case, p, g, state, p16, n, ss):
        _, wd, step, (_, mu, damp, nesterov) = case
        return _call_flat(cl, ptr, stream, p, g, state[0] if mu != 0 else None, p16, n, ss, wd, mu, damp, nesterov, step == 1)

    def tiles(self, cl, ptr, stream, case, p, g, state, p16, tab, njobs, tiles, seg_tab, ss):
        _, wd, step, (_, mu, damp, nesterov) = case
        return _call_tiles(cl, ptr, stream, p, g, state[0] if mu != 0 else None, p16, tab, njobs, tiles, seg_tab, ss, wd, mu, damp,
                           nesterov, step == 1)


class _Adam:
    """clip + Adam at op level; ``state`` is [m, v]."""
    names = ("exp_avg", "exp_avg_sq")
    cases = ADAM_GRID

    def state0(self, n, case, seed):
        clip, _, step = case
        p, g, m, v, sumsq = _adam_state(n, step, clip, seed)
        return p, g, [m, v], sumsq

    def _tail(self, case, ss, stream):
        _, wd, step = case
        return (_null(ss), c_float(MAX_NORM), c_float(LR), c_float(B1), c_float(B2), c_float(EPS), c_float(wd), c_int(step), stream())

    def flat(self, cl, ptr, stream, case, p, g, state, p16, n, ss):
        return cl.ce_adam_step(ptr(p), ptr(g), ptr(state[0]), ptr(state[1]), ptr(p16), c_long(n), *self._tail(case, ss, stream))

    def tiles(self, cl, ptr, stream, case, p, g, state, p16, tab, njobs, tiles, seg_tab, ss):
        return cl.ce_adam_step_tiles(ptr(p), ptr(g), ptr(state[0]), ptr(state[1]), ptr(p16), _null(tab), c_int(njobs), c_int(tiles),
                                     ptr(seg_tab), c_int(seg_tab.shape[0]), *self._tail(case, ss, stream))


RULES = {"sgd_momentum": lambda: _Sgd(True), "sgd_plain": lambda: _Sgd(False), "adam": _Adam}


@gpu
@pytest.mark.parametrize("rule", sorted(RULES))
def test_tiled_flat_and_segment_forms_are_bit_identical(rule):
    """The three kernel forms update through one element function per rule: the flat kernel, the tile + segment launch and a
    launch of segments only (the whole range cut into chunks of at most 2048) leave the same bits in the masters, every state
    buffer and the bf16 mirror -- for SGD with momentum (plain, Nesterov, dampening), SGD without and Adam, over the grids of
    their fp64 tests (clip active / inactive / off x weight decay 0 / 0.1 x steps), on the layout of
    test_adam_step_tiles_against_fp64 (the ragged 72 x 200 matrix among the tiles).  The flat form runs over TILE_N + 3
    elements, so its length is no multiple of 4; the table forms cover TILE_N and must leave the three behind it alone."""
    cl, ptr, stream = _lib()
    r = RULES[rule]()
    N, n = TILE_N, TILE_N + 3
    seg_tab = torch.tensor(TILE_SEGS, dtype=torch.int64).to(DEV)
    all_segs = torch.tensor([(lo, min(lo + 2048, N)) for lo in range(0, N, 2048)], dtype=torch.int64).to(DEV)
    assert r.cases
    for case in r.cases:
        p0, g0, state0, sumsq = r.state0(n, case, 300 + case[2])
        out = {}
        for form in ("flat", "tiles", "segments"):
            p, g = _dev(p0, g0)
            state = _dev(*state0)
            p16 = torch.full((n,), 4.0, device=DEV, dtype=torch.bfloat16)
            ss = torch.tensor([sumsq], device=DEV) if sumsq is not None else None
            if form == "flat":
                rc = r.flat(cl, ptr, stream, case, p, g, state, p16, n, ss)
            elif form == "tiles":
                wts = [torch.empty((c, rows), device=DEV, dtype=torch.bfloat16) for _, rows, c in TILE_MATS]
                tab, tiles = _job_table(TILE_MATS, p16, wts)
                rc = r.tiles(cl, ptr, stream, case, p, g, state, p16, tab, len(TILE_MATS), tiles, seg_tab, ss)
            else:
                rc = r.tiles(cl, ptr, stream, case, p, g, state, p16, None, 0, 0, all_segs, ss)
            torch.cuda.synchronize()
            assert rc == 0, cl.ce_last_error()
            out[form] = (p, *state, p16)
        start = (p0, *state0, torch.full((n,), 4.0, dtype=torch.bfloat16))
        for form in ("tiles", "segments"):
            for i, what in enumerate(("masters", *r.names, "bf16 mirror")):
                a, b = out[form][i], out["flat"][i]
                assert torch.equal(a[:N], b[:N]), (rule, case, form, what, int((a[:N] != b[:N]).sum()))
                assert torch.equal(a[N:].cpu(), start[i][N:]), (rule, case, form, what)
        assert bool((out["flat"][-1][N:] != 4.0).all()), (rule, case)                   # the flat form did reach its ragged end


# ---- step(): the saturation poll on the sharded exit (no GPU) --------------------------------------------------------------------

class _FlatModel(torch.nn.Module):
    """What ``step()`` touches of the model: the flat buffers, the hooks around the update and a ``grad_sync.plan``."""

    def __init__(self, n=8):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(n))
        self._flat, self._flat_grad = torch.zeros(n), torch.ones(n)
        self._flat16 = torch.zeros(n, dtype=torch.bfloat16)
        self._offsets = {"w": 0}
        self.grad_sync = types.SimpleNamespace(plan=object())
        self.polls, self.stale = 0, []

    def _ready(self):
        pass

    def _settle_first_touch(self):
        pass

    def wait_transposes(self):
        pass

    def mark_operands_stale(self, **kw):
        self.stale.append(kw)

    def poll_stream16_saturation(self):
        self.polls += 1


class _RecordingLib:
    """Stands in for the shared library: every entry point records its name and succeeds."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append(name)
            return 0
        return entry


@pytest.mark.parametrize("which", ["FusedAdam", "FusedSGD"])
def test_sharded_step_polls_the_saturation_counters(monkeypatch, which):
    """With ``sat_poll_every=1`` a sharded ``step()`` (``grad_sync.plan`` set, the collectives active) ends with
    ``poll_stream16_saturation`` like every other step: once, after the range callbacks went through the flat entry point."""
    from clip_event_amd import distributed as D
    from clip_event_amd import optim
    fake = _RecordingLib()
    monkeypatch.setattr(optim, "lib", lambda: fake)
    monkeypatch.setattr(optim, "stream", lambda: None)
    monkeypatch.setattr(D, "active", lambda: True)
    seen = []

    def sharded_update(plan, params, sumsq, sumsq_fn, update_fn):
        seen.append((plan, params, sumsq))
        sumsq_fn(0, 4)
        update_fn(0, 4)
    monkeypatch.setattr(D, "sharded_update", sharded_update)
    m = _FlatModel()
    opt = optim.FusedAdam(m) if which == "FusedAdam" else optim.FusedSGD(m, momentum=0.9)
    opt.sat_poll_every = 1
    opt.step()
    assert m.polls == 1
    assert len(seen) == 1 and all(a is b for a, b in zip(seen[0], (m.grad_sync.plan, m._flat, opt.sumsq)))
    assert fake.calls == ["ce_sumsq", "ce_adam_step" if which == "FusedAdam" else "ce_sgd_step"]
    assert m.stale == [dict(mirror_fresh=False)] and opt._moments_stale and opt.step_count == 1
