"""CPU: what the fused head's Python side decides without a GPU -- the library calls every head node makes (names, integer
arguments, which buffers alias), the route ``engine.head_route`` picks for every criterion on both sides of each threshold, and
the split choice as the ``*_workspace_bytes`` entry points expose it."""
import itertools

import pytest
import torch

NA, NB, E, ET = 5, 7, 128, 256
SEL = [0, 2, 6]                                  # query rows of the second direction


class Recorder:
    """Stands in for the loaded library: records (name, arguments), returns 0 (4096 from a ``*_bytes`` function)."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            return 4096 if name.endswith("_bytes") else 0
        return fn

    def names(self):
        return [name for name, _ in self.calls]

    def ints(self, name):
        """The integer arguments of every call of ``name``, in call order."""
        return [[a for a in args if isinstance(a, int)] for n, args in self.calls if n == name]

    def pointers(self, name):
        """The pointer arguments (None: a null pointer, or the stream stub) of every call of ``name`` by position, in call order."""
        return [[getattr(a, "value", None) for a in args] for n, args in self.calls if n == name]


@pytest.fixture
def rec(monkeypatch):
    from clip_event_amd import functional
    r = Recorder()
    monkeypatch.setattr(functional, "lib", lambda: r)
    monkeypatch.setattr(functional, "stream", lambda: None)
    return r


def _inputs():
    g = torch.Generator().manual_seed(0)
    a = torch.randn(NA, E, generator=g, requires_grad=True)
    b = torch.randn(NB, E, generator=g, requires_grad=True)
    ls = torch.tensor(2.0, requires_grad=True)
    return a, b, ls, torch.arange(NA), torch.arange(NB) % NA, torch.tensor(SEL)


def _split(rec):
    """(forward names, backward names) around the first backward call."""
    names = rec.names()
    cut = next(i for i, n in enumerate(names) if n.endswith("_bwd") and n != "ce_l2norm_bwd")
    return names[:cut], names[cut:]


def test_infonce_one_direction_calls(rec):
    from clip_event_amd.functional import InfoNCEFn
    a, b, ls, ya, _, _ = _inputs()
    loss = InfoNCEFn.apply(a, b, ls, ya, None)
    assert loss.shape == ()
    loss.backward()
    fwd, bwd = _split(rec)
    assert fwd == ["ce_l2norm_fwd", "ce_l2norm_fwd", "ce_infonce_workspace_bytes", "ce_infonce_fwd"]
    assert bwd == ["ce_infonce_bwd", "ce_l2norm_bwd", "ce_l2norm_bwd"]
    assert rec.ints("ce_l2norm_fwd") == [[128, 128, 5, 128], [128, 128, 7, 128]]
    assert rec.ints("ce_infonce_workspace_bytes") == [[5]]
    assert rec.ints("ce_infonce_fwd") == [[128, 5, 128, 7, 128]]
    assert rec.ints("ce_infonce_bwd") == [[128, 5, 128, 7, 128]]
    assert rec.ints("ce_l2norm_bwd") == [[128, 128, 128, 5, 128, 0], [128, 128, 128, 7, 128, 0]]
    assert rec.pointers("ce_infonce_fwd")[0][2] is None                      # no query gather
    assert a.grad.shape == (NA, E) and b.grad.shape == (NB, E) and ls.grad.shape == ()


def test_infonce_one_direction_with_a_query_gather(rec):
    from clip_event_amd.functional import InfoNCEFn
    a, b, ls, _, yb, sel = _inputs()
    InfoNCEFn.apply(b, a, ls, yb, sel).backward()
    assert rec.ints("ce_infonce_workspace_bytes") == [[3]]
    assert rec.ints("ce_infonce_fwd") == [[128, 3, 128, 5, 128]]
    assert rec.ints("ce_infonce_bwd") == [[128, 3, 128, 5, 128]]
    assert rec.pointers("ce_infonce_fwd")[0][2] is not None


def test_infonce_pair_calls_and_aliasing(rec):
    from clip_event_amd.functional import InfoNCEFn
    a, b, ls, ya, yb, sel = _inputs()
    li, lt = InfoNCEFn.apply(a, b, ls, ya, None, yb, sel)
    (li + lt).backward()
    fwd, bwd = _split(rec)
    assert fwd == ["ce_l2norm_fwd", "ce_l2norm_fwd", "ce_infonce_workspace_bytes", "ce_infonce_fwd", "ce_infonce_fwd"]
    assert bwd == ["ce_infonce_bwd", "ce_infonce_bwd", "ce_l2norm_bwd", "ce_l2norm_bwd"]
    assert rec.ints("ce_l2norm_fwd") == [[128, 128, 5, 128], [128, 128, 7, 128]]
    assert rec.ints("ce_infonce_workspace_bytes") == [[5]]
    assert rec.ints("ce_infonce_fwd") == [[128, 5, 128, 7, 128], [128, 3, 128, 5, 128]]
    assert rec.ints("ce_infonce_bwd") == [[128, 5, 128, 7, 128], [128, 3, 128, 5, 128]]
    assert rec.ints("ce_l2norm_bwd") == [[128, 128, 128, 5, 128, 0], [128, 128, 128, 7, 128, 0]]
    # ce_infonce_fwd(q, ldq, sel, nq, k, ldk, nk, E, logit_scale, labels, lse, loss, workspace, stream)
    fi, ft = rec.pointers("ce_infonce_fwd")
    assert fi[0] == ft[4] and fi[4] == ft[0]                              # each matrix normalised once
    assert fi[12] == ft[12] and fi[12] is not None                   # one workspace
    assert fi[2] is None and ft[2] is not None
    assert ft[11] == fi[11] + 4                                           # the two losses: neighbours in one buffer
    # ce_infonce_bwd(q, ldq, sel, nq, k, ldk, nk, E, logit_scale, labels, lse, grad, dq, dk, dlogit_scale, stream)
    bi, bt = rec.pointers("ce_infonce_bwd")
    assert bt[12] == bi[13] and bt[13] == bi[12] and bi[12] != bi[13]     # one gradient buffer per matrix
    assert bi[14] == bt[14]                                               # one logit_scale slot
    assert bi[13] == bi[12] + NA * E * 4 and bi[14] == bi[13] + NB * E * 4          # dq | dk | scalars: one fill
    lb = rec.pointers("ce_l2norm_bwd")
    assert lb[0][0] == bi[12] and lb[1][0] == bi[13]


def test_sigmoid_calls(rec):
    from clip_event_amd.functional import SigmoidHeadFn
    a, b, ls, ya, _, _ = _inputs()
    bias = torch.tensor(-10.0, requires_grad=True)
    SigmoidHeadFn.apply(a, b, ls, bias, ya, None).backward()
    fwd, bwd = _split(rec)
    assert fwd == ["ce_l2norm_fwd", "ce_l2norm_fwd", "ce_sigmoid_head_workspace_bytes", "ce_sigmoid_head_fwd"]
    assert bwd == ["ce_sigmoid_head_bwd", "ce_l2norm_bwd", "ce_l2norm_bwd"]
    assert rec.ints("ce_sigmoid_head_workspace_bytes") == [[5, 7]]
    assert rec.ints("ce_sigmoid_head_fwd") == [[128, 5, 128, 7, 128]]
    assert rec.ints("ce_sigmoid_head_bwd") == [[128, 5, 128, 7, 128]]
    assert rec.ints("ce_l2norm_bwd") == [[128, 128, 128, 5, 128, 0], [128, 128, 128, 7, 128, 0]]
    # ce_sigmoid_head_bwd(q, ldq, sel, nq, k, ldk, nk, E, scale, bias, labels, grad, dq, dk, dlogit_scale, dlogit_bias, stream)
    p = rec.pointers("ce_sigmoid_head_bwd")[0]
    assert p[13] == p[12] + NA * E * 4 and p[14] == p[13] + NB * E * 4 and p[15] == p[14] + 4
    assert bias.grad.shape == () and ls.grad.shape == ()


def test_sigmoid_both_directions_share_the_gradient_buffers(rec):
    from clip_event_amd.functional import SigmoidHeadFn
    a, b, ls, ya, yb, sel = _inputs()
    bias = torch.tensor(-10.0, requires_grad=True)
    l0, l1 = SigmoidHeadFn.apply(a, b, ls, bias, ya, None, yb, sel)
    (l0 + l1).backward()
    assert rec.ints("ce_sigmoid_head_workspace_bytes") == [[5, 7], [3, 5]]
    assert rec.ints("ce_sigmoid_head_fwd") == [[128, 5, 128, 7, 128], [128, 3, 128, 5, 128]]
    assert rec.ints("ce_sigmoid_head_bwd") == [[128, 5, 128, 7, 128], [128, 3, 128, 5, 128]]
    p0, p1 = rec.pointers("ce_sigmoid_head_bwd")
    assert p1[12] == p0[13] and p1[13] == p0[12] and p0[14] == p1[14] and p0[15] == p1[15]
    assert rec.names().count("ce_l2norm_fwd") == 2 and rec.names().count("ce_l2norm_bwd") == 2


def _teacher():
    g = torch.Generator().manual_seed(1)
    return torch.randn(NA, ET, generator=g), torch.randn(NB, ET, generator=g), torch.tensor(4.605)


def test_distill_pair_calls_and_aliasing(rec):
    from clip_event_amd.functional import DistillHeadFn
    a, b, ls, _, _, sel = _inputs()
    ta, tb, tls = _teacher()
    li, lt = DistillHeadFn.apply(a, b, ls, ta, tb, tls, None, True, sel)
    (li + lt).backward()
    fwd, bwd = _split(rec)
    assert fwd == ["ce_l2norm_fwd"] * 4 + ["ce_distill_head_workspace_bytes", "ce_distill_head_fwd", "ce_distill_head_fwd"]
    assert bwd == ["ce_distill_head_bwd", "ce_distill_head_bwd", "ce_rowdot_sum", "ce_l2norm_bwd", "ce_l2norm_bwd"]
    assert rec.ints("ce_l2norm_fwd") == [[128, 128, 5, 128], [128, 128, 7, 128], [256, 256, 5, 256], [256, 256, 7, 256]]
    assert rec.ints("ce_distill_head_workspace_bytes") == [[5]]
    assert rec.ints("ce_distill_head_fwd") == [[128, 5, 128, 7, 128, 256, 256, 256], [128, 3, 128, 5, 128, 256, 256, 256]]
    assert rec.ints("ce_distill_head_bwd") == [[128, 5, 128, 7, 128, 256, 256, 256], [128, 3, 128, 5, 128, 256, 256, 256]]
    assert rec.ints("ce_rowdot_sum") == [[128, 128, 5, 128]]
    assert rec.ints("ce_l2norm_bwd") == [[128, 128, 128, 5, 128, 0], [128, 128, 128, 7, 128, 0]]
    # ce_distill_head_fwd(q, ldq, sel, nq, k, ldk, nk, Es, scale, tq, ldtq, tk, ldtk, Et, tscale, lse_s, lse_t, v, loss, ws, stream)
    fi, ft = rec.pointers("ce_distill_head_fwd")
    assert fi[0] == ft[4] and fi[4] == ft[0] and fi[9] == ft[11] and fi[11] == ft[9]          # student and teacher: normalised once
    assert fi[19] == ft[19] and fi[19] is not None                   # one workspace
    assert fi[2] is None and ft[2] is not None
    # ce_distill_head_bwd(..., tscale, lse_s, lse_t, v, grad, dq, dk, stream)
    bi, bt = rec.pointers("ce_distill_head_bwd")
    assert bt[19] == bi[20] and bt[20] == bi[19] and bi[19] != bi[20]
    assert (bi[15], bi[16], bi[17]) == (fi[15], fi[16], fi[17]) and (bt[15], bt[16], bt[17]) == (ft[15], ft[16], ft[17])
    # ce_rowdot_sum(x, ldx, y, ldy, n, E, out, stream): <a^, da^> over the accumulated buffer, into the scalar slot behind both
    rd = rec.pointers("ce_rowdot_sum")[0]
    assert rd[0] == fi[0] and rd[2] == bi[19] and rd[6] == bi[20] + NB * E * 4


def test_distill_one_direction_calls(rec):
    from clip_event_amd.functional import DistillHeadFn
    a, b, ls, _, _, sel = _inputs()
    ta, tb, tls = _teacher()
    loss = DistillHeadFn.apply(b, a, ls, tb, ta, tls, sel)
    assert loss.shape == ()
    loss.backward()
    fwd, bwd = _split(rec)
    assert fwd == ["ce_l2norm_fwd"] * 4 + ["ce_distill_head_workspace_bytes", "ce_distill_head_fwd"]
    assert bwd == ["ce_distill_head_bwd", "ce_rowdot_sum", "ce_l2norm_bwd", "ce_l2norm_bwd"]
    assert rec.ints("ce_distill_head_workspace_bytes") == [[3]]
    assert rec.ints("ce_distill_head_fwd") == [[128, 3, 128, 5, 128, 256, 256, 256]]
    assert rec.ints("ce_distill_head_bwd") == [[128, 3, 128, 5, 128, 256, 256, 256]]
    assert rec.ints("ce_rowdot_sum") == [[128, 128, 7, 128]]


def test_distill_refuses_teacher_rows_that_do_not_match(rec):
    from clip_event_amd.functional import DistillHeadFn
    a, b, ls, _, _, _ = _inputs()
    ta, tb, tls = _teacher()
    with pytest.raises(RuntimeError, match="do not match the student"):
        DistillHeadFn.apply(a, b, ls, tb, tb, tls, None)
    assert rec.calls == []


# ---- the router -------------------------------------------------------------------------------------------------------------

def _route(kind, **kw):
    from clip_event_amd.engine import head_route
    args = dict(rows=256, keys=256, width=512)
    args.update(kw)
    return head_route(kind, **args)


def test_route_ce_thresholds_and_forces():
    big, below = dict(rows=256, keys=512), dict(rows=256, keys=511)      # 2^17 logits, and one key row fewer
    assert _route("ce", **big) == "fused"
    assert _route("ce", **below) == "logits"
    assert _route("ce", **below, small_ok=True) == "small"
    assert _route("ce", rows=255, keys=512, small_ok=True) == "small"                  # one query row fewer
    assert _route("ce", **big, small_ok=True) == "fused"
    assert _route("ce", **below, fused_env="1", small_ok=True) == "fused"
    assert _route("ce", **big, fused_env="0") == "logits"
    assert _route("ce", **below, fused_env="0", small_ok=True) == "logits"             # a forced value switches the small head off too
    assert _route("ce", **below, small_env="0", small_ok=True) == "logits"
    assert _route("ce", **big, small_env="0") == "fused"
    assert _route("ce", **below, small_ok=True, has_index_pos=False) == "logits"
    assert _route("ce", **big, width=500) == "logits"                                  # a width the fused head does not take
    assert _route("ce", **big, width=500, small_ok=True) == "small"
    assert _route("ce", **big, width=1152, fused_env="1") == "logits"
    assert _route("ce", **big, overbatch=False) == "logits"                            # the per-instance layout
    assert _route("ce", **big, overbatch=False, fused_env="1", small_ok=True) == "logits"


def test_route_ce_global_batch_counts_every_rank():
    # 64 local images x 256 local texts x 8 ranks = 2^17: the caller passes keys = local texts x world size
    assert _route("ce", rows=64, keys=256 * 8, dist_global=True) == "fused"
    assert _route("ce", rows=64, keys=256 * 4, dist_global=True) == "logits"
    assert _route("ce", rows=64, keys=256 * 4, dist_global=True, small_ok=True) == "logits"       # never the small head across ranks
    assert _route("ce", rows=64, keys=256 * 4, dist_global=True, fused_env="1") == "fused"
    assert _route("ce", rows=64, keys=256 * 8, dist_global=True, fused_env="0") == "logits"


def test_route_sigmoid():
    for rows, keys in ((1, 1), (256, 256), (4096, 20480)):
        assert _route("sigmoid", rows=rows, keys=keys) == "fused"
        assert _route("sigmoid", rows=rows, keys=keys, fused_env="1") == "fused"
        assert _route("sigmoid", rows=rows, keys=keys, fused_env="0") == "logits"
        assert _route("sigmoid", rows=rows, keys=keys, small_ok=True) == "fused"
    assert _route("sigmoid", width=500) == "logits"
    assert _route("sigmoid", width=500, fused_env="1") == "logits"
    assert _route("sigmoid", dist_global=True) == "fused"


def test_route_distill_thresholds_and_forces():
    at, below = dict(rows=1 << 14, keys=1 << 14), dict(rows=(1 << 14) - 1, keys=1 << 14)         # 2^28 logits, one row fewer
    assert _route("distill", **at, teacher_width=768) == "fused"
    assert _route("distill", **below, teacher_width=768) == "logits"
    assert _route("distill", **below, teacher_width=768, fused_env="1") == "fused"
    assert _route("distill", **at, teacher_width=768, fused_env="0") == "logits"
    assert _route("distill", **at, teacher_width=700) == "logits"
    assert _route("distill", **at, width=500, teacher_width=768, fused_env="1") == "logits"
    assert _route("distill", **at, teacher_width=768, dist_global=True) == "fused"
    assert _route("distill", **below, teacher_width=768, small_ok=True) == "logits"


@pytest.mark.parametrize("kind", ["bce", "kl", None])
def test_route_other_criteria_always_take_logits(kind):
    for rows, keys, force, small, glob in itertools.product((16, 4096), (16, 20480), ("", "0", "1"), (False, True), (False, True)):
        assert _route(kind, rows=rows, keys=keys, fused_env=force, small_ok=small, dist_global=glob) == "logits"


# ---- the split choice, through the workspace sizes that expose it -------------------------------------------------------------

SIZES = (1, 31, 32, 33, 512, 4096, 20480)
MAX_SPLITS, HB = 64, 32


def _div_up(a, b):
    return (a + b - 1) // b


def _splits(nres, nstr, cap):
    """About two workgroups per CU (512 over the resident blocks), no more than the streamed blocks or ``cap``, at least 1."""
    return max(1, min(_div_up(512, _div_up(nres, HB)), _div_up(nstr, HB), cap))


def test_workspace_sizes_follow_the_split_choice():
    from clip_event_amd._lib import lib
    cl = lib()
    for nq, nk in itertools.product(SIZES, SIZES):
        assert cl.ce_sigmoid_head_workspace_bytes(nq, nk) == _div_up(nq, HB) * _splits(nq, nk, MAX_SPLITS) * 4, (nq, nk)
        for splits, k in itertools.product((0, 1, 3, 64), (1, 8, 10, 16)):
            rows = 32 * (512 + _div_up(nq, HB)) if splits == 0 else nq * min(splits, _div_up(nk, HB))
            bucket = 1 if k == 1 else (8 if k <= 8 else 16)
            assert cl.ce_score_topk_workspace_bytes(nq, nk, k, splits) == 4 * (nq + rows * (3 + 2 * bucket)), (nq, nk, k, splits)
    for nq in SIZES:
        assert cl.ce_infonce_workspace_bytes(nq) == MAX_SPLITS * nq * 2 * 4
        assert cl.ce_distill_head_workspace_bytes(nq) == MAX_SPLITS * nq * 2 * 4
    assert cl.ce_sigmoid_head_workspace_bytes(0, 5) == 0 and cl.ce_sigmoid_head_workspace_bytes(5, 0) == 0
