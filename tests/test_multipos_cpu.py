"""CPU (no GPU): the multi-positive (group-id) targets -- the fp64 reference against torch's own cross entropy, the group layout
of ``distributed.global_groups``, the route ``engine.head_route`` picks for "multipos", the library calls ``MultiPosHeadFn`` and
the group form of ``SigmoidHeadFn`` make (recorded on CPU tensors, the pattern of tests/test_head_calls_cpu.py), and
``CriterionSigmoid``'s default, which is what it was."""
import pytest
import torch
import torch.nn.functional as F

from tests.multipos_ref import multipos_loss_from_logits, positives, sigmoid_loss_from_logits

NA, NB, E = 5, 7, 128
SEL = [0, 2, 6]


# ---- the reference ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nq,nk", [(5, 7), (16, 48)])
def test_reference_is_cross_entropy_with_one_positive_per_row(nq, nk):
    g = torch.Generator().manual_seed(nq * 100 + nk)
    x = torch.randn(nq, nk, generator=g, dtype=torch.float64) * 6
    labels = torch.randperm(nk, generator=g)[:nq]
    gk = torch.full((nk,), -1, dtype=torch.int64)
    gk[labels] = torch.arange(nq) + 1000                   # every other key: nobody's positive
    ref = multipos_loss_from_logits(x, positives(torch.arange(nq) + 1000, gk))
    ce = F.cross_entropy(x, labels)
    assert abs(float(ref - ce)) <= 1e-12 * abs(float(ce))


@pytest.mark.parametrize("nq,nk", [(6, 12), (16, 48)])
def test_reference_is_soft_cross_entropy_against_the_uniform_set_target(nq, nk):
    """-(softmax(mask logits) * log_softmax(x)).sum(1).mean(): the mask logits are 0 on a row's positives and -inf elsewhere,
    so their softmax is uniform over the set.  Sets of one to four keys; every row has a positive."""
    g = torch.Generator().manual_seed(nq + nk)
    x = torch.randn(nq, nk, generator=g, dtype=torch.float64) * 6
    gq = torch.arange(nq)
    gk = torch.arange(nk) % nq                             # nk / nq keys per query, interleaved
    gk[-1] = 0
    pos = positives(gq, gk)
    assert int(pos.sum(1).min()) >= 1 and int(pos.sum(1).max()) >= 3
    mask_logits = torch.where(pos, torch.zeros_like(x), torch.full_like(x, float("-inf")))
    want = -(torch.softmax(mask_logits, dim=1) * torch.log_softmax(x, dim=1)).sum(1).mean()
    got = multipos_loss_from_logits(x, pos)
    assert abs(float(got - want)) <= 1e-12 * abs(float(want))


def test_reference_rows_without_positives_and_negative_ids():
    """-1 == -1 is no match; a row without a positive adds nothing and the divisor stays the row count."""
    x = torch.randn(4, 6, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    gq = torch.tensor([7, -1, 9, 5])
    gk = torch.tensor([7, -1, -1, 7, 3, 5])
    pos = positives(gq, gk)
    assert pos.tolist() == [[True, False, False, True, False, False], [False] * 6, [False] * 6,
                            [False, False, False, False, False, True]]
    lse = torch.logsumexp(x, 1)
    want = ((lse[0] - (x[0, 0] + x[0, 3]) / 2) + (lse[3] - x[3, 5])) / 4
    assert abs(float(multipos_loss_from_logits(x, pos) - want)) <= 1e-14
    # the sigmoid form: BCE-with-logits against the multi-hot target, times nk
    bce = F.binary_cross_entropy_with_logits(x, pos.double()) * 6
    assert abs(float(sigmoid_loss_from_logits(x, pos) - bce)) <= 1e-12 * abs(float(bce))


# ---- the layout ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rank", [0, 1])
@pytest.mark.parametrize("num_pos,num_neg", [(1, 0), (1, 2), (2, 2)])
def test_global_groups_follow_the_layout_formulas(num_pos, num_neg, rank):
    from clip_event_amd.distributed import global_groups, global_labels
    B, K = 3, num_pos + num_neg
    gi, gt, ip = global_groups(B, num_pos, num_neg, rank_=rank)
    assert gi.dtype == gt.dtype == torch.int64
    assert gi.tolist() == [rank * B + i for i in range(B)]
    assert gt.tolist() == [(rank * B + i) if j < num_pos else -1 for i in range(B) for j in range(K)]
    assert ip.tolist() == [i * K + j for i in range(B) for j in range(num_pos)]
    if (num_pos, num_neg) == (2, 2) and B >= 2:
        assert ip.tolist()[:4] == [0, 1, 4, 5]                     # dataset_voa.py:658-663
    if num_pos == 1:
        assert torch.equal(ip, global_labels(B, num_pos, num_neg, True, rank_=rank)[2])
    else:
        with pytest.raises(RuntimeError, match="description_num_pos == 1"):
            global_labels(B, num_pos, num_neg, True, rank_=rank)      # the refusal stays


# ---- the router ------------------------------------------------------------------------------------------------------------------

def _route(kind, **kw):
    from clip_event_amd.engine import head_route
    args = dict(rows=256, keys=256, width=512)
    args.update(kw)
    return head_route(kind, **args)


def test_route_multipos():
    for rows, keys in ((1, 1), (256, 256), (4096, 20480)):
        assert _route("multipos", rows=rows, keys=keys) == "fused"
        assert _route("multipos", rows=rows, keys=keys, fused_env="1") == "fused"
        assert _route("multipos", rows=rows, keys=keys, fused_env="0") == "logits"
        assert _route("multipos", rows=rows, keys=keys, small_ok=True) == "fused"      # never the three-launch head
    for width in (128, 1024):
        assert _route("multipos", width=width) == "fused"
    for width in (64, 500, 1152):                                                       # both sides of fused_head_ok
        assert _route("multipos", width=width) == "logits"
        assert _route("multipos", width=width, fused_env="1") == "logits"
        assert _route("multipos", width=width, small_ok=True) == "logits"
    assert _route("multipos", dist_global=True) == "fused"
    # the existing kinds route as before
    assert _route("ce", rows=256, keys=511, small_ok=True) == "small" and _route("ce", rows=256, keys=512) == "fused"
    assert _route("sigmoid") == "fused" and _route("sigmoid", fused_env="0") == "logits"


# ---- the recorded library calls --------------------------------------------------------------------------------------------------

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
        return [[a for a in args if isinstance(a, int)] for n, args in self.calls if n == name]

    def pointers(self, name):
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
    names = rec.names()
    cut = next(i for i, n in enumerate(names) if n.endswith("_bwd") and n != "ce_l2norm_bwd")
    return names[:cut], names[cut:]


def test_multipos_pair_calls_and_aliasing(rec):
    from clip_event_amd.functional import MultiPosHeadFn
    a, b, ls, ga, gb, sel = _inputs()
    li, lt = MultiPosHeadFn.apply(a, b, ls, ga, gb, None, True, sel)
    (li + lt).backward()
    fwd, bwd = _split(rec)
    assert fwd == ["ce_l2norm_fwd", "ce_l2norm_fwd", "ce_multipos_head_workspace_bytes", "ce_multipos_head_fwd", "ce_multipos_head_fwd"]
    assert bwd == ["ce_multipos_head_bwd", "ce_multipos_head_bwd", "ce_l2norm_bwd", "ce_l2norm_bwd"]
    assert rec.ints("ce_l2norm_fwd") == [[128, 128, 5, 128], [128, 128, 7, 128]]
    assert rec.ints("ce_multipos_head_workspace_bytes") == [[5]]
    assert rec.ints("ce_multipos_head_fwd") == [[128, 5, 128, 7, 128], [128, 3, 128, 5, 128]]
    assert rec.ints("ce_multipos_head_bwd") == [[128, 5, 128, 7, 128], [128, 3, 128, 5, 128]]
    assert rec.ints("ce_l2norm_bwd") == [[128, 128, 128, 5, 128, 0], [128, 128, 128, 7, 128, 0]]
    # ce_multipos_head_fwd(q, ldq, sel, nq, k, ldk, nk, E, logit_scale, qgroup, kgroup, lse, invpos, loss, workspace, stream)
    fi, ft = rec.pointers("ce_multipos_head_fwd")
    assert fi[0] == ft[4] and fi[4] == ft[0]                              # each matrix normalised once
    assert fi[9] == ft[10] and fi[10] == ft[9] and fi[9] != fi[10]        # the two id vectors, read the other way round
    assert fi[9] == ga.data_ptr() and fi[10] == gb.data_ptr()             # int64 already: no copy
    assert fi[14] == ft[14] and fi[14] is not None                        # one workspace
    assert fi[2] is None and ft[2] is not None
    assert ft[13] == fi[13] + 4                                           # the two losses: neighbours in one buffer
    assert fi[12] == fi[11] + NA * 4 and ft[12] == ft[11] + len(SEL) * 4  # lse | invpos per direction
    # ce_multipos_head_bwd(q, ldq, sel, nq, k, ldk, nk, E, logit_scale, qgroup, kgroup, lse, invpos, grad, dq, dk, dlogit_scale, stream)
    bi, bt = rec.pointers("ce_multipos_head_bwd")
    assert (bi[11], bi[12]) == (fi[11], fi[12]) and (bt[11], bt[12]) == (ft[11], ft[12])
    assert bt[14] == bi[15] and bt[15] == bi[14] and bi[14] != bi[15]     # one gradient buffer per matrix
    assert bi[16] == bt[16]
    assert bi[15] == bi[14] + NA * E * 4 and bi[16] == bi[15] + NB * E * 4          # dq | dk | scalars: one fill
    lb = rec.pointers("ce_l2norm_bwd")
    assert lb[0][0] == bi[14] and lb[1][0] == bi[15]
    assert a.grad.shape == (NA, E) and b.grad.shape == (NB, E) and ls.grad.shape == ()


def test_multipos_one_direction_with_a_query_gather(rec):
    from clip_event_amd.functional import MultiPosHeadFn
    a, b, ls, ga, gb, sel = _inputs()
    loss = MultiPosHeadFn.apply(b, a, ls, gb, ga, sel)
    assert loss.shape == ()
    loss.backward()
    fwd, bwd = _split(rec)
    assert fwd == ["ce_l2norm_fwd", "ce_l2norm_fwd", "ce_multipos_head_workspace_bytes", "ce_multipos_head_fwd"]
    assert bwd == ["ce_multipos_head_bwd", "ce_l2norm_bwd", "ce_l2norm_bwd"]
    assert rec.ints("ce_multipos_head_workspace_bytes") == [[3]]
    assert rec.ints("ce_multipos_head_fwd") == [[128, 3, 128, 5, 128]]
    assert rec.pointers("ce_multipos_head_fwd")[0][2] is not None


def test_multipos_refuses_id_vectors_of_the_wrong_length(rec):
    from clip_event_amd.functional import MultiPosHeadFn
    a, b, ls, ga, gb, _ = _inputs()
    with pytest.raises(RuntimeError, match="group ids"):
        MultiPosHeadFn.apply(a, b, ls, gb, ga, None)
    assert [n for n in rec.names() if not n.startswith("ce_l2norm")] == []


def test_sigmoid_group_form_calls(rec):
    from clip_event_amd.functional import SigmoidHeadFn
    a, b, ls, ga, gb, _ = _inputs()
    bias = torch.tensor(-10.0, requires_grad=True)
    SigmoidHeadFn.apply(a, b, ls, bias, None, None, None, None, (ga, gb)).backward()
    fwd, bwd = _split(rec)
    assert fwd == ["ce_l2norm_fwd", "ce_l2norm_fwd", "ce_sigmoid_head_workspace_bytes", "ce_sigmoid_head_group_fwd"]
    assert bwd == ["ce_sigmoid_head_group_bwd", "ce_l2norm_bwd", "ce_l2norm_bwd"]
    assert rec.ints("ce_sigmoid_head_workspace_bytes") == [[5, 7]]
    assert rec.ints("ce_sigmoid_head_group_fwd") == [[128, 5, 128, 7, 128]]
    assert rec.ints("ce_sigmoid_head_group_bwd") == [[128, 5, 128, 7, 128]]
    # ce_sigmoid_head_group_bwd(q, ldq, sel, nq, k, ldk, nk, E, scale, bias, qgroup, kgroup, grad, dq, dk, dscale, dbias, stream)
    p = rec.pointers("ce_sigmoid_head_group_bwd")[0]
    assert p[10] == ga.data_ptr() and p[11] == gb.data_ptr()
    assert p[14] == p[13] + NA * E * 4 and p[15] == p[14] + NB * E * 4 and p[16] == p[15] + 4
    assert bias.grad.shape == () and ls.grad.shape == ()


def test_sigmoid_label_form_makes_the_calls_it_made(rec):
    from clip_event_amd.functional import SigmoidHeadFn
    a, b, ls, ya, _, _ = _inputs()
    bias = torch.tensor(-10.0, requires_grad=True)
    SigmoidHeadFn.apply(a, b, ls, bias, ya, None).backward()
    assert rec.names() == ["ce_l2norm_fwd", "ce_l2norm_fwd", "ce_sigmoid_head_workspace_bytes", "ce_sigmoid_head_fwd",
                           "ce_sigmoid_head_bwd", "ce_l2norm_bwd", "ce_l2norm_bwd"]


# ---- the criteria on the host ----------------------------------------------------------------------------------------------------

def _capture_elem_loss(monkeypatch):
    from clip_event_amd import losses
    seen = []

    class Stub:
        @staticmethod
        def apply(x, y, mode):
            seen.append((x.clone(), y.clone(), mode))
            return x.sum() * 0

    monkeypatch.setattr(losses, "_ElemLossFn", Stub)
    return seen


def test_criterion_sigmoid_is_unchanged_by_default(monkeypatch):
    """``CriterionSigmoid()`` has ``multi_positive`` False and hands BCE-with-logits the one-hot target of the label column --
    labels that would be a different target read as group ids."""
    from clip_event_amd.losses import CriterionSigmoid
    seen = _capture_elem_loss(monkeypatch)
    crit = CriterionSigmoid()
    assert crit.kind == "sigmoid" and crit.multi_positive is False
    x = torch.randn(3, 6, generator=torch.Generator().manual_seed(1))
    labels, text_labels = torch.tensor([0, 2, 4]), torch.tensor([0, 0, 1, 1, 2, 2])
    out = crit(x, None, labels, text_labels, constrastive_overbatch=True, logit_bias=torch.tensor(-10.0))
    assert sorted(out) == ["loss_sig"] and len(seen) == 1
    xb, target, mode = seen[0]
    onehot = torch.zeros(3, 6)
    onehot[torch.arange(3), labels] = 1.0
    assert mode == 0 and torch.equal(target, onehot) and torch.equal(xb, x - 10.0)


def test_criterion_sigmoid_multi_positive_builds_the_multi_hot_target(monkeypatch):
    from clip_event_amd.losses import CriterionSigmoid
    seen = _capture_elem_loss(monkeypatch)
    crit = CriterionSigmoid(multi_positive=True)
    x = torch.zeros(3, 6)
    gi, gt = torch.tensor([0, -1, 2]), torch.tensor([0, 0, -1, -1, 2, 7])
    crit(x, None, gi, gt, constrastive_overbatch=True, logit_bias=torch.tensor(-10.0))
    assert seen[0][1].tolist() == [[1, 1, 0, 0, 0, 0], [0] * 6, [0, 0, 0, 0, 1, 0]]
    with pytest.raises(RuntimeError, match="negatives"):
        crit(x, None, gi, gt, constrastive_overbatch=False, logit_bias=torch.tensor(-10.0))


def test_criterion_multipositive_refusals():
    from clip_event_amd.losses import CriterionMultiPositive
    import clip_event_amd
    crit = CriterionMultiPositive()
    assert crit.kind == "multipos" and clip_event_amd.CriterionMultiPositive is CriterionMultiPositive
    x = torch.zeros(2, 4)
    with pytest.raises(RuntimeError, match="constrastive_overbatch=True"):
        crit(x, x.t(), torch.arange(2), torch.arange(4), constrastive_overbatch=False)
    with pytest.raises(RuntimeError, match="group ids"):
        crit(x, x.t())
