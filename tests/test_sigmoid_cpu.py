"""CPU (no GPU): the sigmoid pairwise loss's reference against BCE-with-logits, and the opt-in ``logit_bias`` parameter through
the model's host-side surfaces -- state dict, parameter groups, the trainable tables, ``build_model``."""
import pytest
import torch
import torch.nn.functional as F

from oracle import clip_oracle as O
from tests.sigmoid_ref import sigmoid_loss_from_logits

CFG = O.ClipConfig(64, 64, 2, 128, 32, 20, 512, 128, 2, 3)


def _sd():
    return {k: v.clone() for k, v in O.init_params(CFG, 3).items()}


def _clip():
    from clip_event_amd.model import build_model
    return build_model(_sd())


@pytest.mark.parametrize("nq,nk", [(5, 7), (16, 48)])
def test_reference_is_bce_with_logits_times_nk(nq, nk):
    """-(1/nq) sum log sigma(z x) is BCE-with-logits (mean over nq * nk elements) against the one-hot target, times nk -- the
    identity ``losses.CriterionSigmoid`` is built on -- in fp64 to 1e-12, with saturated entries of both signs."""
    g = torch.Generator().manual_seed(nq * 100 + nk)
    x = torch.randn(nq, nk, generator=g, dtype=torch.float64) * 8 - 5
    labels = torch.randint(0, nk, (nq,), generator=g)
    onehot = torch.zeros(nq, nk, dtype=torch.float64)
    onehot[torch.arange(nq), labels] = 1.0
    ref = sigmoid_loss_from_logits(x, labels)
    bce = F.binary_cross_entropy_with_logits(x, onehot) * nk
    assert abs(float(ref - bce)) <= 1e-12 * abs(float(bce))
    # and term by term: a positive pays softplus(-x), a negative softplus(x)
    by_hand = (F.softplus(-x) * onehot + F.softplus(x) * (1 - onehot)).sum() / nq
    assert abs(float(ref - by_hand)) <= 1e-12 * abs(float(by_hand))


def test_logit_bias_is_opt_in():
    """Without ``enable_logit_bias`` the model has the reference's keys and parameters; with it exactly one more key, a scalar
    fp32 parameter at the given value; a second call sets the value and adds nothing."""
    ref_keys = sorted(_sd())
    m = _clip()
    assert sorted(m.state_dict()) == ref_keys and "logit_bias" not in ref_keys
    n_params, n_elems = len(list(m.parameters())), sum(p.numel() for p in m.parameters())
    assert getattr(m, "logit_bias", None) is None
    m.enable_logit_bias()
    assert sorted(m.state_dict()) == sorted(ref_keys + ["logit_bias"])
    assert len(list(m.parameters())) == n_params + 1 and sum(p.numel() for p in m.parameters()) == n_elems + 1
    assert m.logit_bias.shape == () and m.logit_bias.dtype == torch.float32 and m.logit_bias.requires_grad
    assert float(m.logit_bias.detach()) == -10.0
    m.enable_logit_bias(init=-3.5)
    assert float(m.logit_bias.detach()) == -3.5 and len(list(m.parameters())) == n_params + 1


def test_no_decay_groups_put_the_bias_with_the_scale():
    from clip_event_amd.optim import no_decay_groups
    m = _clip()
    m.enable_logit_bias()
    decay, no_decay = no_decay_groups(m, 0.2)
    assert no_decay["weight_decay"] == 0.0 and decay["weight_decay"] == 0.2
    assert "logit_bias" in no_decay["params"] and "logit_scale" in no_decay["params"] and "logit_bias" not in decay["params"]


def test_trainable_tables_give_the_bias_a_head_segment_and_no_tile():
    """``tower_of`` answers 'head'; in the tables of a flat layout in miniature the bias has one segment of four elements (the
    16-byte round-up of one element) and one chunk, is in no tile, follows its group, and leaves the tables when frozen.  The
    model's own plan (host form) does not count it towards a tower: both towers frozen and the bias trainable is 'locked'."""
    from clip_event_amd.model import tower_of, trainable_tables
    assert tower_of("logit_bias") == "head" and tower_of("logit_scale") == "head"
    shapes = {"logit_scale": (), "logit_bias": (), "visual.proj": (8, 4),
              "visual.transformer.resblocks.0.attn.in_proj_weight": (24, 8), "text_projection": (8, 4)}
    offsets = {n: 64 * i for i, n in enumerate(shapes)}
    tiles = ["visual.transformer.resblocks.0.attn.in_proj_weight"]
    t = trainable_tables(offsets, shapes, {n: True for n in shapes}, {"logit_bias": 1, "logit_scale": 1}, tiles)
    lo = offsets["logit_bias"]
    assert (lo, lo + 4) in t["segments"] and (lo, lo + 4) in t["chunks"]
    assert t["segment_group"][t["segments"].index((lo, lo + 4))] == 1
    assert [n for n, _ in t["tiles"]] == tiles
    frozen = trainable_tables(offsets, shapes, {n: n != "logit_bias" for n in shapes}, None, tiles)
    assert (lo, lo + 4) not in frozen["segments"] and (lo, lo + 4) not in frozen["chunks"]
    m = _clip()
    m.enable_logit_bias()
    for n, p in m.named_parameters():
        p.requires_grad_(n == "logit_bias")
    plan = m.trainable_plan()
    assert plan.locked == {"visual": True, "text": True} and not plan.plain


def test_build_model_round_trips_the_bias_and_a_dict_without_it_keeps_it():
    from clip_event_amd.model import build_model
    m = _clip()
    m.enable_logit_bias(init=-7.25)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    m2 = build_model(dict(sd))
    assert float(m2.logit_bias) == -7.25 and sorted(m2.state_dict()) == sorted(sd)
    for k in sd:
        assert torch.equal(m2.state_dict()[k], sd[k]), k
    # a reference state dict (no key) into a model that has the bias: loads, the bias keeps its value
    plain = _sd()
    plain["logit_scale"] = torch.tensor(1.5)
    m2.load_state_dict(plain)
    assert float(m2.logit_bias) == -7.25 and float(m2.logit_scale) == 1.5
    assert "logit_bias" not in plain                      # the caller's dict is left alone
    # and a model without the bias still refuses a key it does not have (strict load, as before)
    with pytest.raises(RuntimeError, match="logit_bias"):
        _clip().load_state_dict(sd)


def test_criterion_sigmoid_refuses_the_per_instance_layout():
    from clip_event_amd.losses import CriterionSigmoid
    crit = CriterionSigmoid()
    assert crit.kind == "sigmoid"
    x = torch.zeros(2, 3)
    with pytest.raises(RuntimeError, match="negatives"):
        crit(x, None, constrastive_overbatch=False, logit_bias=torch.tensor(-10.0))
