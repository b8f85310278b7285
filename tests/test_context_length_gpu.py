"""GPU: the text tower at another context length through the model (``CLIP.set_context_length``) -- a checkpoint
that is native at 248 tokens with packing on, packed against dense above 128 tokens, a twin model that is native at the run
length, the oracle on the resized state dict, the routing by the batch's longest caption, train steps, the native length, the
micro-batched step.

Tiny geometry: text width 128, 2 heads, 3 blocks, native context 77; run lengths 160 and 248 (packed long attention: captions
beyond 128 tokens), 32 (truncation).  Bounds are those the same quantities have elsewhere in the suite, named at each use."""
import contextlib

import numpy as np
import pytest
import torch

from tests.test_image_size_gpu import _atomic_slices, _bits_equal, _twin_rule
from tests.test_micro_batch_gpu import _compare_to_unchunked
from tests.test_micro_batch_gpu import _step_gradients as _mb_step_gradients
from tests.test_model_gpu import _cos, _grad_report, _mk, _rel

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TINY = (64, 64, 2, 128, 32, 77, 512, 128, 2, 3)
T0, D, VOCAB, RES = 77, 128, 512, 64
SEED = 5
U = 2.0 ** -24


@pytest.fixture(params=[False, True], ids=["stream32", "stream16"])
def stream16(request, monkeypatch):
    """Both residual-stream formats (fixture of tests/test_model_gpu.py)."""
    monkeypatch.setenv("CE_STREAM16", "1" if request.param else "0")
    return request.param


def _cfg(T=T0):
    from oracle import clip_oracle as O
    return O.ClipConfig(*(TINY[:5] + (T,) + TINY[6:]))


def _crit():
    from clip_event_amd.losses import CriterionContrastive
    return CriterionContrastive("ce")


def _captions(lens, T, seed):
    """[len(lens), T] token rows whose lengths (tokens up to and including the EOT) are ``lens``: SOT, ids, EOT, zero padding; a
    length of 1 is the EOT alone."""
    rng = np.random.default_rng(seed)
    out = np.zeros((len(lens), T), dtype=np.int64)
    for i, n in enumerate(lens):
        assert 1 <= n <= T
        if n > 1:
            out[i, 0] = VOCAB - 2
            out[i, 1:n - 1] = rng.integers(1, VOCAB - 2, size=n - 2)
        out[i, n - 1] = VOCAB - 1
    return torch.from_numpy(out)


def _data(T, B=4, K=3):
    from oracle import clip_oracle as O
    from clip_event_amd import synthetic as S
    img = S.synthetic_images(B, RES, seed=21)
    txt = S.synthetic_tokens(B * K, T, VOCAB, seed=22, min_len=1)
    return img, txt, O.build_labels(B, 1, K - 1, True)


def _run(m, img, txt, labels):
    """Text features, loss and the gradient slices by name of one forward + backward."""
    yi, yt, ip = labels
    img, txt = img.to(DEV), txt.to(DEV)
    with torch.no_grad():
        feat = m.encode_text(txt).clone()
    m.zero_grad()
    li, lt = m(img, txt)
    ld = _crit()(li, lt, yi.to(DEV), yt.to(DEV), index_pos=ip.to(DEV), constrastive_overbatch=True)
    loss = ld["loss_i"] + ld["loss_t"]
    loss.backward()
    torch.cuda.synchronize()
    return dict(feat=feat, li=li.detach().cpu(), lt=lt.detach().cpu(), loss=float(loss.detach()),
                ld={k: float(v.detach()) for k, v in ld.items()},
                grads={n: m._gview(n).detach().clone() for n, _ in m.named_parameters()})


def _twin(sd, T, keep=20):
    """A model that is native at ``T``: the same weights, the positional table ``stretch_host`` rounded to fp32."""
    from clip_event_amd.model import build_model
    from clip_event_amd.posembed import resize_text_state_dict
    return build_model(resize_text_state_dict({k: v.clone() for k, v in sd.items()}, T, keep)).to(DEV)


# ---- 1. a checkpoint that is native at a long context -------------------------------------------------------------------------

def test_native_long_checkpoint_runs_packed(stream16):
    """Native at 248 tokens, packing on, lengths on both sides of the 128-token limit of the short kernels.  Features against
    the fp32 oracle at the cosine tests/test_model_gpu.py::test_tiny_features_bf16_oracle asks (its rel-L2 bound against the
    bf16 oracle is a figure measured at 77 tokens and is printed here, not asserted)."""
    from oracle import clip_oracle as O
    sd = O.init_params(_cfg(), SEED)
    m = _twin(sd, 248)
    assert m.pack_text and m.context_length == m.native_context_length == 248
    txt = _captions([1, 128, 129, 248, 2, 64, 65, 127, 200, 33, 192, 193], 248, seed=3)
    w = torch.from_numpy(np.random.default_rng(3).standard_normal((12, TINY[0])).astype(np.float32)).to(DEV)
    f = m.encode_text(txt.to(DEV))
    (f * w).sum().backward()
    torch.cuda.synchronize()
    rsd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    with (O.stream_f16() if stream16 else contextlib.nullcontext()), torch.no_grad():
        f16 = O.encode_text(rsd, _cfg(248), txt, bf16=True)
    f32 = O.encode_text(rsd, _cfg(248), txt)
    print(f"[native 248] rel-l2 vs bf16-oracle {_rel(f.detach(), f16):.2e}, cos vs fp32 {_cos(f.detach(), f32):.6f}")
    assert _cos(f.detach(), f32) > 0.9995
    for n, p in m.named_parameters():
        if not n.startswith("visual.") and n != "logit_scale":
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0.0, n
    assert tuple(m.positional_embedding.grad.shape) == (248, D)


# ---- 2. packed against dense --------------------------------------------------------------------------------------------------

def test_packed_equals_dense_at_run_length_160(stream16):
    """tests/test_model_gpu.py::test_text_packing_matches_dense_layout at run length 160 on the 77-native model."""
    from clip_event_amd import synthetic as S
    m, _ = _mk(_cfg(), SEED)
    m.set_context_length(160)
    txt = S.synthetic_tokens(24, 160, VOCAB, seed=11, min_len=1).to(DEV)
    txt[3, :] = 0
    txt[3, 0], txt[3, 1] = VOCAB - 2, VOCAB - 1                               # empty caption: SOT EOT
    lens = (txt.argmax(dim=-1) + 1).cpu()
    assert int((lens > 128).sum()) >= 2 and int(lens.min()) == 2
    w = torch.from_numpy(np.random.default_rng(3).standard_normal((24, TINY[0])).astype(np.float32)).to(DEV)
    res = {}
    for packed in (True, False):
        m.pack_text = packed
        m.zero_grad(set_to_none=True)
        f = m.encode_text(txt)
        (f * w).sum().backward()
        torch.cuda.synchronize()
        res[packed] = (f.detach().cpu(), {n: p.grad.detach().cpu().clone() for n, p in m.named_parameters()
                                          if p.grad is not None})
    m.pack_text = True
    assert tuple(res[True][1]["positional_embedding"].shape) == (T0, D)
    assert _rel(res[True][0], res[False][0]) < 1e-5
    worst = 0.0
    for n, g in res[False][1].items():
        if float(g.norm()) == 0.0:
            assert float(res[True][1][n].norm()) == 0.0, n
            continue
        worst = max(worst, _rel(res[True][1][n], g))
        assert _rel(res[True][1][n], g) < 2e-3, (n, _rel(res[True][1][n], g))
    print(f"[packing at 160] features rel {_rel(res[True][0], res[False][0]):.2e}, worst grad rel {worst:.2e}")


# ---- 3. twin model ------------------------------------------------------------------------------------------------------------

def _pos_grad_follows_the_twin(tag, got, ta, tb, T, keep=20):
    """The rule of tests/test_image_size_gpu.py::_pos_grad_follows_the_twin for the stretch: ``m``'s positional gradient against
    W^T applied in fp64 to the twin's [T, d] gradient, element by element, within the op-level bound of
    tests/test_context_length_ops.py ((n_c + 2) u |W|^T |dT|) plus 4 x the transpose of the two twin runs' difference."""
    from clip_event_amd.posembed import text_weights
    W = text_weights(T0, T, keep)
    a, b = ta.cpu().numpy().astype(np.float64), tb.cpu().numpy().astype(np.float64)
    ref = W.T @ a
    n_c = (W != 0).sum(axis=0)[:, None]
    bound = (n_c + 2) * U * (np.abs(W).T @ np.abs(a)) + 4 * (np.abs(W).T @ np.abs(a - b))
    err = np.abs(got.cpu().numpy().astype(np.float64) - ref)
    nz = bound > 0
    print(f"[{tag}] positional gradient: worst |err| / bound {float((err[nz] / bound[nz]).max()):.3f}; twin runs "
          f"{'agree' if np.array_equal(a, b) else 'differ'}")
    assert bool((err <= bound).all())
    assert float(np.abs(ref).max()) > 0.0


@pytest.mark.parametrize("T", [160, 248, 32])
def test_equals_a_twin_that_is_native_at_the_run_length(T, stream16):
    from clip_event_amd import posembed
    m, sd = _mk(_cfg(), SEED)
    assert m.set_context_length(T) == T
    m._ready()
    table = m._text_pos_run().clone()
    host = torch.from_numpy(posembed.stretch_host(sd["positional_embedding"], T).astype(np.float32))
    assert tuple(table.shape) == (T, D) and _bits_equal(table, host)
    img, txt, labels = _data(T)
    got = _run(m, img, txt, labels)
    a, b = (_run(_twin(sd, T), img, txt, labels) for _ in range(2))
    exact = sum(_twin_rule(k, got[k], a[k], b[k]) for k in ("feat", "li", "lt"))
    # The losses are NOT under the bit rule: ce_xent_fwd adds its rows' terms into the mean with float atomics, so the same
    # logits (bit-equal above) give loss_i / loss_t that differ in the last place from run to run -- two twin runs that happen
    # to agree say nothing about a third.  16 = 4 + 12 rows, each add rounding at most the running sum: 16 u |loss|.
    assert abs(got["loss"] - a["loss"]) <= 4 * abs(a["loss"] - b["loss"]) + 16 * U * abs(a["loss"])
    atomic = _atomic_slices(m, 4, 5, txt)
    loose = 0
    for n in a["grads"]:
        if n == "positional_embedding":
            continue
        if _twin_rule(n, got["grads"][n], a["grads"][n], b["grads"][n], atomics=n in atomic):
            exact += 1
        else:
            loose += 1
    print(f"[twin {T} tokens] {exact} tensors bit-equal, {loose} within 4 x spread")
    assert tuple(got["grads"]["positional_embedding"].shape) == (T0, D)
    assert m.positional_embedding.grad.data_ptr() == m._gview("positional_embedding").data_ptr()
    # The positional gradient.  Packed, its reduction over the captions (ce_pos_embed_bwd_packed, in the twin and in the scratch
    # the transpose reads) adds up to 8 partial sums per element with float atomics -- the slice is one of _atomic_slices, which
    # takes the spread rule whatever two runs say: W^T applied to the twin's gradient, rel-L2 within 4 x the twin runs' spread.
    Wt = torch.from_numpy(posembed.text_weights(T0, T, 20).T.copy())
    ra, rb = (Wt @ r["grads"]["positional_embedding"].cpu().double() for r in (a, b))
    assert not _twin_rule("positional_embedding (packed)", got["grads"]["positional_embedding"], ra, rb, atomics=True)
    assert float(ra.abs().max()) > 0.0
    # Dense, the reduction is ce_batch_reduce -- one writer per element, the same order in both models -- and the element-wise rule
    # of tests/test_image_size_gpu.py holds: the op-level bound plus 4 x the transpose of the twin runs' difference.
    dense = []
    for model in (m, _twin(sd, T), _twin(sd, T)):
        model.pack_text = False
        dense.append(_run(model, img, txt, labels)["grads"]["positional_embedding"])
    m.pack_text = True
    _pos_grad_follows_the_twin(f"twin {T} tokens, dense layout", *dense, T)


# ---- 4. the oracle, and the routing by the longest caption --------------------------------------------------------------------

def _against_the_oracle(tag, T, img, txt, labels, stream16, want_tokens=None):
    """Bounds of tests/test_model_gpu.py::test_tiny_against_oracle (logits, losses, gradients) and the cosine of
    ::test_tiny_features_bf16_oracle (text features; its rel-L2 figure, measured at 77 tokens, is printed only); the oracle stretches the table inside the graph, so
    ``positional_embedding`` receives autograd's gradient at its native shape."""
    from oracle import clip_oracle as O
    from clip_event_amd.functional import _text_desc, text_packing
    from clip_event_amd.posembed import resize_text_state_dict, text_weights
    cfg = _cfg(T)
    yi, yt, ip = labels
    sd = O.init_params(_cfg(), SEED)
    q = {k: v.detach().clone().requires_grad_(True) for k, v in sd.items()}
    p = dict(q)
    p["positional_embedding"] = (torch.from_numpy(text_weights(T0, T, 20)) @ q["positional_embedding"].double()).float()
    li32, lt32 = O.clip_forward(p, cfg, img, txt, True)
    ld32 = O.criterion_contrastive(li32, lt32, yi, yt, ip)
    sum(ld32.values()).backward()
    g32 = {k: v.grad for k, v in q.items()}
    rsd = resize_text_state_dict(sd, T)
    with (O.stream_f16() if stream16 else contextlib.nullcontext()), torch.no_grad():
        li16, lt16 = O.clip_forward(rsd, cfg, img, txt, True, bf16=True)
        f16 = O.encode_text(rsd, cfg, txt, bf16=True)
    with torch.no_grad():
        f32 = O.encode_text(rsd, cfg, txt)
    m, _ = _mk(_cfg(), SEED)
    m.set_context_length(T)
    got = _run(m, img, txt, labels)
    if want_tokens is not None:
        assert _text_desc(m, text_packing(m, txt.to(DEV))).tokens == want_tokens
    print(f"[{tag}] text features rel-l2 vs bf16-oracle {_rel(got['feat'], f16):.2e}, cos vs fp32 {_cos(got['feat'], f32):.6f}; "
          f"logits vs bf16-oracle max|d| {float((got['li'] - li16).abs().max()):.4f}, vs fp32 {float((got['li'] - li32.detach()).abs().max()):.4f}")
    assert _cos(got["feat"], f32) > 0.9995
    assert (got["li"] - li16).abs().max() < 0.05 and (got["lt"] - lt16).abs().max() < 0.05
    assert (got["li"] - li32.detach()).abs().max() < 0.15 and (got["lt"] - lt32.detach()).abs().max() < 0.15
    for k in ("loss_i", "loss_t"):
        print(f"[{tag}] {k} {got['ld'][k]:.5f} (oracle {float(ld32[k]):.5f})")
        assert abs(got["ld"][k] - float(ld32[k])) < 2e-2
    worst, rels = _grad_report(m, g32, tag)
    assert worst[0] > 0.98 and np.median(rels) < 0.03
    pg, rg = m.positional_embedding.grad, g32["positional_embedding"]
    print(f"[{tag}] positional gradient against autograd through the stretch: cos {_cos(pg, rg):.5f}, rel-l2 {_rel(pg, rg):.4f}")
    assert tuple(pg.shape) == tuple(rg.shape) == (T0, D) and _cos(pg, rg) > 0.98


def test_against_the_oracle_at_160_tokens(stream16):
    img, txt, labels = _data(160)
    _against_the_oracle("oracle at 160 tokens", 160, img, txt, labels, stream16, want_tokens=160)


@pytest.mark.parametrize("longest,tokens", [(128, 128), (200, 248)], ids=["short-kernels", "packed-long-kernels"])
def test_routing_by_the_longest_caption(longest, tokens, stream16):
    """Run length 248: a batch whose captions all fit 128 tokens is sized for 128 (the short kernels), one 200-token caption
    sends the pass to the packed long kernels; both against the oracle."""
    img, _, labels = _data(248)
    lens = [longest, 2, 77, 33, 64, 65, 100, 17, 128, 5, 96, 50]
    txt = _captions(lens, 248, seed=9)
    _against_the_oracle(f"routing, longest {longest}", 248, img, txt, labels, stream16, want_tokens=tokens)


# ---- 5. train steps, the native length ----------------------------------------------------------------------------------------

def test_train_steps_at_run_length_160(stream16):
    from clip_event_amd import posembed
    from clip_event_amd.engine import train_step
    from clip_event_amd.optim import FusedAdam
    m, sd = _mk(_cfg(), SEED)
    native, _ = _mk(_cfg(), SEED)
    native._ready()
    m.set_context_length(160)
    img, txt, (yi, yt, ip) = _data(160)
    args = (img.to(DEV), txt.to(DEV), yi.to(DEV), yt.to(DEV), ip.to(DEV))
    with torch.no_grad():
        f0 = m.encode_text(args[1]).clone()
    before = m._text_pos_run().clone()
    opt = FusedAdam(m, lr=1e-3, max_norm=1.0)
    for _ in range(2):
        ld = train_step(m, _crit(), opt, *args)
        assert all(np.isfinite(float(v)) for v in ld.values())
    assert m.context_length == 160
    # optimiser state and checkpoint have the native shapes
    assert opt.m.shape == opt.v.shape == native._flat.shape == m._flat.shape
    ck = m.state_dict()
    assert {k: tuple(v.shape) for k, v in ck.items()} == {k: tuple(v.shape) for k, v in native.state_dict().items()}
    assert tuple(ck["positional_embedding"].shape) == (T0, D)
    assert not torch.equal(ck["positional_embedding"].cpu(), sd["positional_embedding"])
    # the table follows the parameter: a forward after the steps adds the stretch of the parameter as it is now
    with torch.no_grad():
        f1 = m.encode_text(args[1]).clone()
    used = m._text_pos_run()
    fresh = posembed.stretch(m.positional_embedding.detach().clone(), 160)
    assert _bits_equal(used, fresh) and not torch.equal(used, before) and not torch.equal(f1, f0)
    twin = _twin({k: v.detach().cpu() for k, v in ck.items()}, 160)
    diff = (twin.positional_embedding.detach() != fresh)
    print(f"[train steps] twin table against the device stretch: {int(diff.sum())} elements differ, rows "
          f"{sorted(set(diff.nonzero()[:, 0].tolist()))[:12]}, max |d| {float((twin.positional_embedding.detach() - fresh).abs().max()):.3e}")
    assert _bits_equal(twin.positional_embedding.detach(), fresh)
    with torch.no_grad():
        assert _bits_equal(twin.encode_text(args[1]), f1)


class _Counting:
    """Stands in front of the loaded library: counts the calls of the two stretch entry points."""

    def __init__(self, real):
        self.real, self.fwd, self.bwd = real, 0, 0

    def __getattr__(self, name):
        if name == "ce_pos_stretch_fwd":
            self.fwd += 1
        elif name == "ce_pos_stretch_bwd":
            self.bwd += 1
        return getattr(self.real, name)


@pytest.fixture
def counted(monkeypatch):
    from clip_event_amd import posembed
    c = _Counting(posembed.lib())
    monkeypatch.setattr(posembed, "lib", lambda: c)
    return c


def test_native_length_is_the_parent_behaviour(stream16, counted):
    """tests/test_image_size_gpu.py::test_native_size_is_the_parent_behaviour for the text side."""
    img, txt, labels = _data(T0)
    never, _ = _mk(_cfg(), SEED)
    ref = _run(never, img, txt, labels)
    assert counted.fwd == 0 and counted.bwd == 0
    assert never._text_pos_run() is None and never._tpos_cache == {}
    m, _ = _mk(_cfg(), SEED)
    m.set_context_length(160)
    with torch.no_grad():
        m.encode_text(_data(160)[1].to(DEV))
    assert counted.fwd == 1
    with pytest.raises(RuntimeError, match="expected 160 tokens"):
        m.encode_text(txt.to(DEV))
    m.set_context_length(None)
    got = _run(m, img, txt, labels)
    assert counted.fwd == 1 and counted.bwd == 0
    assert torch.equal(got["feat"], ref["feat"])
    again = _run(never, img, txt, labels)
    atomic = _atomic_slices(m, 4, 5, txt)
    for n in ref["grads"]:
        _twin_rule(n, got["grads"][n], ref["grads"][n], again["grads"][n], atomics=n in atomic)
    with pytest.raises(RuntimeError, match="expected 77 tokens"):
        m.encode_text(_data(160)[1].to(DEV))


# ---- 6. the micro-batched step ------------------------------------------------------------------------------------------------

def test_micro_batched_step_at_run_length_160(stream16):
    """B = 3 images of 2 captions in chunks of 2 (a ragged last chunk) against the unchunked step
    (tests/test_micro_batch_gpu.py::_compare_to_unchunked: losses within 3e-3, every parameter's gradient within 2e-3 rel-L2).

    The shape is the smallest that has a caption beyond 128 tokens in one chunk (152) and none in the other (longest 124), so
    the chunks would split between the short and the tiled attention kernels if each were routed by its own longest caption:
    the step routes them all by the step's longest (``model._route_longest``).  It also keeps the unchunked pass (493 text
    rows) and the chunks (325, 168) inside one kernel class of the NT GEMM planner, which changes kernels at 513 and at 1024
    rows for this tower's four GEMM shapes -- the premise of the 2e-3 bound, which is what "a different tile choice at a smaller
    M" costs, and which the suite's own micro-batch tests meet the same way.  Across a class boundary the bound is not
    reachable at this geometry with or without the feature: B = 5, K = 3 (1152 rows against 493 / 415 / 244) measured 1.35e-2 /
    1.64e-2 (fp32 / fp16 stream) at run length 160 and 1.70e-2 on the same model at its native 77 tokens, where the text
    features of the first 12 captions (446 rows) already differ by 2e-3 - 3e-3 from the same captions in the 15-caption pass
    (565 rows) while every caption under 30 tokens is bit-equal: fp32-level differences between two GEMM kernels, carried to
    the bf16 level by the roundings behind them."""
    from clip_event_amd.functional import host_lengths
    img, txt, (yi, yt, ip) = _data(160, 3, 2)
    lens = host_lengths(txt).reshape(3, 2)
    assert int(lens.max()) > 128 and int(lens[:2].max()) <= 128 and int(lens.sum()) <= 512
    args = (img.to(DEV), txt.to(DEV), yi.to(DEV), yt.to(DEV), ip.to(DEV))
    out = []
    for mb in (2, None):
        m, _ = _mk(_cfg(), SEED)
        m.set_context_length(160)
        out.append((m,) + _mb_step_gradients(m, _crit(), *args, mb))
        assert getattr(m, "_route_longest", None) is None            # the step's hint does not outlive the step
    (m, ld, g), (_, ld_ref, g_ref) = out
    o = m._offsets["positional_embedding"]
    assert float(g_ref[o:o + T0 * D].abs().max()) > 0.0
    _compare_to_unchunked("160 tokens, micro_batch=2", m, g, g_ref, ld, ld_ref)
