"""GPU: the public interface over ``ce_score_topk`` (clip_event_amd/inference.py): no [nq, nk] matrix is allocated, a bank
encoded once gives ``zero_shot``'s numbers at the best k candidates, and the retrieval metrics are those of the fp64 ranks."""
import numpy as np
import pytest
import torch

from tests import retrieval_ref as RR

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N_IMG, N_TXT, E = 24, 40, 128


def test_retrieval_metrics_never_holds_the_matrix():
    from clip_event_amd.inference import retrieval_metrics
    n, e = 8192, 128
    g = torch.Generator(device="cpu").manual_seed(3)
    img = torch.randn(n, e, generator=g).to(DEV)
    txt = (img.cpu() + 0.5 * torch.randn(n, e, generator=g)).to(DEV)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = retrieval_metrics(img, txt)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    print(f"[retrieval_metrics {n} x {n}, E = {e}] peak rise {rise / 2**20:.1f} MiB; the matrix would be {n * n * 4 / 2**20:.0f} MiB; {out}")
    assert rise < n * n * 4 // 4
    assert out["i2t_n"] == n and out["t2i_n"] == n
    assert out["i2t_R@1"] > 0.9 and out["t2i_R@1"] > 0.9          # each text is its image plus noise half its size


@pytest.fixture(scope="module")
def tiny():
    """A tiny oracle configuration with embed_dim 128: the model, 24 images, 40 candidate texts, and what ``zero_shot`` and the
    new interface return for them (computed once)."""
    from oracle import clip_oracle as O
    from clip_event_amd import synthetic as S
    from clip_event_amd.inference import encode_bank, zero_shot, zero_shot_topk
    from clip_event_amd.model import build_model
    cfg = O.ClipConfig(E, 64, 2, 128, 32, 20, 512, 128, 2, 2)
    m = build_model({k: v.clone() for k, v in O.init_params(cfg, 13).items()}).to(DEV)
    img = S.synthetic_images(N_IMG, cfg.image_resolution, seed=31).to(DEV)
    txt = S.synthetic_tokens(N_TXT, cfg.context_length, cfg.vocab_size, seed=32, min_len=2).to(DEV)
    scores, pred_idx, probs = zero_shot(m, img, txt)
    bank = encode_bank(m, text=txt)
    top_probs, top_idx = zero_shot_topk(m, img, bank, 5)
    with torch.no_grad():
        raw_i, raw_t = m.encode_image(img), m.encode_text(txt)
    torch.cuda.synchronize()
    return dict(m=m, img=img, txt=txt, scores=scores, pred_idx=pred_idx, probs=probs, bank=bank, top_probs=top_probs,
                top_idx=top_idx, raw_i=raw_i, raw_t=raw_t)


def test_zero_shot_topk_agrees_with_zero_shot(tiny):
    probs, top_probs, top_idx = tiny["probs"].cpu(), tiny["top_probs"].cpu(), tiny["top_idx"].cpu()
    assert tuple(top_probs.shape) == (N_IMG, 5) and tuple(top_idx.shape) == (N_IMG, 5) and top_idx.dtype == torch.int64
    assert tuple(tiny["bank"].shape) == (N_TXT, E) and tiny["bank"].dtype == torch.float32
    assert torch.allclose(tiny["bank"].norm(dim=1).cpu(), torch.ones(N_TXT), atol=1e-5)
    at = probs.gather(1, top_idx)
    print(f"[zero_shot_topk] max |probs - zero_shot probs at idx| {float((top_probs - at).abs().max()):.3e}")
    assert float((top_probs - at).abs().max()) < 1e-5
    best2 = probs.topk(2, dim=1).values
    clear = (best2[:, 0] - best2[:, 1]) > 1e-5
    print(f"[zero_shot_topk] images whose two best probabilities differ by more than 1e-5: {int(clear.sum())} of {N_IMG}")
    assert torch.equal(top_idx[clear, 0], tiny["pred_idx"].cpu()[clear])
    assert bool((top_probs[:, 1:] <= top_probs[:, :-1]).all())


def test_encode_bank_in_chunks_equals_one_chunk(tiny):
    from clip_event_amd.inference import encode_bank
    m = tiny["m"]
    for kw, whole in ((dict(text=tiny["txt"]), tiny["bank"]), (dict(image=tiny["img"]), encode_bank(m, image=tiny["img"]))):
        parts = encode_bank(m, chunk=7, **kw)
        torch.cuda.synchronize()
        print(f"[encode_bank {list(kw)[0]}] chunk 7 against one chunk: max |d| {float((parts - whole).abs().max()):.3e}")
        assert torch.equal(parts, whole)
    with pytest.raises(ValueError):
        encode_bank(m)


def test_score_topk_refuses_what_the_kernel_does_not_take():
    from clip_event_amd.inference import score_topk
    with pytest.raises(ValueError):
        score_topk(torch.zeros(4, 64, device=DEV), torch.zeros(9, 64, device=DEV))
    with pytest.raises(ValueError):
        score_topk(torch.zeros(4, 128, device=DEV), torch.zeros(9, 128, device=DEV), k=17)


def test_retrieval_metrics_equal_the_fp64_ranks(tiny):
    """Both directions over 24 images and 40 texts (image i belongs to text i; texts 24..39 have no image).  A query whose
    fp64 rank could change under a score error of tol = (E + 2) 2^-24 (the band of tests/test_retrieval_ops.py) is given the
    target -1 on both sides, so it is left out of both; at least 20 of the 24 must remain in each direction."""
    from clip_event_amd.inference import metrics_from_ranks, retrieval_metrics
    I = tiny["raw_i"].double().cpu().numpy()
    T = tiny["raw_t"].double().cpu().numpy()
    I /= np.linalg.norm(I, axis=1, keepdims=True)
    T /= np.linalg.norm(T, axis=1, keepdims=True)
    tol = (E + 2) * 2.0 ** -24
    targets, refs = {}, {}
    for name, q, b in (("i2t", I, T), ("t2i", T, I)):
        target = np.arange(q.shape[0])
        target[target >= min(N_IMG, b.shape[0])] = -1
        S = RR.scores64(q, b)
        lo, hi = RR.rank_bounds(S, target, 2 * tol)
        ambiguous = (lo != hi)
        print(f"[{name}] ambiguous queries: {int(ambiguous.sum())} of {int((target >= 0).sum())} with a target")
        target[ambiguous] = -1
        assert int((target >= 0).sum()) >= 20
        targets[name] = target
        refs[name] = RR.reference(q, b, 1, target=target).rank
    got = retrieval_metrics(tiny["raw_i"], tiny["raw_t"], text_of_image=torch.from_numpy(targets["i2t"]).to(DEV),
                            image_of_text=torch.from_numpy(targets["t2i"]).to(DEV))
    for name in ("i2t", "t2i"):
        want = metrics_from_ranks(torch.from_numpy(refs[name]))
        print(f"[{name}] {want}")
        for key, v in want.items():
            assert got[f"{name}_{key}"] == v, (name, key, got[f"{name}_{key}"], v)
