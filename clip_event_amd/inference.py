"""Zero-shot scoring on the HIP forward path: what the reference's salient-event selection does
with the model (src/preprocess/preprocess_description_contrastive.py:127-132): ``model(image, text)`` under
``no_grad``, softmax of ``logits_per_image`` over the candidate texts, best candidate and its probability.

Beyond that one call: a bank of candidates encoded once (``encode_bank``), the best k candidates with their
probabilities (``zero_shot_topk``) and image<->text retrieval numbers (``retrieval_metrics``), all on ``ce_score_topk``,
which sweeps the similarity tiles and never writes the [B, N] matrix."""
from __future__ import annotations

from typing import Dict, NamedTuple, Optional, Sequence, Tuple

import torch


def _dense(model):
    """Context in which the image tower sees every patch: inference never applies patch dropout, even on a model that was
    left in training mode (``CLIP.no_patch_dropout``)."""
    return getattr(model, "module", model).no_patch_dropout()


@torch.no_grad()
def zero_shot(model, image: torch.Tensor, text: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``image`` [B,3,R,R], ``text`` [N,77] candidate descriptions shared by all images ->
    ``(scores [B], pred_idx [B], probs [B,N])``.  Uses the over-batch logits whatever the training setting."""
    saved = model.constrastive_overbatch
    model.constrastive_overbatch = True
    try:
        with _dense(model):
            logits_per_image, _ = model(image, text)
    finally:
        model.constrastive_overbatch = saved
    probs = logits_per_image.softmax(dim=-1)
    scores, pred_idx = torch.max(probs, dim=-1)
    return scores, pred_idx, probs


class TopK(NamedTuple):
    values: torch.Tensor              # [nq, k] scores, best first
    indices: torch.Tensor             # [nq, k] int64 bank rows (-1 past the end of a bank smaller than k)
    lse: torch.Tensor                 # [nq] log-sum-exp of the scores of the whole bank
    rank: Optional[torch.Tensor]      # [nq] int64 0-based rank of ``target`` (-1: no valid target), None without targets


def _l2norm(x: torch.Tensor) -> torch.Tensor:
    from . import functional as F
    return F._l2norm(x.detach().float().contiguous())[0]


@torch.no_grad()
def score_topk(queries: torch.Tensor, bank: torch.Tensor, k: int = 1, logit_scale=None, target=None,
               normalized: bool = False) -> TopK:
    """The best ``k`` rows of ``bank`` [N,E] for every row of ``queries`` [B,E]: score = exp(logit_scale) * cosine
    (``logit_scale`` a tensor, a float or None for plain cosines), ties broken by the lower bank row.  ``target`` [B]
    (optional) asks for the rank of that bank row among all N.  ``normalized``: both inputs are unit rows already."""
    from . import ops
    if queries.dim() != 2 or bank.dim() != 2 or queries.shape[1] != bank.shape[1]:
        raise ValueError(f"queries {tuple(queries.shape)} and bank {tuple(bank.shape)} must be [B,E] and [N,E]")
    E = queries.shape[1]
    if E % 128 != 0 or not 128 <= E <= 1024:
        raise ValueError(f"embedding width {E}: the scoring kernel takes multiples of 128 in 128..1024 (there is no fallback)")
    if not 1 <= k <= 16:
        raise ValueError(f"k = {k}: the scoring kernel keeps 1..16 candidates per query")
    if queries.shape[0] < 1 or bank.shape[0] < 1:
        raise ValueError("empty queries or bank")
    dev = queries.device
    if normalized:
        q, b = queries.detach().float().contiguous(), bank.detach().float().contiguous()
    else:
        q, b = _l2norm(queries), _l2norm(bank)
    if logit_scale is not None:
        logit_scale = torch.as_tensor(logit_scale).detach().to(device=dev, dtype=torch.float32).reshape(1)
    if target is not None:
        target = torch.as_tensor(target).to(device=dev, dtype=torch.int64).contiguous()
    return TopK(*ops.score_topk(q, b, k, logit_scale=logit_scale, target=target))


@torch.no_grad()
def encode_bank(model, image: Optional[torch.Tensor] = None, text: Optional[torch.Tensor] = None, chunk: int = 256) -> torch.Tensor:
    """Unit-norm fp32 features [N,E] of ``image`` [N,3,R,R] or ``text`` [N,77], encoded ``chunk`` rows at a time through
    the tower that keeps no stash (no gradient will follow): a bank for ``zero_shot_topk`` / ``retrieval_metrics``."""
    if (image is None) == (text is None):
        raise ValueError("encode_bank takes exactly one of image= and text=")
    x = image if text is None else text
    dev = model.logit_scale.device
    out = []
    for i in range(0, x.shape[0], chunk):
        part = x[i:i + chunk].to(dev)
        with _dense(model):
            f = model.encode_image(part) if text is None else model.encode_text(part)
        out.append(_l2norm(f))
    return out[0] if len(out) == 1 else torch.cat(out)


@torch.no_grad()
def zero_shot_topk(model, image: torch.Tensor, bank: torch.Tensor, k: int = 5) -> Tuple[torch.Tensor, torch.Tensor]:
    """``zero_shot`` against a bank from ``encode_bank(model, text=...)``: ``(probs [B,k], idx [B,k])``, the k most
    probable candidates of every image and their softmax probabilities over the whole bank."""
    with _dense(model):
        q = _l2norm(model.encode_image(image.to(bank.device)))
    top = score_topk(q, bank, k, logit_scale=model.logit_scale, normalized=True)
    return torch.exp(top.values - top.lse[:, None]), top.indices


def metrics_from_ranks(rank: torch.Tensor, ks: Sequence[int] = (1, 5, 10)) -> Dict[str, float]:
    """Recall@k (fraction of queries whose target is among the first k), median and mean rank (1-based) from 0-based
    ranks; queries with rank -1 (no target) are left out, ``n`` is how many were counted."""
    r = rank.detach().reshape(-1).to("cpu", torch.float64)
    r = r[r >= 0]
    n = int(r.numel())
    nan = float("nan")
    out = {f"R@{k}": (float((r < k).double().mean()) if n else nan) for k in ks}
    out["median_rank"] = float(torch.quantile(r + 1, 0.5)) if n else nan
    out["mean_rank"] = float((r + 1).mean()) if n else nan
    out["n"] = n
    return out


@torch.no_grad()
def retrieval_metrics(image_features: torch.Tensor, text_features: torch.Tensor, text_of_image=None, image_of_text=None,
                      ks: Sequence[int] = (1, 5, 10)) -> Dict[str, float]:
    """Image->text (``i2t_``) and text->image (``t2i_``) retrieval over an evaluation set: ``text_of_image`` [n_img] is the
    text row that belongs to each image, ``image_of_text`` [n_txt] the image of each text (default: row i with row i)."""
    dev = image_features.device
    I, T = _l2norm(image_features), _l2norm(text_features)
    if text_of_image is None:
        text_of_image = torch.arange(I.shape[0], device=dev)
    if image_of_text is None:
        image_of_text = torch.arange(T.shape[0], device=dev)
    out = {}
    for prefix, q, b, tgt in (("i2t_", I, T, text_of_image), ("t2i_", T, I, image_of_text)):
        rank = score_topk(q, b, 1, target=tgt, normalized=True).rank
        out.update({prefix + key: v for key, v in metrics_from_ranks(rank, ks).items()})
    return out
