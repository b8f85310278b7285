#!/usr/bin/env python3
"""One form of the tower backward's in_proj bias gradient (started by tests/test_attention_fold_ops.py with CE_ATTN_FOLD=0 or
unset: the tower reads it once per process).  A 10-layer model -- more blocks than the partial-sum ring has slots --, width 128,
2 heads, 17 tokens in both towers, batch 3: the image tower runs dense, the text tower packed (captions of different lengths)
with ``sel_rows``, both with the pruned last block.  Saves every parameter gradient of one backward pass and, from the fp32
oracle of the same parameters, sum_i |dqkv[i, c]| per in_proj bias (the scale of its rounding bound) to the file named on the
command line.

    CE_ATTN_FOLD=0 python tests/attn_fold_child.py /tmp/atomic.pt
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LAYERS, WIDTH, HEADS, TOKENS, BATCH = 10, 128, 2, 17, 3


def column_magnitudes(O, cfg, sd, img, txt, labels):
    """{in_proj bias name: sum over rows of |d loss / d qkv|, [3 width]} in fp32: each bias enters the oracle as one copy per row,
    so its gradient is the per-row dqkv."""
    import torch
    q = {k: v.detach().clone().requires_grad_(True) for k, v in sd.items()}
    rows = {}
    for name in sd:
        if name.endswith("attn.in_proj_bias"):
            rows[name] = sd[name].detach().expand(BATCH, TOKENS, -1).clone().requires_grad_(True)
            q[name] = rows[name]
    yi, yt, ip = labels
    ld = O.criterion_contrastive(*O.clip_forward(q, cfg, img, txt), yi, yt, ip)
    sum(ld.values()).backward()
    return {name: t.grad.abs().sum((0, 1)) for name, t in rows.items()}


def main(out):
    import torch
    from oracle import clip_oracle as O
    from clip_event_amd import synthetic as S
    from clip_event_amd.losses import CriterionContrastive
    from clip_event_amd.model import build_model
    dev = "cuda:0"
    cfg = O.ClipConfig(64, 128, LAYERS, WIDTH, 32, TOKENS, 512, WIDTH, HEADS, LAYERS)
    assert cfg.vision_tokens == TOKENS and cfg.vision_heads == HEADS
    sd = O.init_params(cfg, 11)
    m = build_model({k: v.clone() for k, v in sd.items()}).to(dev)
    img = S.synthetic_images(BATCH, cfg.image_resolution, seed=1)
    txt = S.synthetic_tokens(BATCH, cfg.context_length, cfg.vocab_size, seed=2, min_len=2)
    labels = O.build_labels(BATCH, 1, 0, True)
    lens = (txt.argmax(dim=-1) + 1).tolist()
    assert len(set(lens)) > 1 and min(lens) < TOKENS, f"captions {lens}: the text tower would not run packed"
    yi, yt, ip = (t.to(dev) for t in labels)
    m.zero_grad()
    ld = CriterionContrastive("ce")(*m(img.to(dev), txt.to(dev)), yi, yt, index_pos=ip)
    sum(ld.values()).backward()
    torch.cuda.synchronize()
    grads = {n: p.grad.detach().float().cpu().clone() for n, p in m.named_parameters() if p.grad is not None}
    mags = column_magnitudes(O, cfg, sd, img, txt, labels)
    torch.save({"attn_fold": int(os.environ.get("CE_ATTN_FOLD", "1")), "lens": lens, "grads": grads, "mags": mags}, out)
    print(f"captions {lens}, {len(grads)} gradients, {len(mags)} in_proj biases", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
