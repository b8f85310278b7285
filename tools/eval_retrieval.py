#!/usr/bin/env python3
"""Image<->text retrieval over N synthetic pairs: the synthetic model (clip_event_amd/synthetic.py) encodes N images and N
captions chunk by chunk (``inference.encode_bank``), ``inference.retrieval_metrics`` gives R@1/5/10 and the ranks in both
directions without the N x N matrix, and the same numbers are taken from a chunked ``(q @ k.T).topk`` + rank count in torch
on the same features.  Prints the metrics and the time of both (HIP events, warm-up, median over the repeats).

    python tools/eval_retrieval.py --n 8192 50000
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from clip_event_amd import synthetic as S
from clip_event_amd.inference import encode_bank, metrics_from_ranks, retrieval_metrics

DEV = "cuda:0"


def encode_pairs(model, n, chunk, seed):
    """Unit-norm features of n synthetic (image, caption) pairs; the inputs are generated chunk by chunk (50 k images are
    30 GB of pixels)."""
    res, ctx, vocab = model.visual.input_resolution, model.context_length, model.vocab_size
    img_f, txt_f = [], []
    for i in range(0, n, chunk):
        b = min(chunk, n - i)
        img_f.append(encode_bank(model, image=S.synthetic_images(b, res, seed=seed + i), chunk=chunk))
        txt_f.append(encode_bank(model, text=S.synthetic_tokens(b, ctx, vocab, seed=seed + i + 1), chunk=chunk))
    return torch.cat(img_f), torch.cat(txt_f)


def torch_ranks(q, k, target, kmax, chunk):
    """The baseline: per chunk of queries the [chunk, N] similarity block, its top-kmax, and the rank of the target by
    counting (score descending, index ascending)."""
    ranks, tops = [], []
    cols = torch.arange(k.shape[0], device=q.device)[None, :]
    for i in range(0, q.shape[0], chunk):
        s = q[i:i + chunk] @ k.t()
        t = target[i:i + chunk, None]
        st = s.gather(1, t)
        if kmax:
            tops.append(s.topk(min(kmax, k.shape[0]), dim=1).indices)
        ranks.append(((s > st) | ((s == st) & (cols < t))).sum(dim=1))
    return torch.cat(ranks), (torch.cat(tops) if kmax else None)


def torch_metrics(I, T, ks, chunk, topk=True):
    out = {}
    diag = torch.arange(I.shape[0], device=I.device)
    for prefix, q, k in (("i2t_", I, T), ("t2i_", T, I)):
        rank, _ = torch_ranks(q, k, diag, max(ks) if topk else 0, chunk)
        out.update({prefix + key: v for key, v in metrics_from_ranks(rank, ks).items()})
    return out


def time_ms(fn, repeats, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return statistics.median(times), min(times), max(times)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, nargs="+", default=[8192], help="pairs to encode and score")
    ap.add_argument("--geometry", default="vit_b32", choices=sorted(S.GEOMETRY))
    ap.add_argument("--encode-chunk", type=int, default=512)
    ap.add_argument("--torch-chunk", type=int, default=4096, help="query rows per similarity block of the torch baseline")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=999)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_retrieval needs a GPU: a time taken anywhere else says nothing")
    if args.repeats < 20:
        raise SystemExit("--repeats below 20: the median would not be trusted")
    ks = (1, 5, 10)
    model = S.synthetic_model(args.geometry).to(DEV)
    E = model.embed_dim
    for n in args.n:
        I, T = encode_pairs(model, n, args.encode_chunk, args.seed)
        torch.cuda.synchronize()
        ours = retrieval_metrics(I, T, ks=ks)
        base = torch_metrics(I, T, ks, args.torch_chunk)
        diff = sorted(key for key in ours if ours[key] != base[key])
        t_ours = time_ms(lambda: retrieval_metrics(I, T, ks=ks), args.repeats, args.warmup)
        t_base = time_ms(lambda: torch_metrics(I, T, ks, args.torch_chunk), args.repeats, args.warmup)
        t_count = time_ms(lambda: torch_metrics(I, T, ks, args.torch_chunk, topk=False), args.repeats, args.warmup)
        flops = 2 * 2.0 * n * n * E                      # both directions
        print(f"metrics N={n}: " + ", ".join(f"{key} {v:.4g}" for key, v in ours.items())
              + (f"; torch differs in {diff}" if diff else "; torch gives the same"), flush=True)
        print(f"eval_retrieval N={n} E={E}: retrieval_metrics {t_ours[0]:.2f} ms (median of {args.repeats}, {t_ours[1]:.2f}..{t_ours[2]:.2f}; "
              f"{flops / t_ours[0] / 1e9:.1f} TF/s on 4 N^2 E), torch chunked matmul + topk + count {t_base[0]:.2f} ms "
              f"({t_base[1]:.2f}..{t_base[2]:.2f}; without the topk, which the ranks do not need, {t_count[0]:.2f} ms; blocks of {min(args.torch_chunk, n)} x {n}, {min(args.torch_chunk, n) * n * 4 / 2**20:.0f} MiB)",
              flush=True)


if __name__ == "__main__":
    main()
