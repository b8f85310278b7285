#!/usr/bin/env python3
"""The loss heads alone, forward + backward, on synthetic features: the fused sigmoid pairwise head (``SigmoidHeadFn``: one
direction, three sweeps) against the fused InfoNCE head with both directions (``InfoNCEFn``: six sweeps and two merges) at
the same shape in the same process, alternating, each sample one HIP-event interval around one forward + backward; the median
and the spread (min .. max) of the samples are printed, and one JSON line at the end.

Shapes (images x texts x embed dim): 256 x 256 x 512 (config 2), 512 x 2560 x 512 (B = 512, K = 5, one process) and
4096 x 20480 x 512 (config 3's whole batch in one process: an 84 M-element logits matrix that neither head forms).
``--logits`` adds the logits + criterion path of both losses where its matrix stays below 1 GB.  ``--distill`` adds the
distillation row: the fused distillation head with both directions (``DistillHeadFn``, student width 512, teacher width 768)
against logits + ``CriterionDistill`` (four logits matrices) at all three shapes.  ``--topk`` adds ``ops.score_topk`` (k = 10, with
a target: pre-pass, sweep and merge, forward only) on the normalised features at the same shapes.  ``--multipos P`` adds the
multi-positive head with both directions (``MultiPosHeadFn``: the first P of every image's texts carry its group id; six sweeps and
two merges, as the InfoNCE pair, the second direction over P times as many rows)."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from clip_event_amd import ops
from clip_event_amd.functional import DistillHeadFn, InfoNCEFn, MultiPosHeadFn, SigmoidHeadFn, logits_from_features
from clip_event_amd.losses import CriterionContrastive, CriterionDistill, CriterionSigmoid

DEV = "cuda:0"
SHAPES = ((256, 256, 512), (512, 2560, 512), (4096, 20480, 512))


def sample(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--iters", type=int, default=30, help="timed samples per head and shape")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--logits", action="store_true", help="also time logits + criterion")
    ap.add_argument("--distill", action="store_true", help="also time the distillation head, fused and on logits")
    ap.add_argument("--topk", action="store_true", help="also time ops.score_topk (k = 10, with a target)")
    ap.add_argument("--multipos", type=int, default=0, metavar="P", help="also time the multi-positive head, P positives per image")
    ap.add_argument("--teacher-dim", type=int, default=768)
    args = ap.parse_args()
    torch.manual_seed(0)
    results = []
    for nq, nk, E in SHAPES:
        K = nk // nq
        fi = torch.randn(nq, E, device=DEV, requires_grad=True)
        ft = torch.randn(nk, E, device=DEV, requires_grad=True)
        ls = torch.tensor(2.659, device=DEV, requires_grad=True)
        lb = torch.tensor(-10.0, device=DEV, requires_grad=True)
        yi = torch.arange(nq, device=DEV) * K
        yt = torch.arange(nq, device=DEV).repeat_interleave(K)
        ip = torch.arange(0, nk, K, device=DEV)

        def sigmoid():
            SigmoidHeadFn.apply(fi, ft, ls, lb, yi, None).backward()

        def infonce():
            li, lt = InfoNCEFn.apply(fi, ft, ls, yi, None, yt, ip)
            (li + lt).backward()

        heads = {"sigmoid": sigmoid, "infonce_pair": infonce}
        if args.logits and nq * nk * 4 < (1 << 30):
            crit_s, crit_c = CriterionSigmoid(), CriterionContrastive("ce")

            def sigmoid_logits():
                lpi, _ = logits_from_features(fi, ft, ls, True, want="image")
                crit_s(lpi, None, yi, logit_bias=lb)["loss_sig"].backward()

            def infonce_logits():
                ld = crit_c(*logits_from_features(fi, ft, ls, True), yi, yt, index_pos=ip)
                (ld["loss_i"] + ld["loss_t"]).backward()

            heads.update(sigmoid_logits=sigmoid_logits, infonce_logits=infonce_logits)
        if args.distill:
            tfi = torch.randn(nq, args.teacher_dim, device=DEV)
            tft = torch.randn(nk, args.teacher_dim, device=DEV)
            tls = torch.tensor(4.605, device=DEV)
            crit_d = CriterionDistill()

            def distill():
                li, lt = DistillHeadFn.apply(fi, ft, ls, tfi, tft, tls, None, True, ip)
                (li + lt).backward()

            def distill_logits():
                with torch.no_grad():
                    tlpi, tlpt = logits_from_features(tfi, tft, tls, True)
                ld = crit_d(*logits_from_features(fi, ft, ls, True), tlpi, tlpt, index_pos=ip)
                (ld["loss_dist_i"] + ld["loss_dist_t"]).backward()

            heads.update(distill=distill, distill_logits=distill_logits)
        if args.multipos:
            P = min(args.multipos, K)
            col = torch.arange(nk, device=DEV)
            gi = torch.arange(nq, device=DEV)
            gt = torch.where(col % K < P, col // K, torch.full_like(col, -1))
            ip_mp = torch.nonzero(col % K < P).flatten()

            def multipos():
                li, lt = MultiPosHeadFn.apply(fi, ft, ls, gi, gt, None, True, ip_mp)
                (li + lt).backward()

            heads.update(multipos=multipos)
        if args.topk:
            with torch.no_grad():
                qn, kn = torch.nn.functional.normalize(fi.detach(), dim=1), torch.nn.functional.normalize(ft.detach(), dim=1)
            lsd = ls.detach().reshape(1)

            def topk():
                ops.score_topk(qn, kn, 10, logit_scale=lsd, target=yi)

            heads.update(topk=topk)
        for fn in heads.values():
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        times = {name: [] for name in heads}
        for _ in range(args.iters):                      # alternate: both heads see the same clocks and neighbours
            for name, fn in heads.items():
                times[name].append(sample(fn))
        row = {"nq": nq, "nk": nk, "E": E}
        for name, ts in times.items():
            row[name] = {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts)}
        row["sigmoid_over_infonce_pair"] = row["sigmoid"]["median_ms"] / row["infonce_pair"]["median_ms"]
        if args.multipos:
            row["multipos_over_infonce_pair"] = row["multipos"]["median_ms"] / row["infonce_pair"]["median_ms"]
        if args.distill:
            row["distill_over_distill_logits"] = row["distill"]["median_ms"] / row["distill_logits"]["median_ms"]
        results.append(row)
        print(f"{nq} x {nk} x {E}: " + "; ".join(f"{name} {r['median_ms']:.3f} ms ({r['min_ms']:.3f} .. {r['max_ms']:.3f})"
                                                 for name, r in row.items() if isinstance(r, dict))
              + f"; sigmoid / InfoNCE pair {row['sigmoid_over_infonce_pair']:.2f}"
              + (f"; multipos / InfoNCE pair {row['multipos_over_infonce_pair']:.2f}" if args.multipos else "")
              + (f"; distill fused / logits {row['distill_over_distill_logits']:.2f}" if args.distill else ""), flush=True)
        del fi, ft
    print(json.dumps({"bench": "head", "iters": args.iters, "results": results}))


if __name__ == "__main__":
    main()
