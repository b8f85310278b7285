#!/usr/bin/env python3
"""The reference's training loop (train.py:101-250 / engine.py:24-102) on the drop-in API, end to end on synthetic
data: decoded uint8 images -> on-device preprocessing -> CLIP forward (hard-negative descriptions, per-batch labels as
dataset_voa.py builds them) -> CriterionContrastive -> fused clip + Adam (``--optimizer sgd``: fused clip + SGD with momentum,
the reference's other optimiser; ``--optimizer lion``: fused clip + Lion, optim.FusedLion, at a tenth of Adam's rate as its paper
advises) -> warm-up cosine schedule -> checkpoint in
the reference's layout -> resume from it.  A smoke run of every host-side component together, not a benchmark.

``--micro-batch N`` runs every step in chunks of N images (engine.train_step(micro_batch=N): the step for batches whose
activation stash does not fit).

Partial fine-tuning: ``--lock-image-tower`` / ``--lock-text-tower`` freeze a tower (``--unlocked-layers N``: except its top N blocks
and its output side), ``--no-decay-groups`` puts gains, biases and ``logit_scale`` into a parameter group without weight decay,
``--adamw`` decouples the decay (``--optimizer adam`` only; both with a weight decay of 0.1; the fused step stays in use; Lion's decay
is always decoupled).

``--patch-dropout P`` trains the image tower on a random ``1 - P`` of the patches of every image (CLIP.set_patch_dropout).

``--loss sigmoid`` trains with the sigmoid pairwise loss of SigLIP (losses.CriterionSigmoid on the fused sigmoid head) and its
learnable logit bias (``CLIP.enable_logit_bias``; ``--logit-bias INIT``, default -10); the checkpoint carries the bias.

``--loss multipos --positives P`` trains with P positive captions per image (``distributed.global_groups``: the first P of every
image's P + 2 captions carry its group id) on ``losses.CriterionMultiPositive`` (the fused multi-positive head: each row's target is
uniform over its positives); ``--positives P`` with ``--loss sigmoid`` is ``CriterionSigmoid(multi_positive=True)`` on the same layout.

``--distill-arch ARCH`` adds knowledge distillation (``engine.Distillation``: ``loss_dist_i`` / ``loss_dist_t``; at this batch size
on logits + ``losses.CriterionDistill``, CE_FUSED_HEAD=1 for the fused distillation head) from a frozen teacher of the named geometry, randomly initialised or loaded from ``--distill-checkpoint``;
``--distill-weight W`` scales the two terms.  A teacher of another resolution gets the batch resized to its own.

``--ema DECAY`` keeps an exponential moving average of the weights in the fused step (``optimizer.enable_ema``; ``--ema-warmup``:
the ramped decay of ``optim.ema_rate``); the checkpoint carries it, the resumed run restores it, and the end prints
``inference.retrieval_metrics`` on the fixed batch for the raw and for the averaged weights (``optimizer.averaged()``).

``--augment`` replaces the evaluation transform by open_clip's training transform on the device (``preprocess.Augment``:
``RandomResizedCrop(scale=(0.9, 1.0))``; ``--aug-scale``, ``--aug-hflip``, ``--aug-color-jitter B C S H``, ``--aug-color-jitter-prob``,
``--aug-gray-scale-prob`` are its ``--aug-cfg`` fields) with ``draw`` = the step, so that the run resumed at step 20 sees the crops the
first run would have seen there.

``--lora RANK`` (``--lora-alpha A``, ``--lora-targets ...``, ``--lora-layers N``) trains low-rank adapters on the block matrices over a
frozen base (``CLIP.enable_lora``) at 100 x the learning rate; the checkpoint carries the adapters and their config, and the model
read back has them.

``--image-size R`` runs and trains the image tower at ``R`` x ``R`` instead of the checkpoint's own resolution (``CLIP.set_image_size``:
the positional table is resampled, the parameter keeps its shape); ``--image-size-schedule STEP:R ...`` changes the size at the given
steps (progressive resizing: cheap low-resolution steps first).  The synthetic images, the augmentation and the evaluation pass
follow the size; the setting is not in the checkpoint, so the resumed run sets it again.

``--context-length T`` (``--context-keep K``) runs and trains the text tower on ``T``-token rows instead of the checkpoint's 77
(``CLIP.set_context_length``: the first K rows of the positional table copied, the rest stretched; the parameter keeps its shape).  The
captions are tokenised at ``T`` and, beyond 77 tokens, padded out with repeated sentences so that some exceed the 128 tokens of the short
attention kernels.  Like the image size the setting is not in the checkpoint: the resumed run sets it again."""
import argparse
import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from clip_event_amd import checkpoint, clip, distributed as D, inference, synthetic as S
from clip_event_amd.engine import Distillation, train_step as engine_train_step
from clip_event_amd.losses import CriterionContrastive, CriterionMultiPositive, CriterionSigmoid
from clip_event_amd.optim import FusedAdam, FusedLion, FusedSGD, build_lr_scheduler, build_optimizer, no_decay_groups
from clip_event_amd.preprocess import Augment, preprocess

CAPTIONS = list(S.ASCII_CAPTIONS)


def batch(rng, B, K, dev, aug=None, draw=0, n_px=224, positives=None, context=77):
    sizes = [(int(rng.integers(240, 640)), int(rng.integers(240, 640))) for _ in range(B)]
    imgs = [torch.from_numpy(rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)).to(dev) for (w, h) in sizes]
    image = preprocess(imgs, n_px=n_px) if aug is None else aug(imgs, draw=draw)   # clip.py:62-69 / the training transform, on the GPU
    texts = [CAPTIONS[int(rng.integers(len(CAPTIONS)))] + f" number {int(rng.integers(1000))}" for _ in range(B * K)]
    if context > 77:                                                            # long captions: a third of them several sentences long
        texts = [t if i % 3 else " ".join([t] * int(rng.integers(2, 2 + context // 16))) for i, t in enumerate(texts)]
    text = clip.tokenize(texts, context_length=context)                                               # clip.py:168-201: stays on the HOST, as the reference's loader
                                                                                # yields it -- train_step copies it and keeps the caption lengths
    if positives is None:
        yi, yt, ip = D.global_labels(B, 1, K - 1, True, device=dev)             # dataset_voa.py:605-664
    else:                                                                       # group ids: the first `positives` captions of an image
        yi, yt, ip = D.global_groups(B, positives, K - positives, device=dev)
    return (image, text, yi, yt, ip), imgs


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--micro-batch", type=int, default=None, metavar="N", help="images per chunk of a step (default: unchunked)")
    ap.add_argument("--optimizer", choices=("adam", "sgd", "lion"), default="adam",
                    help="cfg['optimizer'] of engine.py:129-151, or 'lion' (optim.FusedLion)")
    ap.add_argument("--lock-image-tower", action="store_true", help="freeze the image tower (CLIP.lock_image_tower)")
    ap.add_argument("--lock-text-tower", action="store_true", help="freeze the text tower (CLIP.lock_text_tower)")
    ap.add_argument("--unlocked-layers", type=int, default=0, metavar="N", help="blocks a locked tower keeps trainable, from the top")
    ap.add_argument("--no-decay-groups", action="store_true", help="optim.no_decay_groups: no weight decay on gains, biases, logit_scale")
    ap.add_argument("--adamw", action="store_true", help="decoupled weight decay (FusedAdam(decoupled=True))")
    ap.add_argument("--patch-dropout", type=float, default=0.0, metavar="P",
                    help="train the image tower on a random 1 - P of the patches (CLIP.set_patch_dropout)")
    ap.add_argument("--ema", type=float, default=None, metavar="DECAY", help="weight EMA in the fused step (optimizer.enable_ema)")
    ap.add_argument("--ema-warmup", action="store_true", help="with --ema: ramp the decay up (optim.ema_rate)")
    ap.add_argument("--loss", choices=("ce", "sigmoid", "multipos"), default="ce",
                    help="contrastive criterion: InfoNCE, the sigmoid pairwise loss, or InfoNCE over a set of positives per row")
    ap.add_argument("--positives", type=int, default=None, metavar="P",
                    help="with --loss multipos (default 2) or --loss sigmoid: positive captions per image, labels as group ids")
    ap.add_argument("--logit-bias", type=float, default=None, metavar="INIT",
                    help="with --loss sigmoid: initial logit bias (default -10)")
    ap.add_argument("--distill-arch", choices=sorted(S.GEOMETRY), default=None, metavar="ARCH",
                    help="distil from a frozen teacher of this geometry (engine.Distillation)")
    ap.add_argument("--distill-weight", type=float, default=1.0, metavar="W", help="with --distill-arch: weight of the two terms")
    ap.add_argument("--distill-checkpoint", default=None, metavar="PATH", help="with --distill-arch: the teacher's checkpoint")
    ap.add_argument("--augment", action="store_true", help="open_clip's training transform on the device (preprocess.Augment), draw = step")
    ap.add_argument("--aug-scale", type=float, nargs=2, default=None, metavar=("LO", "HI"), help="with --augment: RandomResizedCrop scale (0.9 1.0)")
    ap.add_argument("--aug-hflip", type=float, default=None, metavar="P", help="with --augment: probability of a horizontal flip (0)")
    ap.add_argument("--aug-color-jitter", type=float, nargs=4, default=None, metavar=("B", "C", "S", "H"),
                    help="with --augment: ColorJitter(brightness, contrast, saturation, hue)")
    ap.add_argument("--aug-color-jitter-prob", type=float, default=None, metavar="P", help="with --aug-color-jitter: its probability (0.8)")
    ap.add_argument("--aug-gray-scale-prob", type=float, default=None, metavar="P", help="with --augment: RandomGrayscale probability (0)")
    ap.add_argument("--lora", type=int, default=None, metavar="RANK", help="low-rank adapters on the block matrices (CLIP.enable_lora); the base is frozen")
    ap.add_argument("--lora-alpha", type=float, default=None, metavar="A", help="with --lora: alpha (default 2 x RANK)")
    ap.add_argument("--lora-targets", nargs="+", default=None, metavar="T", help="with --lora: of in_proj out_proj c_fc c_proj (default all)")
    ap.add_argument("--lora-layers", type=int, default=None, metavar="N", help="with --lora: the top N blocks of each tower only")
    ap.add_argument("--image-size", type=int, default=None, metavar="R", help="run the image tower at R x R (CLIP.set_image_size)")
    ap.add_argument("--image-size-schedule", nargs="+", default=(), metavar="STEP:R", help="from step STEP on, run at R x R")
    ap.add_argument("--context-length", type=int, default=None, metavar="T", help="run the text tower on T-token rows (CLIP.set_context_length)")
    ap.add_argument("--context-keep", type=int, default=20, metavar="K", help="with --context-length: leading positions copied, not stretched")
    args = ap.parse_args()
    try:
        schedule = sorted((int(a), int(b)) for a, b in (item.split(":") for item in args.image_size_schedule))
    except ValueError:
        ap.error("--image-size-schedule takes STEP:R pairs of integers")
    aug_cfg = {k: v for k, v in (("scale", args.aug_scale), ("hflip", args.aug_hflip), ("color_jitter", args.aug_color_jitter),
                                 ("color_jitter_prob", args.aug_color_jitter_prob), ("gray_scale_prob", args.aug_gray_scale_prob))
               if v is not None}
    if aug_cfg and not args.augment:
        ap.error("--aug-* options go with --augment")
    if args.distill_arch is None and (args.distill_checkpoint is not None or args.distill_weight != 1.0):
        ap.error("--distill-weight / --distill-checkpoint go with --distill-arch")
    if args.logit_bias is not None and args.loss != "sigmoid":
        ap.error("--logit-bias goes with --loss sigmoid")
    if args.positives is not None and (args.loss == "ce" or args.positives < 1):
        ap.error("--positives P >= 1 goes with --loss multipos or --loss sigmoid")
    if args.loss == "multipos" and args.positives is None:
        args.positives = 2
    if args.ema_warmup and args.ema is None:
        ap.error("--ema-warmup goes with --ema")
    if args.adamw and args.optimizer != "adam":
        ap.error("--adamw goes with --optimizer adam")
    if args.lora is None and (args.lora_alpha is not None or args.lora_targets is not None or args.lora_layers is not None):
        ap.error("--lora-alpha / --lora-targets / --lora-layers go with --lora")
    mb = args.micro_batch
    dev = torch.device("cuda", 0)
    # (SGD's clipped step is lr x a unit-norm gradient: it needs a far larger lr than Adam's per-element lr to move the loss; Lion's
    # step is lr per element whatever the gradient is: a tenth of Adam's rate, as its paper advises)
    cfg = {"optimizer": args.optimizer, "lr": {"adam": 1e-5, "lion": 1e-6, "sgd": 0.05}[args.optimizer], "weight_decay": 0.0, "momentum": 0.9, "lr_scheduler": "warmup",
           "max_epoch": 40, "warmup_epoch": 4, "lr_steps": [], "lr_gamma": 0.1, "task": "clipevent"}
    B, K = 16, 3 if args.positives is None else args.positives + 2
    P = args.positives
    rng = np.random.default_rng(0)
    model = S.synthetic_model("vit_b32", seed=0).to(dev)
    model.set_hyps(constrastive_overbatch=True, alignment=False, multiattention=False)
    criterion = {"ce": lambda: CriterionContrastive("ce"), "sigmoid": lambda: CriterionSigmoid(multi_positive=P is not None),
                 "multipos": CriterionMultiPositive}[args.loss]()
    if args.loss == "sigmoid":
        model.enable_logit_bias(-10.0 if args.logit_bias is None else args.logit_bias)      # before the optimiser is built
    if args.no_decay_groups or args.adamw:
        cfg["weight_decay"] = 0.1
    if args.lora is not None:
        # B starts at 0 and only the adapters move: the usual adapter rates are 10 - 100 x the full fine-tuning rate
        cfg["lr"] *= 100.0

    def lock(m):
        if args.lora is not None and m.lora_config() is None:          # (a model read from a checkpoint brings its adapters along)
            m.enable_lora(rank=args.lora, alpha=2.0 * args.lora if args.lora_alpha is None else args.lora_alpha,
                          targets=args.lora_targets or ("in_proj", "out_proj", "c_fc", "c_proj"), layers=args.lora_layers)
        if args.lock_image_tower:
            m.lock_image_tower(args.unlocked_layers)
        if args.lock_text_tower:
            m.lock_text_tower(args.unlocked_layers)

    def make_optimizer(m):
        if not (args.no_decay_groups or args.adamw):
            return build_optimizer(cfg, m)                                      # engine.py:129-151; frozen parameters: still the fused step
        groups = no_decay_groups(m, cfg["weight_decay"]) if args.no_decay_groups else None
        if args.optimizer == "adam":
            return FusedAdam(m, lr=cfg["lr"], weight_decay=cfg["weight_decay"], max_norm=1.0, decoupled=args.adamw, groups=groups)
        if args.optimizer == "lion":
            return FusedLion(m, lr=cfg["lr"], weight_decay=cfg["weight_decay"], max_norm=1.0, groups=groups)
        return FusedSGD(m, lr=cfg["lr"], momentum=cfg["momentum"], weight_decay=cfg["weight_decay"], max_norm=1.0, groups=groups)

    train_step = engine_train_step
    if args.distill_arch is not None:
        if args.distill_checkpoint is not None:
            teacher = checkpoint.load_checkpoint(args.distill_checkpoint, device=dev)[0]
        else:
            teacher = S.synthetic_model(args.distill_arch, seed=1).to(dev)
        distill = Distillation(teacher, weight=args.distill_weight)
        res = int(teacher.visual.input_resolution)

        def train_step(m, crit, opt, image, *rest, **kw):
            timg = None
            if image.shape[-1] != res:              # the teacher's own resolution
                timg = torch.nn.functional.interpolate(image.float(), size=(res, res), mode="bilinear", align_corners=False).to(image.dtype)
            return engine_train_step(m, crit, opt, image, *rest, distill=distill, teacher_image=timg, **kw)

    native = int(model.visual.native_resolution)

    def size_at(step):
        size = native if args.image_size is None else args.image_size
        for first, r in schedule:
            if step >= first:
                size = r
        return size

    augs = {}

    def aug_at(size):
        """The training transform at ``size`` (one per size: all of them count the same draws), or None."""
        if not args.augment:
            return None
        if size not in augs:
            augs[size] = Augment(size, seed=0, **aug_cfg)
        return augs[size]

    def images_at(size, imgs, draw):
        return preprocess(imgs, n_px=size) if not args.augment else aug_at(size)(imgs, draw=draw)

    lock(model)
    model.set_patch_dropout(args.patch_dropout, seed=0)
    size = model.set_image_size(size_at(0))           # a ValueError names the rule a bad size breaks
    ctx = model.set_context_length(args.context_length, keep=args.context_keep)      # likewise
    optimizer = make_optimizer(model)
    if args.ema is not None:
        optimizer.enable_ema(args.ema, warmup=args.ema_warmup)
    scheduler = build_lr_scheduler(cfg, optimizer, 0)                           # engine.py:154-176
    aug = aug_at(size)
    data, decoded = batch(rng, B, K, dev, aug, n_px=size, positives=P, context=ctx)          # one fixed batch: the loss must fall
    losses = []
    for it in range(20):
        if size_at(it) != size:                                                 # progressive resizing: the same images at the new size
            size = model.set_image_size(size_at(it))
            aug = aug_at(size)
            data = (images_at(size, decoded, it),) + data[1:]
        elif aug is not None:
            data = (aug(decoded, draw=it),) + data[1:]                          # the same images, cropped (jittered) anew every step
        ld = train_step(model, criterion, optimizer, *data, check_finite=True, micro_batch=mb)
        scheduler.step()
        losses.append(float(sum(v.detach() for v in ld.values())))
    print("loss:", " ".join(f"{v:.3f}" for v in losses[::3]), "lr", optimizer.param_groups[0]["lr"])
    # (a locked tower, or an image tower that sees other patches every step, cannot follow the fixed batch as fast: the loss
    # must still fall; so must the sigmoid loss, which starts at about |logit_bias| per image -- every positive pair far on the
    # wrong side -- and has 20 steps at lr 1e-5 to pull the positives up; so must Lion's, which at a tenth of Adam's rate moves
    # every weight by at most 1e-6 per step where Adam's first steps move it by 1e-5: measured 6.72 -> 5.81)
    # (with P positives per image the image rows cannot go below log P: the uniform target over P unrelated captions)
    slow = (args.lock_image_tower or args.lock_text_tower or args.patch_dropout or args.loss != "ce" or args.distill_arch
            or args.optimizer == "lion" or args.augment or args.lora is not None or schedule)
    assert losses[-1] < (0.5 if not slow else 1.0) * losses[0]
    with tempfile.TemporaryDirectory() as d:
        path = checkpoint.save_model_on_master(model, d, cfg["task"], 20, 0.0, optimizer)      # engine.py:202-218
        model2, opt_state, begin_epoch, _ = checkpoint.load_checkpoint(path, device=dev)       # train.py:101-124
        assert (getattr(model2, "logit_bias", None) is not None) == (args.loss == "sigmoid")   # build_model enables it from the key
        assert model2.lora_config() == model.lora_config()                                      # the checkpoint's 'lora' entry
        lock(model2)
        # neither the rate nor the draw counter is in the checkpoint: a resumed run sets them again
        model2.set_patch_dropout(args.patch_dropout, seed=0)
        model2.patch_draw = model.patch_draw
        assert model2.visual.input_resolution == native                                         # nor is the run size
        assert model2.context_length == model2.native_context_length                           # nor is the run length
        model2.set_context_length(args.context_length, keep=args.context_keep)
        size = model2.set_image_size(size_at(20))
        if size != model.visual.input_resolution:
            model.set_image_size(size)
            data = (images_at(size, decoded, 20),) + data[1:]
        optimizer2 = make_optimizer(model2)
        optimizer2.load_state_dict(opt_state)
        ema = checkpoint.load_ema(path)
        assert (ema is not None) == (args.ema is not None)
        if ema is not None:
            optimizer2.load_ema_state_dict(ema)                                               # decay, warm-up, update count, average
            assert optimizer2.ema_updates == optimizer.ema_updates == 20
        scheduler2 = build_lr_scheduler(cfg, optimizer2, begin_epoch)
    if aug is not None:
        # the draws are a hash of (seed, rank, draw, sample): a resumed run needs the settings and the step, nothing else
        aug = aug_at(size)
        aug.draw = 20
        aug2 = Augment(model2.visual.input_resolution, seed=0, **aug_cfg)
        aug2.load_state_dict(aug.state_dict())
        data = (aug2(decoded),) + data[1:]
        assert aug2.draw == 21 and torch.equal(data[0], aug(decoded, draw=20)) and not torch.equal(data[0], aug(decoded, draw=19))
        print("resumed run draws the crops of step 20 again")
    assert begin_epoch == 20 and abs(optimizer2.param_groups[0]["lr"] - optimizer.param_groups[0]["lr"]) < 1e-12
    a = train_step(model, criterion, optimizer, *data, micro_batch=mb)
    b = train_step(model2, criterion, optimizer2, *data, micro_batch=mb)
    la, lb = float(sum(v.detach() for v in a.values())), float(sum(v.detach() for v in b.values()))
    print(f"resumed run continues: loss {la:.5f} vs {lb:.5f}")
    assert abs(la - lb) < 1e-3 * max(1.0, abs(la))
    new, _ = batch(rng, B, K, dev, aug, 21, n_px=size, positives=P, context=ctx)                          # a fresh ragged batch goes through too
    ld = train_step(model2, criterion, optimizer2, *new, micro_batch=mb)
    scheduler2.step()
    assert all(torch.isfinite(v) for v in ld.values())
    # a longer stretch of fresh batches with no host synchronisation in the loop: host-side caption lengths, the run-ahead
    # limit of engine.train_step, the asynchronous poll of the fp16-stream clamp counters (every 16 optimiser steps)
    import time
    batches = [batch(rng, 32, K, dev, aug, 22 + i, n_px=size, positives=P, context=ctx)[0] for i in range(8)]
    for it in range(4):                                                         # new batch size: workspaces are allocated here
        train_step(model2, criterion, optimizer2, *batches[it], micro_batch=mb)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for it in range(96):
        ld = train_step(model2, criterion, optimizer2, *batches[it % 8], micro_batch=mb)
        scheduler2.step()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / 96
    assert all(torch.isfinite(v) for v in ld.values()) and model2.stream16_saturation() == (0, 0)
    print(f"96 steps at B = 32, K = {K}, {size} px, {ctx} tokens: {dt * 1e3:.2f} ms/step, clamp counters {model2.stream16_saturation()}")
    if args.ema is not None:
        image, text, _, _, ip = data

        def retrieval():                                                        # the fixed batch: every image against its own caption
            with torch.no_grad(), model2.no_patch_dropout():                    # an evaluation sees every patch (--patch-dropout)
                fi, ft = model2.encode_image(image), model2.encode_text(text.to(dev)[ip])
            return inference.retrieval_metrics(fi, ft)

        raw = retrieval()
        with optimizer2.averaged():
            avg = retrieval()
        for name, r in (("raw", raw), ("averaged", avg)):
            print(f"retrieval on the fixed batch, {name:8s} weights:", " ".join(f"{k} {v:.3f}" for k, v in r.items()))
        assert optimizer2.ema_updates == 20 + 2 + 4 + 96 and retrieval() == raw
    print("train_synthetic OK")


if __name__ == "__main__":
    main()
