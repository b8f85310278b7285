#!/usr/bin/env python3
"""Throughput of the on-device preprocessing (ce_preprocess) on a batch of decoded 640x480 uint8 images; with
``--augment``, also of the training transform (ce_augment): crop + flip only, and open_clip's full
``--aug-cfg`` set (colour jitter with probability 0.8, greyscale with probability 0.2), planned on the host every batch."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from clip_event_amd.preprocess import Augment, preprocess

B = 256
imgs = [torch.randint(0, 256, (480, 640, 3), dtype=torch.uint8, device="cuda:0") for _ in range(B)]


def measure(name, fn, N=50):
    for i in range(3):
        fn(i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(N):
        out = fn(3 + i)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / N
    print(f"{name}: {B} images 640x480 -> [B,3,224,224] fp32: {dt*1e3:.2f} ms/batch = {B/dt:,.0f} images/s "
          f"({B*480*640*3/dt/1e9:.1f} GB/s of source bytes)")


measure("preprocess", lambda i: preprocess(imgs))
if "--augment" in sys.argv[1:]:
    crop = Augment(224, hflip=0.5)
    full = Augment(224, hflip=0.5, color_jitter=(0.32, 0.32, 0.32, 0.08), color_jitter_prob=0.8, gray_scale_prob=0.2)
    measure("augment, crop + flip", lambda i: crop(imgs, draw=i))
    measure("augment, full aug-cfg", lambda i: full(imgs, draw=i))
    sizes = [(640, 480)] * B
    t0 = time.perf_counter()
    for i in range(20):
        full.plan(sizes, i)
    print(f"host planning alone (full aug-cfg): {(time.perf_counter() - t0) / 20 * 1e3:.2f} ms/batch")
