"""References for the patch-dropout tests (no GPU): a numpy restatement of the ``ce_patch_keep`` sampler as
include/clip_event_hip.h states it, and the oracle's image tower restated with a keep list."""
import numpy as np
import torch

_M32 = np.uint64(0xFFFFFFFF)


def fmix32(h):
    """murmur3 finaliser on uint32 (held in uint64 arrays so that no intermediate product is lost)."""
    h = np.asarray(h, dtype=np.uint64) & _M32
    h = h ^ (h >> np.uint64(16))
    h = (h * np.uint64(0x85EBCA6B)) & _M32
    h = h ^ (h >> np.uint64(13))
    h = (h * np.uint64(0xC2B2AE35)) & _M32
    return h ^ (h >> np.uint64(16))


def patch_keys(seed, draws, samples, N):
    """Keys [len(draws), len(samples), N] (uint64 holding uint32 values) of every patch."""
    a = fmix32(np.uint64((int(seed) + 0x9E3779B9) & 0xFFFFFFFF))
    b = fmix32(a ^ (np.asarray(draws, dtype=np.uint64) & _M32))
    c = fmix32(b[:, None] ^ (np.asarray(samples, dtype=np.uint64) & _M32)[None, :])
    return fmix32(c[:, :, None] ^ np.arange(N, dtype=np.uint64)[None, None, :])


def keep_sets(seed, draws, samples, N, keep):
    """Kept patches, ascending: int64 [len(draws), len(samples), keep] -- the ``keep`` smallest keys of every sample."""
    keys = patch_keys(seed, draws, samples, N)
    assert all(len(np.unique(row)) == N for row in keys.reshape(-1, N)[:4])       # a bijection: no ties
    return np.sort(np.argsort(keys, axis=-1, kind="stable")[..., :keep], axis=-1)


def keep_tables(seed, draw, sample0, B, N, keep):
    """What one ``ce_patch_keep`` launch writes: (keep_idx int32 [B, keep], inv int32 [B, N])."""
    idx = keep_sets(seed, [draw], [(sample0 + b) & 0xFFFFFFFF for b in range(B)], N, keep)[0].astype(np.int32)
    inv = np.full((B, N), -1, dtype=np.int32)
    for b in range(B):
        inv[b, idx[b]] = np.arange(keep, dtype=np.int32)
    return idx, inv


def encode_image_keep(p, cfg, image, keep_idx, bf16=False):
    """oracle.clip_oracle.encode_image (CLS output) on the class token and the patches ``keep_idx`` [B, keep] only: token
    1 + j of sample b is the patch embedding of patch keep_idx[b, j] plus positional row 1 + keep_idx[b, j]."""
    from oracle.clip_oracle import _r, _s, layer_norm, residual_block
    B = image.shape[0]
    ps, g, vw = cfg.vision_patch_size, cfg.grid, cfg.vision_width
    idx = torch.as_tensor(np.asarray(keep_idx), dtype=torch.long)
    x = image.float().reshape(B, 3, g, ps, g, ps).permute(0, 2, 4, 1, 3, 5).reshape(B, g * g, 3 * ps * ps)
    x = torch.gather(x, 1, idx[:, :, None].expand(-1, -1, x.shape[-1]))
    x = _r(x, bf16) @ _r(p["visual.conv1.weight"].reshape(vw, -1), bf16).t()   # [B, keep, vw]
    pos = p["visual.positional_embedding"]
    cls = (p["visual.class_embedding"] + pos[0]).expand(B, 1, vw)
    x = torch.cat([cls, x + pos[1 + idx]], dim=1)
    x = _s(layer_norm(x, p["visual.ln_pre.weight"], p["visual.ln_pre.bias"]))
    for i in range(cfg.vision_layers):
        x = residual_block(x, p, f"visual.transformer.resblocks.{i}.", cfg.vision_heads, None, bf16)
    x = layer_norm(x[:, 0, :], p["visual.ln_post.weight"], p["visual.ln_post.bias"])
    return _r(x, bf16) @ _r(p["visual.proj"], bf16)
