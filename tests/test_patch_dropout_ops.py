"""GPU: the four patch-dropout kernels of csrc/embed.hip, one at a time.

* ``ce_patch_keep`` equals the numpy restatement of the hash (tests/patch_dropout_ref.py) exactly, both tables.
* ``ce_im2col_rows`` equals the gathered rows of ``ce_im2col`` bit for bit, on the 16-byte path and on the generic one.
* ``ce_vision_assemble_rows`` equals the fp32 torch expression bit for bit (one fp32 add per element).
* ``ce_pos_embed_bwd_rows`` against an fp64 ``index_add``; untouched rows stay as they were; two runs agree bit for bit."""
import numpy as np
import pytest
import torch

from tests import patch_dropout_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _call(name, *args):
    from clip_event_amd._lib import check, lib, ptr, stream
    check(getattr(lib(), name)(*[ptr(a) if isinstance(a, torch.Tensor) else a for a in args], stream()), name)


def _patch_keep(seed, draw, sample0, B, N, keep, want_inv=True):
    from clip_event_amd._lib import ptr
    idx = torch.full((B, keep), -7, dtype=torch.int32, device=DEV)
    inv = torch.full((B, N), -7, dtype=torch.int32, device=DEV)
    _call("ce_patch_keep", seed, draw, sample0, B, N, keep, idx, inv if want_inv else ptr(None))
    torch.cuda.synchronize()
    return idx.cpu().numpy(), inv.cpu().numpy()


@pytest.mark.parametrize("B,N,keep", [(5, 36, 18), (3, 576, 144), (2, 49, 1), (2, 4, 4), (1, 1024, 256)])
def test_patch_keep_equals_the_restatement(B, N, keep):
    for seed, draw, sample0 in ((0, 0, 0), (12345, 3, 0), (1, 2, 1000), (2 ** 31 + 5, 7, 3), (2 ** 32 - 1, 2 ** 31, 2 ** 32 - 2)):
        idx, inv = _patch_keep(seed, draw, sample0, B, N, keep)
        ref_idx, ref_inv = R.keep_tables(seed, draw, sample0, B, N, keep)
        assert (idx == ref_idx).all(), (seed, draw, sample0)
        assert (inv == ref_inv).all(), (seed, draw, sample0)


def test_patch_keep_without_inverse_table_and_bad_shapes():
    from clip_event_amd._lib import lib, ptr
    idx, inv = _patch_keep(4, 1, 0, 3, 36, 18, want_inv=False)
    assert (idx == R.keep_tables(4, 1, 0, 3, 36, 18)[0]).all() and (inv == -7).all()
    t = torch.zeros(4096 * 2, dtype=torch.int32, device=DEV)
    for B, N, keep in ((1, 36, 0), (1, 36, 37), (1, 4096, 8), (0, 36, 18)):
        assert lib().ce_patch_keep(0, 0, 0, B, N, keep, ptr(t), ptr(None), None) != 0


@pytest.mark.parametrize("B,res,patch,kp", [(3, 96, 16, 768), (2, 56, 14, 640), (2, 64, 32, 3072)])
def test_im2col_rows_equals_gathered_im2col(B, res, patch, kp):
    g = res // patch
    N, keep = g * g, max(1, (g * g) // 2)
    rng = np.random.default_rng(res)
    img = torch.from_numpy(rng.standard_normal((B, 3, res, res)).astype(np.float32)).to(DEV)
    dense = torch.full((B * N, kp), 7.0, dtype=torch.bfloat16, device=DEV)
    _call("ce_im2col", img, dense, B, res, patch, kp)
    for idx_np in (R.keep_tables(3, 0, 0, B, N, keep)[0], np.tile(np.arange(N, dtype=np.int32), (B, 1)),
                   np.full((B, 1), N - 1, dtype=np.int32)):
        k = idx_np.shape[1]
        idx = torch.from_numpy(idx_np).to(DEV)
        rows = torch.full((B * k, kp), 7.0, dtype=torch.bfloat16, device=DEV)
        _call("ce_im2col_rows", img, idx, rows, B, k, res, patch, kp)
        torch.cuda.synchronize()
        want = dense.view(B, N, kp)[torch.arange(B, device=DEV)[:, None], idx.long()].reshape(B * k, kp)
        assert torch.equal(rows.view(torch.int16), want.view(torch.int16))
        if kp > 3 * patch * patch:
            assert float(rows[:, 3 * patch * patch:].abs().max()) == 0.0
    # an index outside 0..N-1 is clamped, not followed
    bad = torch.tensor([[-5, N + 100]] * B, dtype=torch.int32, device=DEV)
    rows = torch.empty((B * 2, kp), dtype=torch.bfloat16, device=DEV)
    _call("ce_im2col_rows", img, bad, rows, B, 2, res, patch, kp)
    torch.cuda.synchronize()
    want = dense.view(B, N, kp)[:, [0, N - 1]].reshape(B * 2, kp)
    assert torch.equal(rows.view(torch.int16), want.view(torch.int16))


@pytest.mark.parametrize("D", [128, 260])
def test_vision_assemble_rows_bit_exact(D):
    B, N, keep = 3, 36, 18
    rng = np.random.default_rng(D)
    t = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32)).to(DEV)      # noqa: E731
    patch, cls, pos = t(B * keep, D), t(D), t(N + 1, D)
    idx = torch.from_numpy(R.keep_tables(9, 1, 0, B, N, keep)[0]).to(DEV)
    x0 = torch.full((B, keep + 1, D), float("nan"), device=DEV)
    _call("ce_vision_assemble_rows", patch, idx, cls, pos, x0, B, N, keep, D)
    torch.cuda.synchronize()
    want = torch.cat([(cls + pos[0]).expand(B, 1, D), patch.view(B, keep, D) + pos[1 + idx.long()]], dim=1)
    assert torch.equal(x0, want)
    bad = idx.clone()
    bad[0, 0], bad[1, -1] = -3, N + 9            # clamped to patches 0 and N-1
    _call("ce_vision_assemble_rows", patch, bad, cls, pos, x0, B, N, keep, D)
    torch.cuda.synchronize()
    assert torch.equal(x0[0, 1], patch[0] + pos[1]) and torch.equal(x0[1, keep], patch[2 * keep - 1] + pos[N])


@pytest.mark.parametrize("B,N,keep,D", [(7, 36, 18, 128), (2, 49, 12, 128), (5, 49, 12, 260), (3, 256, 128, 1024), (2, 36, 36, 128)])
def test_pos_embed_bwd_rows(B, N, keep, D):
    rng = np.random.default_rng(B * N + D)
    dx0 = torch.from_numpy(rng.standard_normal((B, keep + 1, D)).astype(np.float32)).to(DEV)
    start = torch.from_numpy(rng.standard_normal((N + 1, D)).astype(np.float32)).to(DEV)
    idx_np, inv_np = R.keep_tables(2, 5, 0, B, N, keep)
    inv = torch.from_numpy(inv_np).to(DEV)
    outs = []
    for _ in range(2):
        dpos = start.clone()                      # accumulates into a non-zero buffer
        _call("ce_pos_embed_bwd_rows", dx0, inv, dpos, B, N, keep, D)
        torch.cuda.synchronize()
        outs.append(dpos)
    assert torch.equal(outs[0], outs[1])          # no atomics: the same bits every run
    ref = start.double().cpu()
    ref[0] += dx0[:, 0].double().cpu().sum(0)
    ref.index_add_(0, torch.from_numpy(1 + idx_np.reshape(-1)).long(), dx0[:, 1:].double().cpu().reshape(B * keep, D))
    rel = float((outs[0].double().cpu() - ref).norm() / ref.norm())
    print(f"B={B} N={N} keep={keep} D={D}: rel-L2 against fp64 index_add {rel:.2e}")
    assert rel <= 1e-6
    untouched = np.setdiff1d(np.arange(N), idx_np.reshape(-1))
    if keep < N and B * keep < N:
        assert len(untouched) > 0
    if len(untouched):
        rows = torch.from_numpy(1 + untouched).long().to(DEV)
        assert torch.equal(outs[0][rows], start[rows])
