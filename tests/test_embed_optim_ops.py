"""Op-level checks of the input-side gradient / bookkeeping kernels (csrc/embed.hip) and of clip + Adam (csrc/optim.hip)
against torch: bit for bit where a kernel only moves, adds once or rounds, against an fp64 sum where it accumulates.  Every
output lives inside a larger buffer whose other elements hold a sentinel and must come back unchanged.  Bounds per test."""
import math
from ctypes import c_float, c_int, c_long, c_void_p

import numpy as np
import pytest
import torch

DEV = "cuda:0"
U = 2.0 ** -24          # fp32 unit roundoff
gpu = pytest.mark.gpu


def _lib():
    from clip_event_amd._lib import lib, ptr, stream
    return lib(), ptr, stream


def _gen(seed):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return g


def _bits(t):
    return t.view(torch.int16) if t.element_size() == 2 else t.view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a.contiguous()), _bits(b.contiguous()))


def _within(got, want, bound, name):
    """Element-wise |got - want| <= bound (fp64; NaN fails)."""
    err = (got.double() - want).abs()
    ok = bool((err <= bound).all())
    worst = float((err / bound.clamp_min(1e-300)).nan_to_num(float("inf")).max())
    print(f"[{name}] worst |err| / bound {worst:.3f}")
    assert ok, f"{name}: {int((~(err <= bound)).sum())} elements over the bound (worst ratio {worst:.3g})"


# ---------------------------------------------------------------------------------------------------------------
# embed.hip

@gpu
@pytest.mark.parametrize("ps,R,kp", [(32, 224, 3072), (16, 224, 768), (16, 224, 832), (14, 224, 592), (14, 224, 640),
                                     (8, 64, 192), (8, 64, 256)])
def test_im2col_bit_exact_with_zero_padding(ps, R, kp):
    """``ce_im2col`` = torch unfold + bf16 cast bit for bit, columns (c, py, px), rows (b, gy, gx); columns >= 3 p^2 are
    zero.  The images are a view of a buffer with one more (guard) image of finite sentinel pixels behind them: a kernel that
    reads a "fourth channel" for the padded columns picks up the guard instead of zeros, and never leaves the allocation.
    p = 8 / 16 / 32 take the 16-byte path, p = 14 the per-element one; kp = 3 p^2 (p = 14: the smallest multiple of 8) and
    padded (832, 640, 256).  A kp that is not a multiple of 8 is refused."""
    cl, ptr, stream = _lib()
    B, g = 3, R // ps
    buf = torch.full((B + 1, 3, R, R), 1234.5, device=DEV)
    buf[:B] = torch.randn(B, 3, R, R, generator=_gen(ps * 1000 + kp), device=DEV)
    img = buf[:B]
    rows = B * g * g
    out = torch.full((rows + 2, kp), -7.0, device=DEV, dtype=torch.bfloat16)
    rc = cl.ce_im2col(ptr(img), ptr(out), c_int(B), c_int(R), c_int(ps), c_int(kp), stream())
    torch.cuda.synchronize()
    assert rc == 0, cl.ce_last_error()
    ref = img.unfold(2, ps, ps).unfold(3, ps, ps).permute(0, 2, 3, 1, 4, 5).reshape(rows, 3 * ps * ps)
    want = torch.zeros(rows, kp, device=DEV, dtype=torch.bfloat16)
    want[:, :3 * ps * ps] = ref.to(torch.bfloat16)
    padded = out[:rows, 3 * ps * ps:]
    print(f"[im2col p={ps} kp={kp}] nonzero padded elements: {int((padded != 0).sum())} of {padded.numel()}")
    assert _same_bits(out[:rows], want)
    assert bool((out[rows:] == -7.0).all())
    if (3 * ps * ps) % 8:
        assert cl.ce_im2col(ptr(img), ptr(out), c_int(B), c_int(R), c_int(ps), c_int(3 * ps * ps), stream()) != 0


@gpu
@pytest.mark.parametrize("B,T,D", [(3, 50, 768), (2, 197, 68), (1, 2, 4)])
def test_vision_assemble_and_backward_bit_exact(B, T, D):
    """``ce_vision_assemble``: x0[b, t] = (t == 0 ? cls : patch[b, t - 1]) + pos[t] -- one fp32 add, so equal to torch's bit
    for bit; ``ce_vision_assemble_bwd``: the patch rows of dx0 rounded to bf16.  Guard rows untouched."""
    cl, ptr, stream = _lib()
    gen = _gen(B * T + D)
    patch = torch.randn(B * (T - 1), D, generator=gen, device=DEV)
    cls, pos = torch.randn(D, generator=gen, device=DEV), torch.randn(T, D, generator=gen, device=DEV)
    x0 = torch.full((B * T + 1, D), 3.5, device=DEV)
    assert cl.ce_vision_assemble(ptr(patch), ptr(cls), ptr(pos), ptr(x0), c_int(B), c_int(T), c_int(D), stream()) == 0
    dx0 = torch.randn(B * T, D, generator=gen, device=DEV)
    dpatch = torch.full((B * (T - 1) + 1, D), 3.5, device=DEV, dtype=torch.bfloat16)
    assert cl.ce_vision_assemble_bwd(ptr(dx0), ptr(dpatch), c_int(B), c_int(T), c_int(D), stream()) == 0
    torch.cuda.synchronize()
    want = torch.cat([cls.expand(B, 1, D), patch.view(B, T - 1, D)], 1) + pos
    assert _same_bits(x0[:B * T], want.reshape(B * T, D)) and bool((x0[B * T:] == 3.5).all())
    assert _same_bits(dpatch[:-1], dx0.view(B, T, D)[:, 1:].reshape(-1, D).to(torch.bfloat16))
    assert bool((dpatch[-1] == 3.5).all())


def _packed_rows(lens, T):
    return torch.cat([b * T + torch.arange(n) for b, n in enumerate(lens)]).to(torch.int32)


@gpu
@pytest.mark.parametrize("D", [512, 36])
def test_token_embed_bwd_against_fp64(D):
    """``ce_token_embed_bwd`` on a packed batch (src_rows = the live tokens): dtable[id] += dx0[row] against an fp64
    index_add_ into a non-zero table.  Ids repeat (a few ids carry up to ~40 rows), some appear once, the padding id 0 carries
    rows of exact zeros (skipped by the kernel) beside non-zero rows.  Bound per element: one fp32 rounding per atomic add,
    (count + 1) 2^-24 (|start| + sum |dx0|); ids with one contributor are exactly fp32(start + dx0); rel-L2 < 1e-6."""
    cl, ptr, stream = _lib()
    rng = np.random.default_rng(D)
    n, T, V = 8, 20, 300
    lens = [20, 1, 7, 13, 20, 3, 11, 16]
    ids = torch.from_numpy(rng.integers(1, 12, size=(n, T))).long()           # many repeats
    ids[:, 15:] = 0                                                            # padding id
    ids[2, :4] = torch.tensor([200, 201, 202, 203])                            # ids with a single contributor
    src = _packed_rows(lens, T)
    flat_ids = ids.flatten()[src.long()]
    rows = src.numel()
    dx0 = torch.from_numpy(rng.standard_normal((rows, D)).astype(np.float32))
    dx0[flat_ids == 0] = 0.0
    pad_rows = (flat_ids == 0).nonzero().flatten()
    dx0[pad_rows[::2]] = torch.from_numpy(rng.standard_normal((len(pad_rows[::2]), D)).astype(np.float32))   # half the padding rows live
    dx0[5, : D // 2] = 0.0                                                     # exact zeros inside a live row
    start = torch.from_numpy(rng.standard_normal((V, D)).astype(np.float32))
    dtable = torch.cat([start, torch.full((1, D), 9.0)]).to(DEV)              # + guard row
    ids_d, src_d, dx_d = ids.to(DEV), src.to(DEV), dx0.to(DEV)
    rc = cl.ce_token_embed_bwd(ptr(ids_d), ptr(src_d), ptr(dx_d), ptr(dtable), c_long(rows), c_int(D), c_int(V), stream())
    torch.cuda.synchronize()
    assert rc == 0, cl.ce_last_error()
    got = dtable[:V].cpu()
    want = start.double().index_add(0, flat_ids, dx0.double())
    mag = start.double().abs().index_add(0, flat_ids, dx0.double().abs())
    cnt = torch.bincount(flat_ids, minlength=V).double()[:, None]
    _within(got, want, (cnt + 1) * U * mag, f"token_embed_bwd D={D}")
    assert float((got.double() - want).norm() / want.norm()) < 1e-6
    once = cnt[:, 0] == 1
    single = start.clone().index_add(0, flat_ids, dx0)                          # one fp32 add per element for these ids
    assert torch.equal(got[once], single[once]) and int(once.sum()) >= 4
    assert bool((dtable[V:] == 9.0).all())


@gpu
@pytest.mark.parametrize("n", [1, 7, 37])
@pytest.mark.parametrize("D", [68, 512, 4096])
def test_pos_embed_bwd_packed_against_fp64(n, D):
    """``ce_pos_embed_bwd_packed``: dpos[t] += sum over the samples longer than t of dx0[cu[b] + t], into a non-zero dpos,
    for n below / at / above the 8-way sample split, lengths 1..T (1 and T included), D = 68 (17 lanes of 4), 512, 4096.
    Bound per element: (n + 2) 2^-24 (|start| + sum |dx0|) (fp32 partial sums + one atomic per split); rel-L2 < 1e-6; the
    guard row after dpos untouched."""
    cl, ptr, stream = _lib()
    rng = np.random.default_rng(n * 10000 + D)
    T = 77
    lens = rng.integers(1, T + 1, size=n)
    lens[0] = T
    if n > 1:
        lens[1] = 1
    cu = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)]).astype(np.int32))
    R = int(cu[-1])
    dx0 = torch.from_numpy(rng.standard_normal((R, D)).astype(np.float32))
    start = torch.from_numpy(rng.standard_normal((T, D)).astype(np.float32))
    dpos = torch.cat([start, torch.full((1, D), 5.0)]).to(DEV)
    dx_d, cu_d = dx0.to(DEV), cu.to(DEV)
    rc = cl.ce_pos_embed_bwd_packed(ptr(dx_d), ptr(cu_d), ptr(dpos), c_int(n), c_int(T), c_int(D), stream())
    torch.cuda.synchronize()
    assert rc == 0, cl.ce_last_error()
    t_of_row = torch.cat([torch.arange(int(l)) for l in lens])
    want = start.double().index_add(0, t_of_row, dx0.double())
    mag = start.double().abs().index_add(0, t_of_row, dx0.double().abs())
    got = dpos[:T].cpu()
    _within(got, want, (n + 2) * U * mag, f"pos_embed_bwd_packed n={n} D={D}")
    assert float((got.double() - want).norm() / want.norm()) < 1e-6
    assert bool((dpos[T:] == 5.0).all())


@gpu
@pytest.mark.parametrize("B", [1, 3, 5, 256])
@pytest.mark.parametrize("part", ["all", "class_row"])
@pytest.mark.parametrize("accumulate", [0, 1])
def test_batch_reduce_against_fp64(B, part, accumulate):
    """``ce_batch_reduce``: out[i] (+)= sum_b x[b * slab + i] for i < n, over whole slabs (positional-embedding gradient,
    n = slab) and over the first row of each slab only (class embedding, n = D < slab); accumulate 0 overwrites a
    NaN-poisoned out, 1 adds into a non-zero one.  Bound: (B + 2) 2^-24 (|start| + sum |x|); elements past n untouched."""
    cl, ptr, stream = _lib()
    T, D = 50, 768
    slab = T * D
    n = slab if part == "all" else D
    gen = _gen(B * 10 + accumulate)
    x = torch.randn(B, slab, generator=gen, device=DEV)
    start = torch.randn(n, generator=gen, device=DEV)
    out = torch.full((n + 16,), 6.0, device=DEV)
    out[:n] = start if accumulate else float("nan")
    rc = cl.ce_batch_reduce(ptr(x), ptr(out), c_int(B), c_long(slab), c_long(n), c_int(accumulate), stream())
    torch.cuda.synchronize()
    assert rc == 0, cl.ce_last_error()
    xs = x[:, :n].double()
    want = xs.sum(0) + (start.double() if accumulate else 0)
    mag = xs.abs().sum(0) + (start.double().abs() if accumulate else 0)
    _within(out[:n], want, (B + 2) * U * mag, f"batch_reduce B={B} {part} acc={accumulate}")
    assert bool((out[n:] == 6.0).all())


@gpu
@pytest.mark.parametrize("M", [1, 63, 65, 12800])
@pytest.mark.parametrize("N", [8, 264, 3072])
def test_colsum_bf16_against_fp64(M, N):
    """``ce_colsum_bf16``: out[n] += sum_m x[m, n] over a bf16 matrix with ld > N, into a non-zero out.  The kernel sums 8
    rows per lane, 8 lanes per 64-row block and one float atomic per block: at most 16 + ceil(M / 64) roundings on the way,
    so the bound is (16 + ceil(M / 64) + 1) 2^-24 (|start| + sum |x|); a dropped or doubled row block is off by ~8 / M of that
    magnitude or more.  Elements past N untouched."""
    cl, ptr, stream = _lib()
    gen = _gen(M + N)
    ld = N + 16
    x = torch.randn(M, ld, generator=gen, device=DEV).to(torch.bfloat16)
    start = torch.randn(N, generator=gen, device=DEV) * math.sqrt(M)
    out = torch.full((N + 8,), 2.5, device=DEV)
    out[:N] = start
    rc = cl.ce_colsum_bf16(ptr(x), c_long(ld), ptr(out), c_int(M), c_int(N), stream())
    torch.cuda.synchronize()
    assert rc == 0, cl.ce_last_error()
    xs = x[:, :N].double()
    want = start.double() + xs.sum(0)
    mag = start.double().abs() + xs.abs().sum(0)
    _within(out[:N], want, (17 + (M + 63) // 64) * U * mag, f"colsum M={M} N={N}")
    assert bool((out[N:] == 2.5).all())


@gpu
@pytest.mark.parametrize("rows,cols,lds,ldd", [(768, 588, 640, 588), (5, 3, 8, 7), (1, 1000, 1024, 1003)])
def test_add_cols_bit_exact(rows, cols, lds, ldd):
    """``ce_add_cols``: dst[r, c] += src[r, c] for c < cols (the padded conv1 weight gradient folded into the real one):
    one fp32 add, bit-equal to torch; dst columns >= cols and the guard row untouched."""
    cl, ptr, stream = _lib()
    gen = _gen(rows + cols)
    src = torch.randn(rows, lds, generator=gen, device=DEV)
    dst = torch.randn(rows + 1, ldd, generator=gen, device=DEV)
    before = dst.clone()
    assert cl.ce_add_cols(ptr(src), c_long(lds), ptr(dst), c_long(ldd), c_int(rows), c_int(cols), stream()) == 0
    torch.cuda.synchronize()
    want = before.clone()
    want[:rows, :cols] += src[:, :cols]
    assert _same_bits(dst, want)


@gpu
@pytest.mark.parametrize("R,C", [(100, 37), (768, 588), (33, 1000), (1, 5), (64, 64)])
def test_cast_transpose_bit_exact(R, C):
    """``ce_cast_transpose``: the bf16 copy [R, C] (ld16 > C) and the bf16 transposed copy [C, R] (ld16t > R) of an fp32
    matrix, R and C not multiples of the 32 x 32 tile; each output requested alone and both together; RNE casts bit-equal to
    torch's; columns past the row and the guard rows untouched."""
    cl, ptr, stream = _lib()
    w = torch.randn(R, C, generator=_gen(R * C), device=DEV)
    ld16, ld16t = C + 8, R + 24
    for want16, want16t in ((True, False), (False, True), (True, True)):
        w16 = torch.full((R + 1, ld16), -2.0, device=DEV, dtype=torch.bfloat16)
        w16t = torch.full((C + 1, ld16t), -2.0, device=DEV, dtype=torch.bfloat16)
        rc = cl.ce_cast_transpose(ptr(w), ptr(w16) if want16 else c_void_p(0), c_long(ld16), ptr(w16t) if want16t else c_void_p(0),
                                  c_long(ld16t), c_int(R), c_int(C), stream())
        torch.cuda.synchronize()
        assert rc == 0, cl.ce_last_error()
        e16 = torch.full_like(w16, -2.0)
        e16t = torch.full_like(w16t, -2.0)
        if want16:
            e16[:R, :C] = w.to(torch.bfloat16)
        if want16t:
            e16t[:C, :R] = w.t().to(torch.bfloat16)
        assert _same_bits(w16, e16) and _same_bits(w16t, e16t), (want16, want16t)


@gpu
@pytest.mark.parametrize("mode", ["gather", "scatter", "both"])
def test_copy_rows_bit_exact(mode):
    """``ce_copy_rows``: dst[dst_rows[i] or i] = src[src_rows[i] or i] in 16-byte granules with different row strides
    (a row of 128 bytes out of 160-byte source rows into 192-byte destination rows); every byte not named stays."""
    cl, ptr, stream = _lib()
    rng = np.random.default_rng(len(mode))
    src = torch.randn(50, 40, generator=_gen(len(mode)), device=DEV)           # 160-byte rows
    dst = torch.full((60, 48), 8.25, device=DEV)                                # 192-byte rows
    n, row_bytes = 20, 128
    srows = torch.from_numpy(rng.permutation(50)[:n].astype(np.int32)) if mode != "scatter" else None
    drows = torch.from_numpy(rng.permutation(60)[:n].astype(np.int32)) if mode != "gather" else None
    sr_d = srows.to(DEV) if srows is not None else None
    dr_d = drows.to(DEV) if drows is not None else None
    rc = cl.ce_copy_rows(ptr(src), c_long(160), ptr(sr_d), ptr(dst), c_long(192), ptr(dr_d), c_int(n), c_int(row_bytes), stream())
    torch.cuda.synchronize()
    assert rc == 0, cl.ce_last_error()
    want = torch.full((60, 48), 8.25, device=DEV)
    s_idx = srows.long() if srows is not None else torch.arange(n)
    d_idx = drows.long() if drows is not None else torch.arange(n)
    want[d_idx.to(DEV), :32] = src[s_idx.to(DEV), :32]
    assert _same_bits(dst, want)


# ---------------------------------------------------------------------------------------------------------------
# optim.hip: clip + Adam

@gpu
@pytest.mark.parametrize("n", [4097, 4099, 2048 * 1024 + 4097, 2048 * 1024 + 4099])
def test_sumsq_exact_on_exactly_summable_data(n):
    """``ce_sumsq`` adds sum g^2 into *out.  Entries in {0, +-1/4, +-1/2}: every square and every partial sum is a multiple of
    1/16 below 2^20, exact in fp32 whatever the order, so the result must EQUAL the fp64 sum plus the non-zero start -- a
    dropped, doubled or out-of-range element shows.  n = 4k+1, 4k+3 (the scalar tail), and past 2048 blocks x 1024 (the
    grid-stride loop runs twice)."""
    cl, ptr, stream = _lib()
    g = (torch.randint(-2, 3, (n,), generator=_gen(n), device=DEV).float() / 4)
    g[-1] = 0.5                                                              # the tail counts
    out = torch.tensor([1.5, 7.0], device=DEV)
    assert cl.ce_sumsq(ptr(g), c_long(n), ptr(out), stream()) == 0
    torch.cuda.synchronize()
    want = 1.5 + float((g.double() ** 2).sum())
    assert float(out[0]) == want and float(out[1]) == 7.0, (float(out[0]), want)


@gpu
@pytest.mark.parametrize("n", [4097, 4099, 2048 * 1024 + 4099])
def test_sumsq_against_fp64(n):
    """The same on normal data: positive terms, so each fp32 rounding is at most 2^-24 of the running total; the rounding
    chain is 4 per lane-load, 6 in the wave sum, 2 across waves and one atomic per block (at most 2048):
    rel error <= (blocks + 16) 2^-24 of the total."""
    cl, ptr, stream = _lib()
    g = torch.randn(n, generator=_gen(n + 1), device=DEV)
    out = torch.tensor([3.0], device=DEV)
    assert cl.ce_sumsq(ptr(g), c_long(n), ptr(out), stream()) == 0
    torch.cuda.synchronize()
    want = 3.0 + float((g.double() ** 2).sum())
    blocks = min(2048, (n + 1023) // 1024)
    rel = abs(float(out[0]) - want) / want
    print(f"[sumsq n={n}] rel {rel:.2e} (bound {(blocks + 16) * U:.2e})")
    assert rel <= (blocks + 16) * U


# Adam hyper-parameters as the kernel receives them (fp32); the references use the same fp32-rounded values
B1, B2, EPS, LR, MAX_NORM = (float(np.float32(x)) for x in (0.9, 0.999, 1e-8, 1e-3, 1.0))


def adam_ref(p, g, m, v, sumsq, wd, step):
    """fp64 restatement of optim.hip's adam_elem: clip coefficient min(1, max_norm / (sqrt(sumsq) + 1e-6)) (1 without
    sumsq), L2 weight decay into the gradient, moments, bias corrections, update.  Returns (p, m, v, m_mag, v_mag, denom,
    lr_bc1): m_mag = |b1 m| + (1 - b1) |g_eff| and v_mag bound the size of the terms that make up the new m and v."""
    p, g, m, v = (t.double() for t in (p, g, m, v))
    coef = 1.0 if sumsq is None else min(1.0, MAX_NORM / (math.sqrt(sumsq) + 1e-6))
    ge = g * coef + wd * p
    gmag = (g * coef).abs() + wd * p.abs()
    m_mag = B1 * m.abs() + (1 - B1) * gmag
    v_mag = B2 * v + (1 - B2) * gmag * gmag
    m = B1 * m + (1 - B1) * ge
    v = B2 * v + (1 - B2) * ge * ge
    lr_bc1 = LR / (1 - B1 ** step)
    denom = v.sqrt() / math.sqrt(1 - B2 ** step) + EPS
    return p - lr_bc1 * m / denom, m, v, m_mag, v_mag, denom, lr_bc1


def _adam_bounds(ref):
    """Element bounds on (p, m, v) of the fp32 kernel against adam_ref: m and v are about seven fp32 roundings (clip
    coefficient, scaling, decay, moment update) of terms of size m_mag / v_mag: 2^-20 of those (16 ulp); p within 2 ulp of p
    plus 2^-19 of lr_bc1 m_mag / denom (the update's own relative error -- m's, sqrt(v)'s, two divisions, the bias
    corrections rounded to fp32 -- stays near 2^-20).  A clip coefficient that is wrong, unclamped or inverted moves m by a
    factor, at step 1 by exactly the factor."""
    p, m, v, m_mag, v_mag, denom, lr_bc1 = ref
    return (2 * U * p.abs() + 2.0 ** -19 * lr_bc1 * m_mag / denom, 2.0 ** -20 * m_mag, 2.0 ** -20 * v_mag)


def _adam_state(n, step, clip, seed):
    """(p, g, m, v, sumsq or None): g scaled to total norm 10 (clip active / none) or 0.5 (inactive) x max_norm; zero moments
    at step 1 (where m = (1 - b1)(coef g + wd p) shows the coefficient directly), earlier-step-like moments otherwise."""
    gen = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=gen) * 0.02
    g = torch.randn(n, generator=gen)
    g *= (0.5 if clip == "inactive" else 10.0) * MAX_NORM / float(g.double().norm())
    if step == 1:
        m, v = torch.zeros(n), torch.zeros(n)
    else:
        m = torch.randn(n, generator=gen) * 1e-3
        v = (torch.randn(n, generator=gen) * 1e-3) ** 2 + 1e-8
    sumsq = None if clip == "none" else float(np.float32((g.double() ** 2).sum()))
    return p, g, m, v, sumsq


ADAM_GRID = [(clip, wd, step) for clip in ("active", "inactive", "none") for wd in (0.0, 0.1) for step in (1, 2, 1000)]


def test_adam_reference_matches_torch():
    """CPU cross-check of the fp64 restatement: torch.nn.utils.clip_grad_norm_ + torch.optim.Adam(foreach=False) on fp32
    copies land within the kernel's bounds (x4: torch's lerp form of the first moment rounds differently)."""
    for clip, wd, step in ADAM_GRID:
        p0, g0, m0, v0, sumsq = _adam_state(999, step, clip, 5)
        param = torch.nn.Parameter(p0.clone())
        param.grad = g0.clone()
        if sumsq is not None:
            torch.nn.utils.clip_grad_norm_([param], MAX_NORM)
        opt = torch.optim.Adam([param], lr=LR, betas=(B1, B2), eps=EPS, weight_decay=wd, foreach=False)
        opt.state[param] = {"step": torch.tensor(float(step - 1)), "exp_avg": m0.clone(), "exp_avg_sq": v0.clone()}
        opt.step()
        ref = adam_ref(p0, g0, m0, v0, sumsq, wd, step)
        bp, bm, bv = _adam_bounds(ref)
        st = opt.state[param]
        for name, got, want, bound in (("p", param.detach(), ref[0], bp), ("m", st["exp_avg"], ref[1], bm), ("v", st["exp_avg_sq"], ref[2], bv)):
            err = (got.double() - want).abs()
            assert bool((err <= 4 * bound).all()), (clip, wd, step, name, float((err / bound).max()))


def _check_adam(tag, ref, p, m, v):
    bp, bm, bv = _adam_bounds(ref)
    _within(m.cpu(), ref[1], bm, f"{tag} exp_avg")
    _within(v.cpu(), ref[2], bv, f"{tag} exp_avg_sq")
    _within(p.cpu(), ref[0], bp, f"{tag} master")


def _dev(*ts):
    return [t.to(DEV) for t in ts]


@gpu
@pytest.mark.parametrize("n", [7171, 5, 1000003])
def test_adam_step_against_fp64(n):
    """``ce_adam_step`` (flat) for the clip active (norm 10 x max_norm), inactive, and off (sumsq NULL), weight decay 0 / 0.1,
    steps 1 / 2 / 1000, n with n % 4 != 0 and n % 2048 != 0: exp_avg, exp_avg_sq and the masters element-wise against the
    fp64 restatement (_adam_bounds); the bf16 mirror bit-equal to the masters' RNE cast; guard elements untouched."""
    cl, ptr, stream = _lib()
    for clip, wd, step in ADAM_GRID:
        p0, g0, m0, v0, sumsq = _adam_state(n, step, clip, n + step)
        ref = adam_ref(p0, g0, m0, v0, sumsq, wd, step)
        bufs = [torch.cat([t, torch.full((6,), 4.0)]).to(DEV) for t in (p0, g0, m0, v0)]
        p, g, m, v = bufs
        p16 = torch.full((n + 6,), 4.0, device=DEV, dtype=torch.bfloat16)
        ss = torch.tensor([sumsq if sumsq is not None else 0.0], device=DEV)
        rc = cl.ce_adam_step(ptr(p), ptr(g), ptr(m), ptr(v), ptr(p16), c_long(n), ptr(ss) if sumsq is not None else c_void_p(0),
                             c_float(MAX_NORM), c_float(LR), c_float(B1), c_float(B2), c_float(EPS), c_float(wd), c_int(step), stream())
        torch.cuda.synchronize()
        assert rc == 0, cl.ce_last_error()
        tag = f"adam n={n} clip={clip} wd={wd} step={step}"
        _check_adam(tag, ref, p[:n], m[:n], v[:n])
        assert _same_bits(p16[:n], p[:n].to(torch.bfloat16))
        for t in (p, g, m, v):
            assert bool((t[n:] == 4.0).all())
        assert bool((p16[n:] == 4.0).all())


# flat layout of the tiled form: matrices (offset, rows, cols) and [lo, hi) segments covering everything else, lengths 4..2048
# and multiples of 4; the last 8 elements belong to nothing and must stay untouched
TILE_MATS = [(4, 72, 200), (16500, 8, 8), (17000, 136, 64)]
TILE_SEGS = [(0, 4), (14404, 16452), (16452, 16500), (16564, 17000), (25704, 25708)]
TILE_N = 25708


@gpu
def test_adam_step_tiles_against_fp64():
    """``ce_adam_step_tiles``: the same update over a table of bf16-mirrored matrices (72 x 200: ragged 64 x 64 tiles on both
    axes; 8 x 8; 136 x 64) plus segments (lengths 4 to 2048) covering the rest of the flat buffers, for the grid of
    ``test_adam_step_against_fp64``; the mirror bit-equal to the masters' cast, every W^T copy bit-equal to the mirror's
    transpose, the 8 elements outside every matrix and segment untouched in p / m / v / mirror."""
    from clip_event_amd._lib import TransposeJob
    cl, ptr, stream = _lib()
    covered = sorted([(o, o + r * c) for o, r, c in TILE_MATS] + TILE_SEGS)
    assert covered[0][0] == 0 and all(a[1] == b[0] for a, b in zip(covered, covered[1:])) and covered[-1][1] == TILE_N
    n = TILE_N + 8
    seg_tab = torch.tensor(TILE_SEGS, dtype=torch.int64).to(DEV)
    for clip, wd, step in ADAM_GRID:
        p0, g0, m0, v0, sumsq = _adam_state(n, step, clip, 77 + step)
        ref = adam_ref(p0, g0, m0, v0, sumsq, wd, step)
        p, g, m, v = _dev(p0, g0, m0, v0)
        p16 = torch.full((n,), 4.0, device=DEV, dtype=torch.bfloat16)
        wts = [torch.full((c, r), -4.0, device=DEV, dtype=torch.bfloat16) for _, r, c in TILE_MATS]
        jobs, tiles = (TransposeJob * len(TILE_MATS))(), 0
        for i, ((off, r, c), wt) in enumerate(zip(TILE_MATS, wts)):
            jobs[i].src, jobs[i].dst = p16.data_ptr() + 2 * off, wt.data_ptr()
            jobs[i].rows, jobs[i].cols, jobs[i].tile_start = r, c, tiles
            tiles += ((r + 63) // 64) * ((c + 63) // 64)
        tab = torch.frombuffer(bytearray(bytes(jobs)), dtype=torch.uint8).to(DEV)
        ss = torch.tensor([sumsq if sumsq is not None else 0.0], device=DEV)
        rc = cl.ce_adam_step_tiles(ptr(p), ptr(g), ptr(m), ptr(v), ptr(p16), ptr(tab), c_int(len(TILE_MATS)), c_int(tiles), ptr(seg_tab),
                                   c_int(len(TILE_SEGS)), ptr(ss) if sumsq is not None else c_void_p(0), c_float(MAX_NORM), c_float(LR),
                                   c_float(B1), c_float(B2), c_float(EPS), c_float(wd), c_int(step), stream())
        torch.cuda.synchronize()
        assert rc == 0, cl.ce_last_error()
        tag = f"adam tiles clip={clip} wd={wd} step={step}"
        N = TILE_N
        _check_adam(tag, tuple(t[:N] if torch.is_tensor(t) else t for t in ref), p[:N], m[:N], v[:N])
        assert _same_bits(p16[:N], p[:N].to(torch.bfloat16))
        for t, t0 in ((p, p0), (m, m0), (v, v0)):
            assert torch.equal(t[N:].cpu(), t0[N:])
        assert bool((p16[N:] == 4.0).all())
        for (off, r, c), wt in zip(TILE_MATS, wts):
            assert _same_bits(wt, p16[off:off + r * c].view(r, c).t()), (r, c)


@gpu
def test_zero_segments_touches_only_its_chunks():
    """``ce_zero_segments``: zero [lo, hi) for every chunk of the table -- chunks at both ends of the buffer, one of 4
    elements, one longer than a workgroup's 1024-element sweep -- and nothing else (bit-exact)."""
    cl, ptr, stream = _lib()
    N = 20000
    base = torch.randn(N, generator=_gen(11), device=DEV)
    before = base.clone()
    chunks = [(0, 64), (1000, 1004), (2000, 7000), (N - 128, N)]
    tab = torch.tensor(chunks, dtype=torch.int64).to(DEV)
    assert cl.ce_zero_segments(ptr(base), ptr(tab), c_int(len(chunks)), stream()) == 0
    torch.cuda.synchronize()
    want = before.clone()
    for lo, hi in chunks:
        want[lo:hi] = 0.0
    assert _same_bits(base, want)
