"""The LayerNorm family (``ce_layernorm_fwd`` / ``_fwd_t`` / ``_fwd_q8`` / ``_bwd`` / ``_bwd_t`` / ``_bwd_q8`` / ``_bwd_partials`` /
``_fold``: csrc/layernorm.hip) against an fp64 reference of the same operand bits: the element-wise checker, the guarded and
poisoned layouts, the case table and the runner, shared by tests/test_layernorm_ops.py and the child process it starts per
environment form (tests/ln_child.py).  Pure torch; importable without a GPU.

Everything below is fp64, computed from the bits the kernel is given -- the fp16 / bf16 operands as stored (fp16 gradient
operands divided by the power-of-two scale, which is exact), eps as the fp32 number passed, and for the backward the fp32
``mean`` / ``rstd`` arrays it receives.  None of the bounds is fitted to the kernels.

Constants:  u = 2^-24.  gamma_D = min(D, 128) u: any summation of the D row terms whose longest chain of additions is at most
128 (a wave per row up to D = 2048: 8 chunk sums of 4 per lane, a 64-lane tree; any blocked variant).  Per row: A = mean |x|,
A_d = mean |x - mu|, Q = mean (x - mu)^2.

Forward (mu, Q, rstd = (Q + eps)^-1/2, xhat = (x - mu) rstd, y = xhat g + b):
    d_mu     = gamma_D A + u |mu|
    d_Q      = 2 A_d d_mu + d_mu^2 + (gamma_D + 4u) Q
    rho      = d_Q / (2 (Q + eps)) + 4u                        relative error of rstd
    d_xhat_j = rstd d_mu + |xhat_j| (rho + 3u)
    B_y,j    = |g_j| d_xhat_j + 2u (|xhat_j g_j| + |y_j|)
  checks:  mean  |got - mu| <= d_mu;   rstd  |got - rstd| <= rho rstd;   fp32 y  |got - y| <= B_y;
           bf16 / fp16 y  the monotone interval RNE(y - B) <= got <= RNE(y + B) (fp16: ends clamped to +-65504; check_rounded of
           tests/nt_cases.py);   e4m3 copy  bytes and scales bit-equal to the torch restatement of ce_quant_rows_fp8 (q8_ref
           below = _q8_ref of tests/test_hip_ops.py) applied to the bf16 output actually stored -- not to the quantisation kernel.

Backward (gy = dy g, xhat = (x - mean) rstd, c1 = mean gy, c2 = mean gy xhat, t = gy - c1 - xhat c2, dx = t rstd + dx_in):
    d_xhat = 3u |xhat|        d_gy = u |gy|        d_c1 = (gamma_D + 2u) mean |gy|        d_c2 = (gamma_D + 6u) mean |gy xhat|
    d_t    = d_gy + d_c1 + |xhat| d_c2 + |c2| d_xhat + 3u (|gy| + |c1| + |xhat c2|)
    B_dx   = rstd d_t + 2u (|t rstd| + |dx|)
  checks:  fp32 dx_out  |got - dx| <= B_dx;   fp16 dx_out  the interval on dx gscale with B_dx gscale and the +-65504 clamp;
           dxb  bit-equal to RNE-bf16 of the fp32 dx_out stored, where dx_out is fp32; the bf16 interval on dx otherwise;
           e4m3 copy  q8_ref of the dxb actually stored.
  Column sums (dgamma: term dy xhat, d_term 4u |dy xhat| = |dy| d_xhat + one product rounding; dbeta: term dy, d_term 0;
  dxsum: term dx, d_term B_dx), summed over rows in any order, atomics included, always as got - base with a non-zero base:
           |(got - base) - sum_r term| <= C (sum_r |term| + |base|) + sum_r d_term,   C = max(2^-12, M u).
  2^-12 is the TN suite's constant (tests/wgrad_cases.py), valid for M <= 4096 rows; the one longer table row (M = 8197, the
  NW = 16 loop case) takes M u = 2^-11.0, the worst case of an fp32 sum of M terms in any order.
  The partials form: sum_b partials[b] over the ``blocks`` rows against the same reference and bound (base 0), every element of
  partials[0 : blocks][0 : P] written (pre-filled with NaN; P = 2 without dxsum, whose third [D] must then stay NaN: the fold
  does not read it), sentinel guard rows behind; then ce_layernorm_fold adds it into the non-zero bases and dgamma / dbeta /
  dxsum follow the bound above.  A job with a null dxsum leaves its dxsum bit-identical.

On top of every check the relative-L2 limits of the older tests (tests/test_hip_ops.py): 2e-6 fp32 forward, 3e-3 bf16, 1e-5 dx /
dgamma / dbeta, 1e-4 dxsum (fp16 outputs: 4e-4, the NT suite's figure for RNE to 11 bits).  They are flat, with one exception
(fwd_rel_limit below, used by the runner and by the checker's own tests alike).  The 2e-6 of the fp32 forward was stated for rows
of the `plain` class, whose condition number kappa = A / sqrt(Q + eps) of the mean subtraction is 1.1.  The error of an fp32 mean,
some u A, reaches xhat multiplied by rstd, that is as some u kappa of xhat's size: a faithful fp32 two-pass forward on the `offset`
rows (kappa = 600) errs by 3e-5 in lane order and by 2e-4 .. 4e-4 in serial order, above 2e-6 whatever the implementation, so the
emulations fail the flat figure there (and the fp16 output, 4.2e-4 at D = 2048, its 4e-4).  For fp32 and fp16 outputs the limit is
therefore REL_FWD + 2e-6 max(0, kappa / KAPPA_PLAIN - 1): the fp32 figure again for every factor KAPPA_PLAIN = 2 by which the
worst row exceeds the class the figure was stated for; kappa is the largest over the rows with Q > 0 -- the all-zero and the
constant edge rows have rstd = eps^-1/2 but carry no error of the mean (their sums, of D times 0, 3 or 30, are exact in fp32).
That is 6e-4 on `offset` and nothing on `plain` and `mixed` (kappa 0.8 .. 0.9; at D = 4 one four-element row of small spread
reaches 3.7, which makes 3.6e-6); bf16 outputs keep the flat 3e-3 everywhere.  The
per-element bounds are what holds the `offset` rows tightly.  The backward limits are flat: the backward takes mean / rstd as given.

Values (seeded):  plain 2 randn + 0.5;  offset 0.05 randn + 30;  mixed per-row scales e^(3 randn) on x (the exponent clamped to
[-4, 8] so that fp16 operands stay finite) and e^randn on dy.  Edge rows inside every case with enough rows: row 1 all zero, row
2 constant (variance 0, rstd = eps^-1/2), row 3 with a constant dy; eight all-zero dy columns (8 .. 16) leave dgamma / dbeta at
their base bit for bit.  special "limit": one fp16 x element at exactly 65504 (forward counter [0] >= 1 exactly there);  "sat":
one dy row times 2^14, so that dx gscale passes 65504 and the interval check demands the clamp (backward counter [1] >= 1
exactly there, 0 in every other backward launch).

Layouts.  Every matrix has 3 guard rows; mean, rstd, qscale 3 guard elements; w, b, dgamma, dbeta, dxsum 8 floats behind them.
Outputs: everything outside the [M, D] block (rows not named by `rows` included) holds a finite sentinel that must come back
bit-identical; the block of an overwritten output starts as NaN.  Inputs: NaN everywhere outside the operand but inside the
allocation (w[D : D + 8), b[D : D + 8), the columns beside a slice, rows >= M, rows not named by `rows`).
    dense    every ld = D
    wide     every matrix the column slice from column 4 of a buffer with ld = D + 12 (q8: ldq = D + 12; dxb too)
    rows     wide, gather / scatter through a permuted, non-contiguous `rows` without duplicates into 2M + 3 stream rows, and
             lddxb = D + 20 (differs from lddx).  Forward: x gathered, y / q8 / mean / rstd indexed by r.  Backward: x, dx_in,
             dx_out, dxb, q8, qscale indexed by rows[r]; dy, mean, rstd by r.
    inplace  backward, dense, dx_in and dx_out the same buffer; the reference is computed from the values before the launch
    nodxb    backward, dense, dxb = NULL with lddxb = lddx (where a bf16 copy would land inside dx_out): dx_out must pass its
             check and equal the dense launch's dx_out bit for bit
    noin     backward, dense, dx_in = NULL"""
import math
import os
from ctypes import Structure, c_float, c_int, c_long, c_void_p

import torch

from tests.nt_cases import _verdict, check_rounded

U = 2.0 ** -24
ELEM = 2.0 ** -12
T_F32, T_BF16, T_F16 = 0, 1, 2
TNAME = {T_F32: "f32", T_BF16: "bf16", T_F16: "f16"}
DT = {T_F32: torch.float32, T_BF16: torch.bfloat16, T_F16: torch.float16}
EPS = float(torch.tensor(1e-5, dtype=torch.float32))
GUARD, TAIL = 3, 8
SENT = {torch.float32: -2.0 ** 30, torch.bfloat16: -2.0 ** 30, torch.float16: -61440.0, torch.uint8: 0x55}
REL_FWD = {T_F32: 2e-6, T_BF16: 3e-3, T_F16: 4e-4}
REL_DX, REL_DXB, REL_DX16, REL_DW, REL_DXSUM = 1e-5, 3e-3, 4e-4, 1e-5, 1e-4
KAPPA_PLAIN = 2.0
INF = float("inf")
FOLD_MAX = 64           # CE_LN_FOLD_MAX


def gamma_d(D):
    return min(D, 128) * U


def form_of(D):
    """(IT, NW) of the instantiation LN_DISPATCH picks."""
    it = 1 if D <= 256 else 2 if D <= 512 else 3 if D <= 768 else 4 if D <= 1024 else 8
    return it, (16 if it <= 2 else 8 if it <= 4 else 4)


def bwd_blocks(M, D):
    cap = int(os.environ.get("CE_LN_BWD_BLOCKS", "256"))
    return min(-(-M // form_of(D)[1]), cap)


def q8_ref(x_bf16):
    """torch restatement of ce_quant_rows_fp8 (tests/test_hip_ops.py's _q8_ref): bytes, scales.  Evaluated on the host, as there:
    torch's device conversion to float8_e4m3fn does not round ties to even (-23 became -22; the host and the kernels give -24)."""
    dev = x_bf16.device
    xb = x_bf16.float().cpu()
    amax = xb.abs().amax(dim=-1, keepdim=True)
    m, k = torch.frexp(amax)
    e = 9 - k - (m > 0.875).to(k.dtype)
    live = amax >= 2.0 ** -100
    one = torch.ones_like(amax)
    inv = torch.where(live, torch.ldexp(one, e), one)
    q = (xb * inv).to(torch.float8_e4m3fn)
    return q.view(torch.uint8).to(dev), torch.where(live, torch.ldexp(one, -e), one).flatten().to(dev)


# ---------------------------------------------------------------------------------------------------------------
# reference and bounds (fp64)

def fwd_reference(x, w, b, eps=EPS):
    """x [M, D] of any float type (the operand bits), w, b fp32 [D] -> dict of fp64 reference values and bounds."""
    x, g, b = x.double(), w.double()[None, :], b.double()[None, :]
    D = x.shape[1]
    gd = gamma_d(D)
    mu = x.mean(1, keepdim=True)
    d = x - mu
    A, Ad, Q = x.abs().mean(1, keepdim=True), d.abs().mean(1, keepdim=True), (d * d).mean(1, keepdim=True)
    rstd = (Q + eps) ** -0.5
    xh = d * rstd
    y = xh * g + b
    dmu = gd * A + U * mu.abs()
    dQ = 2 * Ad * dmu + dmu * dmu + (gd + 4 * U) * Q
    rho = dQ / (2 * (Q + eps)) + 4 * U
    dxh = rstd * dmu + xh.abs() * (rho + 3 * U)
    By = g.abs() * dxh + 2 * U * ((xh * g).abs() + y.abs())
    kappa = float(torch.where(Q > 0, A / (Q + eps).sqrt(), torch.zeros_like(Q)).max())       # rows that carry an error of the mean
    return dict(mu=mu[:, 0], rstd=rstd[:, 0], xh=xh, y=y, dmu=dmu[:, 0], rho=rho[:, 0], dxh=dxh, By=By, kappa=kappa)


def bwd_reference(d, x, mean, rstd, w, din):
    """d, din: fp64 [M, D] in true units (din None: no dx_in); x the operand bits; mean, rstd the fp32 arrays given."""
    x, g = x.double(), w.double()[None, :]
    D = x.shape[1]
    gd = gamma_d(D)
    rs = rstd.double()[:, None]
    xh = (x - mean.double()[:, None]) * rs
    gy = d * g
    gx = gy * xh
    c1, c2 = gy.mean(1, keepdim=True), gx.mean(1, keepdim=True)
    xc = xh * c2
    t = gy - c1 - xc
    dx = t * rs + (0 if din is None else din)
    dxh, dgy = 3 * U * xh.abs(), U * gy.abs()
    dc1, dc2 = (gd + 2 * U) * gy.abs().mean(1, keepdim=True), (gd + 6 * U) * gx.abs().mean(1, keepdim=True)
    dt = dgy + dc1 + xh.abs() * dc2 + c2.abs() * dxh + 3 * U * (gy.abs() + c1.abs() + xc.abs())
    Bdx = rs * dt + 2 * U * ((t * rs).abs() + dx.abs())
    tw = d * xh
    return dict(dx=dx, Bdx=Bdx, tw=tw, dtw=4 * U * tw.abs(), tb=d, dtb=torch.zeros_like(d))


def fwd_rel_limit(yt, f):
    """The relative-L2 limit of a forward output of type yt, f = fwd_reference(...) (module docstring)."""
    if yt == T_BF16:
        return REL_FWD[yt]
    return REL_FWD[yt] + REL_FWD[T_F32] * max(0.0, f["kappa"] / KAPPA_PLAIN - 1.0)


def check_abs(got, ref, bound):
    got = got.double()
    return _verdict((got - ref).abs(), bound, got, ref)


def check_colsum(got, base, term, dterm):
    """Column sums of `term` [M, D] added into `base` (None: a plain sum), in any order."""
    M = term.shape[0]
    b = torch.zeros_like(term[0]) if base is None else base.double()
    d = got.double() - b
    want = term.sum(0)
    bound = max(ELEM, M * U) * (term.abs().sum(0) + b.abs()) + dterm.sum(0)
    return _verdict((d - want).abs(), bound, d, want)


def check_equal(got, want):
    """Bit equality of two tensors of the same type as a verdict."""
    same = torch.equal(_bits(got), _bits(want))
    bad = 0 if same else int((_bits(got) != _bits(want)).sum())
    return bad, (0.0 if same else INF), 0.0


def _bits(t):
    t = t.contiguous()
    return t if t.dtype == torch.uint8 else t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def passes(res):
    over, _, rel, limit = res
    return over == 0 and rel < limit


# ---------------------------------------------------------------------------------------------------------------
# fp32 emulations (the checker's own test objects: a faithful kernel in torch, and wrong ones)

def rowsum_lanes(t):
    """Row sums in the kernels' order: per lane the 4-element groups of each 256-column chunk, then a 64-lane tree."""
    M, D = t.shape
    it = -(-D // 256)
    p = torch.zeros(M, it * 256, dtype=torch.float32, device=t.device)
    p[:, :D] = t
    p = p.view(M, it, 64, 4)
    s = torch.zeros(M, 64, dtype=torch.float32, device=t.device)
    for i in range(it):
        s = s + ((p[:, i, :, 0] + p[:, i, :, 1]) + (p[:, i, :, 2] + p[:, i, :, 3]))
    n = 64
    while n > 1:
        n //= 2
        s = s[:, :n] + s[:, n:2 * n]
    return s[:, 0]


def rowsum_serial(t):
    s = torch.zeros(t.shape[0], dtype=torch.float32, device=t.device)
    for j in range(t.shape[1]):
        s = s + t[:, j]
    return s


def emulate_fwd(x, w, b, rowsum=rowsum_lanes, eps=EPS, one_pass=False, eps_outside=False):
    """fp32 LayerNorm forward of x (any float type): (mean, rstd, y) fp32.  one_pass: variance as E[x^2] - mu^2;
    eps_outside: rstd = 1 / (sqrt(Q) + eps)."""
    x = x.float()
    D = torch.tensor(float(x.shape[1]), dtype=torch.float32)
    e = torch.tensor(eps, dtype=torch.float32)
    mu = rowsum(x) / D
    d = x - mu[:, None]
    q = (rowsum(x * x) / D - mu * mu).clamp_min(0) if one_pass else rowsum(d * d) / D
    rs = 1.0 / (q.sqrt() + e) if eps_outside else 1.0 / (q + e).sqrt()
    return mu, rs, d * rs[:, None] * w[None, :] + b[None, :]


def emulate_bwd(d, x, mean, rstd, w, din, rowsum=rowsum_lanes):
    """fp32 LayerNorm backward in true units: d, din fp32 (din None), x any float type -> dx, dgamma, dbeta, dxsum (sums over rows, serial)."""
    x = x.float()
    invD = torch.tensor(1.0 / x.shape[1], dtype=torch.float32)
    rs = rstd[:, None]
    xh = (x - mean[:, None]) * rs
    gy = d * w[None, :]
    c1, c2 = rowsum(gy) * invD, rowsum(gy * xh) * invD
    o = (gy - c1[:, None] - xh * c2[:, None]) * rs
    if din is not None:
        o = o + din
    sums = [torch.zeros_like(w) for _ in range(3)]
    for r in range(x.shape[0]):
        sums[0], sums[1], sums[2] = sums[0] + d[r] * xh[r], sums[1] + d[r], sums[2] + o[r]
    return o, sums[0], sums[1], sums[2]


def store(v, t, mul=1.0):
    """What the kernels store of fp32 v in element type t (fp16: times the scale, saturating)."""
    if t == T_F16:
        return (v * mul).clamp(-65504.0, 65504.0).half()
    return v.to(DT[t])


# ---------------------------------------------------------------------------------------------------------------
# values: one set per (M, D, class, seed), shared by every type combination and layout of a case

class Values:
    def __init__(self, M, D, cls="plain", seed=0, dev="cpu", special=()):
        self.M, self.D, self.cls, self.dev, self.special = M, D, cls, dev, tuple(special)
        g = torch.Generator().manual_seed(seed * 1000003 + M * 7919 + D * 31 + len(cls))
        rn = lambda *s: torch.randn(*s, generator=g)
        x, dy, din = rn(M, D), rn(M, D) * 2.0 ** -13, rn(M, D) * 2.0 ** -13
        const = 3.0
        if cls == "plain":
            x = 2 * x + 0.5
        elif cls == "offset":
            x, const = 0.05 * x + 30, 30.0
        else:
            x = (2 * x + 0.5) * torch.exp((3 * rn(M, 1)).clamp(-4.0, 8.0))
            sc = torch.exp(rn(M, 1).clamp(-2.0, 2.0))
            sc[1:3] = 1.0           # (rows 1, 2 have rstd = eps^-1/2 = 316: a scaled fp16 gradient stays below 65504)
            dy = dy * sc
        if M >= 2:
            x[1] = 0
        if M >= 3:
            x[2] = const
        if M >= 4:
            dy[3] = 2.0 ** -13
        self.zero_cols = D >= 16
        if self.zero_cols:
            dy[:, 8:16] = 0
        if "sat" in special:
            dy[M // 2] *= 2.0 ** 14
        x16 = x.clamp(-65504.0, 65504.0).half()
        if "limit" in special:
            x16[0, D - 1] = 65504.0
        self.holds_limit = bool((x16.abs() == 65504.0).any())
        self.x = {T_F32: x.to(dev), T_F16: x16.to(dev)}
        self.dy32, self.din32 = dy.to(dev), din.to(dev)
        self.w, self.b = (1 + 0.1 * rn(D)).to(dev), (0.1 * rn(D)).to(dev)
        s = 2.0 ** -13 * M ** 0.5
        self.base = [(rn(D) * s).to(dev) for _ in range(3)]         # dgamma, dbeta, dxsum
        perm = torch.randperm(2 * M + 3, generator=g)[:M]
        self.perm = perm.to(torch.int32).to(dev)
        self._f, self._b = {}, {}

    def grad(self, which, t, gs):
        """The stored operand of a gradient (dy / dx_in) in type t under the scale gs."""
        v = self.dy32 if which == "dy" else self.din32
        return store(v, t, gs)

    def fwd(self, xt):
        if xt not in self._f:
            self._f[xt] = fwd_reference(self.x[xt], self.w, self.b)
        return self._f[xt]

    def stats(self, xt):
        """The fp32 mean / rstd the backward is given: the reference's, rounded."""
        f = self.fwd(xt)
        return f["mu"].float(), f["rstd"].float()

    def bwd(self, dyt, xt, dit, gs):
        key = (dyt, xt, dit, gs if T_F16 in (dyt, dit) else 0)
        if key not in self._b:
            un = lambda which, t: self.grad(which, t, gs).double() / (gs if t == T_F16 else 1.0)
            mean, rstd = self.stats(xt)
            self._b[key] = bwd_reference(un("dy", dyt), self.x[xt], mean, rstd, self.w, None if dit is None else un("din", dit))
        return self._b[key]


# ---------------------------------------------------------------------------------------------------------------
# layouts

class Mat:
    """A guarded matrix buffer: `n` rows of D columns at column c0 of a [n + GUARD, ld] allocation filled with `fill`."""

    def __init__(self, n, D, dtype, ld, c0, fill, dev):
        self.n, self.D, self.ld, self.c0, self.dtype = n, D, ld, c0, dtype
        self.buf = torch.full((n + GUARD, ld), fill, dtype=dtype, device=dev)

    def put(self, values, idx=None):
        blk = self.buf[:, self.c0:self.c0 + self.D]
        if idx is None:
            blk[:values.shape[0]] = values
        else:
            blk[idx.long()] = values
        return self

    def get(self, idx=None, M=None):
        blk = self.buf[:, self.c0:self.c0 + self.D]
        return blk[:M] if idx is None else blk[idx.long()]

    def ptr(self):
        return self.buf.data_ptr() + self.c0 * self.buf.element_size()

    def outside_is(self, sentinel, idx=None, M=None):
        mask = torch.ones_like(self.buf, dtype=torch.bool)
        if idx is None:
            mask[:M, self.c0:self.c0 + self.D] = False
        else:
            mask[idx.long(), self.c0:self.c0 + self.D] = False
        return bool((self.buf[mask] == sentinel).all())


def _vec(values, n_out, fill_in, fill_out, dev, dtype=torch.float32):
    """[n + guard] vector: `values` (or fill_in where None) then fill_out."""
    n, extra = n_out
    t = torch.full((n + extra,), fill_out, dtype=dtype, device=dev)
    t[:n] = fill_in if values is None else values
    return t


def _lds(D, layout):
    """(ld, first column, lddxb) of a layout."""
    if layout in ("wide", "rows"):
        return D + 12, 4, (D + 20 if layout == "rows" else D + 12)
    return D, 0, D


NAN = float("nan")
FWD_LAYOUTS = ("dense", "wide", "rows")
BWD_LAYOUTS = ("dense", "wide", "rows", "inplace", "nodxb", "noin")


class FwdLaunch:
    """Buffers of one forward launch, the call, an fp32 emulation into the same buffers, and the checks."""

    def __init__(self, v, layout, xt, yt, q8=False, entry="t"):
        self.v, self.layout, self.xt, self.yt, self.q8, self.entry = v, layout, xt, yt, q8, entry
        M, D, dev = v.M, v.D, v.dev
        ld, c0, _ = _lds(D, layout)
        self.ld = ld
        self.rows = v.perm if layout == "rows" else None
        R = 2 * M + 3 if layout == "rows" else M
        self.x = Mat(R, D, DT[xt], ld, c0, NAN, dev).put(v.x[xt], self.rows)
        self.w, self.b = _vec(v.w, (D, TAIL), 0, NAN, dev), _vec(v.b, (D, TAIL), 0, NAN, dev)
        self.y = Mat(M, D, DT[yt], ld, c0, SENT[DT[yt]], dev).put(torch.full((M, D), NAN, dtype=DT[yt], device=dev))
        self.mean, self.rstd = (_vec(None, (M, GUARD), NAN, SENT[torch.float32], dev) for _ in range(2))
        self.q = self.qs = None
        if q8:
            self.q = Mat(M, D, torch.uint8, ld, c0, SENT[torch.uint8], dev).put(torch.full((M, D), 0x7F, dtype=torch.uint8, device=dev))
            self.qs = _vec(None, (M, GUARD), NAN, SENT[torch.float32], dev)

    def describe(self):
        it, nw = form_of(self.v.D)
        return f"fwd IT {it} NW {nw} x {TNAME[self.xt]} y {TNAME[self.yt]}{' +e4m3' if self.q8 else ''} entry {self.entry} {self.layout}"

    def call(self, **override):
        from clip_event_amd import _lib as L
        v = self.v
        P = lambda t: 0 if t is None else t.data_ptr()
        a = dict(x=self.x.ptr(), x_type=self.xt, ldx=self.ld, rows=P(self.rows), w=P(self.w), b=P(self.b), y=self.y.ptr(), y_type=self.yt,
                 ldy=self.ld, mean=P(self.mean), rstd=P(self.rstd), M=v.M, D=v.D, q8=0 if self.q is None else self.q.ptr(),
                 ldq=self.ld if self.q is not None else 0, qscale=P(self.qs), entry=self.entry)
        assert set(override) <= set(a), override
        a.update(override)
        V, cl = c_void_p, L.lib()
        head = (V(a["rows"]), V(a["w"]), V(a["b"]))
        tail = (V(a["mean"]), V(a["rstd"]), c_int(a["M"]), c_int(a["D"]), c_float(EPS))
        if a["entry"] == "plain":
            return cl.ce_layernorm_fwd(V(a["x"]), c_long(a["ldx"]), *head, V(a["y"]), c_long(a["ldy"]), c_int(int(a["y_type"] == T_F32)), *tail, L.stream())
        typed = (V(a["x"]), c_int(a["x_type"]), c_long(a["ldx"]), *head, V(a["y"]), c_int(a["y_type"]), c_long(a["ldy"]), *tail)
        if a["entry"] == "t":
            return cl.ce_layernorm_fwd_t(*typed, L.stream())
        return cl.ce_layernorm_fwd_q8(*typed, V(a["q8"]), c_long(a["ldq"]), V(a["qscale"]), L.stream())

    def emulate(self, rowsum=rowsum_lanes, **wrong):
        """Fills the outputs as a faithful fp32 kernel would, reading the launch's own buffers."""
        M, D = self.v.M, self.v.D
        mu, rs, y = emulate_fwd(self.x.get(self.rows, M), self.w[:D], self.b[:D], rowsum, **wrong)
        self.mean[:M], self.rstd[:M] = mu, rs
        self.y.put(store(y, self.yt))
        if self.q is not None:
            qb, sc = q8_ref(self.y.get(M=M))
            self.q.put(qb)
            self.qs[:M] = sc
        return self

    def guards_intact(self):
        M = self.v.M
        ok = self.y.outside_is(SENT[DT[self.yt]], M=M) and bool((self.mean[M:] == SENT[torch.float32]).all()) and \
            bool((self.rstd[M:] == SENT[torch.float32]).all())
        if self.q is not None:
            ok = ok and self.q.outside_is(SENT[torch.uint8], M=M) and bool((self.qs[M:] == SENT[torch.float32]).all())
        return ok

    def untouched(self):
        M = self.v.M
        ok = self.guards_intact() and bool(self.y.get(M=M).isnan().all()) and bool(self.mean[:M].isnan().all()) and bool(self.rstd[:M].isnan().all())
        if self.q is not None:
            ok = ok and bool((self.q.get(M=M) == 0x7F).all()) and bool(self.qs[:M].isnan().all())
        return ok

    def check(self):
        v, M = self.v, self.v.M
        f = v.fwd(self.xt)
        res = {"mean": check_abs(self.mean[:M], f["mu"], f["dmu"]) + (INF,),
               "rstd": check_abs(self.rstd[:M], f["rstd"], f["rho"] * f["rstd"]) + (INF,)}
        got = self.y.get(M=M)
        if self.yt == T_F32:
            res["y"] = check_abs(got, f["y"], f["By"]) + (fwd_rel_limit(T_F32, f),)
        else:
            res["y"] = check_rounded(got, f["y"], f["By"], DT[self.yt]) + (fwd_rel_limit(self.yt, f),)
        if self.q is not None:
            qb, sc = q8_ref(got)
            res["q8"] = check_equal(self.q.get(M=M), qb) + (INF,)
            res["qscale"] = check_equal(self.qs[:M], sc) + (INF,)
        return res

    def expected_counters(self):
        """(forward counter >= 1?, backward counter >= 1?); False: that counter must be 0."""
        return (self.xt == T_F16 and self.v.holds_limit), False


class Job(Structure):
    """``ce_ln_fold_job`` of include/clip_event_hip.h."""
    _fields_ = [("partials", c_void_p), ("dw", c_void_p), ("db", c_void_p), ("dxsum", c_void_p), ("blocks", c_int), ("D", c_int)]


class BwdLaunch:
    """Buffers of one backward launch (atomic or partials + fold), the call, an fp32 emulation, and the checks."""

    def __init__(self, v, layout, combo, gs=65536.0, dxsum=True, form="atomic", q8=False, entry="t", blocks=None):
        self.v, self.layout, self.combo, self.gs, self.form, self.q8, self.entry = v, layout, combo, gs, form, q8, entry
        dyt, xt, dit, dot = combo
        M, D, dev = v.M, v.D, v.dev
        ld, c0, lddxb = _lds(D, layout)
        self.ld, self.lddxb = ld, lddxb
        self.rows = v.perm if layout == "rows" else None
        R = 2 * M + 3 if layout == "rows" else M
        self.has_in, self.has_dxb, self.want_dxsum = layout != "noin", layout != "nodxb", dxsum
        assert layout != "inplace" or dit == dot
        assert not q8 or self.has_dxb
        self.dit = dit if self.has_in else None
        self.dy = Mat(M, D, DT[dyt], ld, c0, NAN, dev).put(v.grad("dy", dyt, gs))
        self.x = Mat(R, D, DT[xt], ld, c0, NAN, dev).put(v.x[xt], self.rows)
        self.mean, self.rstd = (_vec(s, (M, GUARD), 0, NAN, dev) for s in v.stats(xt))
        self.w = _vec(v.w, (D, TAIL), 0, NAN, dev)
        sent = SENT[DT[dot]]
        if layout == "inplace":
            self.dx = self.din = Mat(R, D, DT[dot], ld, c0, sent, dev).put(v.grad("din", dit, gs), self.rows)
        else:
            self.dx = Mat(R, D, DT[dot], ld, c0, sent, dev).put(torch.full((M, D), NAN, dtype=DT[dot], device=dev), self.rows)
            self.din = Mat(R, D, DT[dit], ld, c0, NAN, dev).put(v.grad("din", dit, gs), self.rows) if self.has_in else None
        self.dxb = self.q = self.qs = None
        if self.has_dxb:
            self.dxb = Mat(R, D, torch.bfloat16, lddxb, c0, SENT[torch.bfloat16], dev).put(
                torch.full((M, D), NAN, dtype=torch.bfloat16, device=dev), self.rows)
        if q8:
            self.q = Mat(R, D, torch.uint8, ld, c0, SENT[torch.uint8], dev).put(torch.full((M, D), 0x7F, dtype=torch.uint8, device=dev), self.rows)
            self.qs = torch.full((R + GUARD,), SENT[torch.float32], device=dev)
            self.qs[self._idx()] = NAN
        self.sums = [_vec(b, (D, TAIL), 0, SENT[torch.float32], dev) for b in v.base]        # dgamma, dbeta, dxsum (+= into the bases)
        self.gscale = torch.tensor([gs], dtype=torch.float32, device=dev) if T_F16 in (dyt, dit, dot) else None
        self.blocks = self.partials = None
        if form == "partials":
            self.blocks = bwd_blocks(M, D) if blocks is None else blocks
            self.partials = torch.full((self.blocks + GUARD, 3, D), SENT[torch.float32], device=dev)
            self.partials[:self.blocks] = NAN

    def _idx(self):
        return torch.arange(self.v.M, device=self.v.dev) if self.rows is None else self.rows.long()

    def describe(self):
        it, nw = form_of(self.v.D)
        c = "/".join(TNAME[t] for t in self.combo)
        return (f"bwd IT {it} NW {nw} {c} gs 2^{int(math.log2(self.gs))} {self.form}{' dxsum' if self.want_dxsum else ''}"
                f"{' +e4m3' if self.q8 else ''} entry {self.entry} {self.layout}")

    def call(self, **override):
        from clip_event_amd import _lib as L
        v = self.v
        dyt, xt, dit, dot = self.combo
        P = lambda t: 0 if t is None else t.data_ptr()
        a = dict(dy=self.dy.ptr(), dy_type=dyt, lddy=self.ld, x=self.x.ptr(), x_type=xt, ldx=self.ld, rows=P(self.rows), mean=P(self.mean),
                 rstd=P(self.rstd), w=P(self.w), dx_in=self.din.ptr() if self.has_in else 0, dxin_type=dit, dx_out=self.dx.ptr(), dx_type=dot,
                 lddx=self.ld, dxb=self.dxb.ptr() if self.has_dxb else 0, lddxb=self.lddxb, dw=P(self.sums[0]), db=P(self.sums[1]),
                 dxsum=P(self.sums[2]) if self.want_dxsum else 0, gscale=P(self.gscale), M=v.M, D=v.D,
                 q8=0 if self.q is None else self.q.ptr(), ldq=self.ld if self.q is not None else 0, qscale=P(self.qs),
                 partials=P(self.partials), entry=self.entry)
        assert set(override) <= set(a), override
        a.update(override)
        V, cl = c_void_p, L.lib()
        if a["entry"] == "plain":
            return cl.ce_layernorm_bwd(V(a["dy"]), c_long(a["lddy"]), c_int(int(a["dy_type"] == T_F32)), V(a["x"]), c_long(a["ldx"]), V(a["rows"]),
                                       V(a["mean"]), V(a["rstd"]), V(a["w"]), V(a["dx_in"]), V(a["dx_out"]), c_long(a["lddx"]), V(a["dxb"]),
                                       c_long(a["lddxb"]), V(a["dw"]), V(a["db"]), V(a["dxsum"]), c_int(a["M"]), c_int(a["D"]), L.stream())
        head = (V(a["dy"]), c_int(a["dy_type"]), c_long(a["lddy"]), V(a["x"]), c_int(a["x_type"]), c_long(a["ldx"]), V(a["rows"]), V(a["mean"]),
                V(a["rstd"]), V(a["w"]), V(a["dx_in"]), c_int(a["dxin_type"]), V(a["dx_out"]), c_int(a["dx_type"]), c_long(a["lddx"]),
                V(a["dxb"]), c_long(a["lddxb"]))
        q = (V(a["q8"]), c_long(a["ldq"]), V(a["qscale"]))
        if self.form == "partials":
            rc = cl.ce_layernorm_bwd_partials(*head, c_int(int(self.want_dxsum)), V(a["gscale"]), c_int(a["M"]), c_int(a["D"]), *q,
                                              V(a["partials"]), L.stream())
            return rc
        sums = (V(a["dw"]), V(a["db"]), V(a["dxsum"]), V(a["gscale"]), c_int(a["M"]), c_int(a["D"]))
        if a["entry"] == "t":
            return cl.ce_layernorm_bwd_t(*head, *sums, L.stream())
        return cl.ce_layernorm_bwd_q8(*head, *sums, *q, L.stream())

    def fold(self):
        """ce_layernorm_fold of this launch's partials into its bases (one job)."""
        from clip_event_amd import _lib as L
        self.partial_sums = self.partials[:self.blocks].double().sum(0)
        self.partials_before = self.partials.clone()
        job = Job(self.partials.data_ptr(), self.sums[0].data_ptr(), self.sums[1].data_ptr(),
                  self.sums[2].data_ptr() if self.want_dxsum else None, self.blocks, self.v.D)
        return L.lib().ce_layernorm_fold((Job * 1)(job), 1, L.stream())

    def emulate(self, rowsum=rowsum_lanes):
        """Fills the outputs as a faithful fp32 kernel would (atomic form), reading the launch's own buffers."""
        v, M, D = self.v, self.v.M, self.v.D
        dyt, xt, dit, dot = self.combo
        idx = self._idx()
        d = self.dy.get(M=M).float() / (self.gs if dyt == T_F16 else 1.0)
        din = None
        if self.has_in:
            din = self.din.get(idx).float() / (self.gs if dit == T_F16 else 1.0)
        o, dw, db, dxs = emulate_bwd(d, self.x.get(idx), self.mean[:M], self.rstd[:M], self.w[:D], din, rowsum)
        self.dx.put(store(o, dot, self.gs), idx)
        if self.has_dxb:
            self.dxb.put(o.bfloat16(), idx)
        if self.q is not None:
            qb, sc = q8_ref(self.dxb.get(idx))
            self.q.put(qb, idx)
            self.qs[idx] = sc
        for s, t in zip(self.sums, (dw, db, dxs) if self.want_dxsum else (dw, db)):
            s[:D] += t
        return self

    def guards_intact(self):
        M, D, idx = self.v.M, self.v.D, self._idx()
        ok = self.dx.outside_is(SENT[DT[self.combo[3]]], idx)
        if self.has_dxb:
            ok = ok and self.dxb.outside_is(SENT[torch.bfloat16], idx)
        if self.q is not None:
            mask = torch.ones_like(self.qs, dtype=torch.bool)
            mask[idx] = False
            ok = ok and self.q.outside_is(SENT[torch.uint8], idx) and bool((self.qs[mask] == SENT[torch.float32]).all())
        ok = ok and all(bool((s[D:] == SENT[torch.float32]).all()) for s in self.sums)
        if self.partials is not None:
            ok = ok and bool((self.partials[self.blocks:] == SENT[torch.float32]).all())
        return ok

    def untouched(self):
        D, idx = self.v.D, self._idx()
        ok = self.guards_intact() and all(torch.equal(s[:D], b) for s, b in zip(self.sums, self.v.base))
        if self.layout != "inplace":
            ok = ok and bool(self.dx.get(idx).isnan().all())
        if self.has_dxb:
            ok = ok and bool(self.dxb.get(idx).isnan().all())
        if self.q is not None:
            ok = ok and bool((self.q.get(idx) == 0x7F).all()) and bool(self.qs[idx].isnan().all())
        if self.partials is not None:
            ok = ok and bool(self.partials[:self.blocks].isnan().all())
        return ok

    def check(self):
        v, M, D = self.v, self.v.M, self.v.D
        dyt, xt, dit, dot = self.combo
        idx = self._idx()
        r = v.bwd(dyt, xt, self.dit, self.gs)
        got = self.dx.get(idx)
        res = {}
        if dot == T_F32:
            res["dx"] = check_abs(got, r["dx"], r["Bdx"]) + (REL_DX,)
        else:
            res["dx"] = check_rounded(got, r["dx"] * self.gs, r["Bdx"] * self.gs, torch.float16) + (REL_DX16,)
        if self.has_dxb:
            gb = self.dxb.get(idx)
            if dot == T_F32:
                res["dxb"] = check_equal(gb, got.bfloat16()) + (INF,)
            else:
                res["dxb"] = check_rounded(gb, r["dx"], r["Bdx"], torch.bfloat16) + (REL_DXB,)
            if self.q is not None:
                qb, sc = q8_ref(gb)
                res["q8"] = check_equal(self.q.get(idx), qb) + (INF,)
                res["qscale"] = check_equal(self.qs[idx], sc) + (INF,)
        terms = [("dgamma", r["tw"], r["dtw"], REL_DW), ("dbeta", r["tb"], r["dtb"], REL_DW), ("dxsum", r["dx"], r["Bdx"], REL_DXSUM)]
        P = 3 if self.want_dxsum else 2
        if self.partials is not None:
            pb = self.partials_before
            unwritten = int(pb[:self.blocks, :P].isnan().sum()) + int((~pb[:self.blocks, P:].isnan()).sum())
            res["partials written"] = (unwritten, INF if unwritten else 0.0, 0.0, INF)
            for k, (name, term, dterm, lim) in enumerate(terms[:P]):
                res["partials " + name] = check_colsum(self.partial_sums[k], None, term, dterm) + (lim,)
        for k, (name, term, dterm, lim) in enumerate(terms):
            if k < P:
                res[name] = check_colsum(self.sums[k][:D], v.base[k], term, dterm) + (lim,)
                if v.zero_cols and k < 2:
                    res[name + " zero columns"] = check_equal(self.sums[k][8:16], v.base[k][8:16]) + (INF,)
            else:
                res["dxsum untouched"] = check_equal(self.sums[k][:D], v.base[k]) + (INF,)
        return res

    def expected_counters(self):
        return False, (self.combo[3] == T_F16 and "sat" in self.v.special)


# ---------------------------------------------------------------------------------------------------------------
# case table

FWD6 = [(T_F32, T_BF16), (T_F32, T_F32), (T_F32, T_F16), (T_F16, T_BF16), (T_F16, T_F32), (T_F16, T_F16)]
TOWER_FWD = [(T_F32, T_BF16), (T_F16, T_BF16)]
BWD8 = [(T_BF16, T_F32, T_F32, T_F32), (T_F32, T_F32, T_F32, T_F32), (T_BF16, T_F16, T_F16, T_F16), (T_BF16, T_F16, T_F32, T_F16),
        (T_BF16, T_F16, T_F32, T_F32), (T_BF16, T_F16, T_F16, T_F32), (T_F16, T_F32, T_F32, T_F32), (T_F16, T_F16, T_F32, T_F32)]
TOWER_BWD = [BWD8[0], BWD8[2]]           # the block LayerNorms on the fp32 and on the fp16 stream
GS = (65536.0, 1024.0)


def _fwd_specs(combos, layouts=FWD_LAYOUTS):
    """(layout, xt, yt, q8, entry): bf16 outputs with and without the e4m3 copy; fp32 x also through ce_layernorm_fwd."""
    out = []
    for layout in layouts:
        for xt, yt in combos:
            out.append((layout, xt, yt, False, "t"))
            if yt == T_BF16:
                out.append((layout, xt, yt, True, "q8"))
            if xt == T_F32 and yt != T_F16 and layout != "wide":
                out.append((layout, xt, yt, False, "plain"))
    return out


def _bwd_specs(combos, layouts=BWD_LAYOUTS, cross=False, gss=(65536.0,)):
    """dicts of BwdLaunch arguments.  cross: with and without dxsum, atomic and partials, q8 on one of them; otherwise the two
    forms alternate over the layouts (dxsum on)."""
    out = []
    for combo in combos:
        for gs in (gss if T_F16 in (combo[0], combo[2], combo[3]) else (65536.0,)):
            for n, layout in enumerate(layouts):
                if (layout == "inplace" and combo[2] != combo[3]) or (gs != 65536.0 and layout != "dense"):
                    continue
                if cross:
                    for dxsum in (True, False):
                        for form in ("atomic", "partials"):
                            out.append(dict(layout=layout, combo=combo, gs=gs, dxsum=dxsum, form=form,
                                            q8=layout != "nodxb" and dxsum == (form == "atomic"), entry="q8"))
                else:
                    out.append(dict(layout=layout, combo=combo, gs=gs, dxsum=True, form=("atomic", "partials")[n % 2],
                                    q8=layout in ("wide", "rows"), entry="q8" if layout in ("wide", "rows") else "t"))
                if combo[0] != T_F16 and combo[1:] == (T_F32, T_F32, T_F32) and layout == "dense":
                    out.append(dict(layout=layout, combo=combo, gs=gs, dxsum=True, form="atomic", q8=False, entry="plain"))
    return out


class Case:
    def __init__(self, name, M, D, cls="plain", special=(), fwd=(), bwd=()):
        self.name, self.M, self.D, self.cls, self.special, self.fwd, self.bwd = name, M, D, cls, tuple(special), list(fwd), list(bwd)


def _table():
    cases = []
    # every D at M = 37 (3 .. 10 workgroups, a ragged last one), the two stream formats of the tower, every layout
    for D in (4, 64, 256, 260, 512, 516, 768, 1000, 1024, 1028, 2048):
        cases.append(Case(f"M37_D{D}", 37, D, "plain", ("limit",), _fwd_specs(TOWER_FWD), _bwd_specs(TOWER_BWD)))
    # the smallest M
    for M, D in ((1, 4), (1, 260), (3, 768), (5, 1028), (3, 2048), (5, 64)):
        cases.append(Case(f"M{M}_D{D}", M, D, "plain", (), _fwd_specs(TOWER_FWD), _bwd_specs(TOWER_BWD)))
    # every built type combination, with / without dxsum, atomic / partials, both scales: D = 768 and a ragged D
    for D in (768, 260):
        cases.append(Case(f"types_D{D}", 37, D, "plain", ("limit",), _fwd_specs(FWD6),
                          _bwd_specs(BWD8, layouts=("dense", "rows", "inplace", "nodxb", "noin"), cross=True, gss=GS)))
    # ill-conditioned rows and rows of very different scales
    for cls in ("offset", "mixed"):
        for D in (4, 260, 768, 2048):
            cases.append(Case(f"{cls}_D{D}", 37, D, cls, (), _fwd_specs(FWD6, ("dense",)), _bwd_specs(BWD8, ("dense", "inplace"))))
    # a gradient past the fp16 limit: the store clamps and the backward counter says so
    sat = [c for c in BWD8 if c[3] == T_F16]
    cases.append(Case("sat_D260", 37, 260, "plain", ("sat",), (), _bwd_specs(sat, ("dense", "inplace", "rows"))))
    # the row loop at default settings: M = 2 * 256 * NW + 5, so every wave consumes two rows, some three, with a ragged tail
    for M, D in ((8197, 256), (4101, 768), (2053, 1028)):
        cases.append(Case(f"loop_M{M}_D{D}", M, D, "plain", (), _fwd_specs(TOWER_FWD, ("dense",)),
                          _bwd_specs(TOWER_BWD, ("wide", "rows")) + _bwd_specs(BWD8, ("dense", "inplace"))))
    return cases


CASES = _table()

# the environment forms (CE_LN_FWD_RPW, CE_LN_BWD_BLOCKS: read once per process) run this fixed subset in a child each:
# odd M (RPW = 2: the surplus row repeats the last one and must not be stored; BLOCKS = 3: 101 rows are 3-9 loop iterations
# per wave), M = 1, and D = 1028 where RPW = 2 falls back to one row per wave
CHILD_CASES = [Case(f"child_M{M}_D{D}", M, D, "plain", ("limit",), _fwd_specs(FWD6 if D == 768 else TOWER_FWD),
                    _bwd_specs(TOWER_BWD, ("dense", "wide", "inplace", "rows")))
               for M, D in ((101, 260), (101, 768), (101, 1028), (1, 768))]


# ---------------------------------------------------------------------------------------------------------------
# runner

class counters:
    """The fp16-stream saturation counters registered for the duration of a with block; afterwards unregistered (NULL), or the
    process's own buffer (clip_event_amd._lib.sat_counters) registered again where there is one."""

    def __init__(self, dev):
        self.t = torch.zeros(2, dtype=torch.int32, device=dev)

    def __enter__(self):
        from clip_event_amd import _lib as L
        assert L.lib().ce_stream16_set_counters(c_void_p(self.t.data_ptr())) == 0
        return self

    def take(self):
        got = self.t.tolist()
        self.t.zero_()
        return got

    def __exit__(self, *exc):
        from clip_event_amd import _lib as L
        own = L._SAT.get(str(self.t.device))
        L.lib().ce_stream16_set_counters(c_void_p(own.data_ptr() if own is not None else 0))
        return False


def _record(case, ln, rc, res, guards, extra_ok, cnt, log, err=""):
    want = ln.expected_counters()
    cnt_ok = cnt is None or all((c >= 1) if w else (c == 0) for c, w in zip(cnt, want))
    fine = rc == 0 and guards and extra_ok and cnt_ok and all(passes(r) for r in res.values())
    rec = dict(case=case.name, cls=case.cls, form=ln.describe(), rc=rc, guards=guards, counters=cnt, counters_ok=cnt_ok,
               over=sum(r[0] for r in res.values()), worst={k: r[1] for k, r in res.items()}, rel={k: r[2] for k, r in res.items()},
               ok=fine)
    log(f"[ln {case.name} {case.cls}] {rec['form']}: " +
        ", ".join(f"{k}: {r[0]} over, ratio {r[1]:.4f}, rel_l2 {r[2]:.2e}" for k, r in res.items()) +
        f", guards {'intact' if guards else 'WRITTEN'}, counters {cnt}{'' if cnt_ok else ' WRONG'}" +
        ("" if extra_ok else ", FORM MISMATCH") + ("" if rc == 0 else f", rc {rc}: {err}"))
    return rec


def run_case(case, seed=0, dev="cuda:0", log=print):
    """Every forward and backward launch of a case, checked against fp64.  One record per launch; rec["ok"]: rc 0, no element over
    its bound, relative L2 inside the older limits, guards intact, the saturation counters as the values demand, and (partials)
    ce_layernorm_bwd_blocks reporting the workgroup count the environment implies."""
    from clip_event_amd._lib import lib
    cl = lib()
    v = Values(case.M, case.D, case.cls, seed, dev, case.special)
    recs, dense_dx = [], {}
    with counters(dev) as cnt:
        for layout, xt, yt, q8, entry in case.fwd:
            ln = FwdLaunch(v, layout, xt, yt, q8, entry)
            rc = ln.call()
            torch.cuda.synchronize()
            recs.append(_record(case, ln, rc, ln.check() if rc == 0 else {}, ln.guards_intact(), True, cnt.take(), log,
                                cl.ce_last_error().decode() if rc else ""))
        for spec in case.bwd:
            # (the partials buffer is sized from what the library reports; the report is held to what the environment implies)
            ln = BwdLaunch(v, **spec, blocks=cl.ce_layernorm_bwd_blocks(case.M, case.D) if spec["form"] == "partials" else None)
            rc = ln.call()
            extra = True
            if rc == 0 and ln.form == "partials":
                extra = ln.blocks == bwd_blocks(case.M, case.D)
                rc = ln.fold()
            torch.cuda.synchronize()
            res = ln.check() if rc == 0 else {}
            key = (spec["combo"], spec["gs"])
            if rc == 0 and spec["layout"] == "dense" and key not in dense_dx:
                dense_dx[key] = ln.dx.get(M=case.M).clone()
            if rc == 0 and spec["layout"] == "nodxb":
                assert key in dense_dx, "the table must run the dense launch of a type combination before its nodxb launch"
                res["dx == dense dx"] = check_equal(ln.dx.get(M=case.M), dense_dx[key]) + (INF,)
            recs.append(_record(case, ln, rc, res, ln.guards_intact(), extra, cnt.take(), log, cl.ce_last_error().decode() if rc else ""))
    return recs


def run_fold(dev="cuda:0", njobs=65, seed=0):
    """One ce_layernorm_fold call of `njobs` jobs (chunked at CE_LN_FOLD_MAX) mixing D in {4, 260, 768} and blocks in {1, 3, 7},
    every fourth job (j % 4 == 1) with a null dxsum, each into its own non-zero destinations.  Returns (rc, records)."""
    from clip_event_amd import _lib as L
    g = torch.Generator().manual_seed(seed + 77)
    jobs, keep = [], []
    for j in range(njobs):
        D, blocks, null = (4, 260, 768)[j % 3], (1, 3, 7)[(j // 3) % 3], j % 4 == 1
        p = torch.randn(blocks + GUARD, 3, D, generator=g).to(dev)
        dst = [_vec((torch.randn(D, generator=g) * blocks ** 0.5).to(dev), (D, TAIL), 0, SENT[torch.float32], dev) for _ in range(3)]
        keep.append((D, blocks, null, p, dst, [d.clone() for d in dst]))
        jobs.append(Job(p.data_ptr(), dst[0].data_ptr(), dst[1].data_ptr(), None if null else dst[2].data_ptr(), blocks, D))
    rc = L.lib().ce_layernorm_fold((Job * njobs)(*jobs), njobs, L.stream())
    torch.cuda.synchronize()
    recs = []
    for j, (D, blocks, null, p, dst, before) in enumerate(keep):
        term = p[:blocks].double()
        res = {}
        for k in range(3):
            if k == 2 and null:
                res["dxsum untouched"] = check_equal(dst[k], before[k])
            else:
                res[("dgamma", "dbeta", "dxsum")[k]] = check_colsum(dst[k][:D], before[k][:D], term[:, k], torch.zeros_like(term[:, k]))
        guards = all(bool((d[D:] == SENT[torch.float32]).all()) for d in dst)
        recs.append(dict(job=j, D=D, blocks=blocks, null_dxsum=null, guards=guards, over=sum(r[0] for r in res.values()),
                         worst=max(r[1] for r in res.values()), ok=guards and all(r[0] == 0 for r in res.values())))
    return rc, recs
