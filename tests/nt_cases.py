"""The NT GEMM family (``ce_gemm_nt``, ``ce_gemm_nt_fp8``, ``ce_gemm_nt_mx8``: csrc/gemm.hip, csrc/gemm_fp8.hip) against an fp64
reference of the same operand bits: the element-wise checker, the operand / output layouts with guards and poison, the case
table and the runner, shared by tests/test_nt_ops.py and the child process it starts per environment form
(tests/nt_child.py).

Reference (fp64, from the operand bits):  ref = A B^T,  mag = |A| |B|^T  (e4m3 operands: the bytes decoded through
torch.float8_e4m3fn, times sa[m] sb[n], or times 2^(sa8 - 127) 2^(sb8 - 127) per 32-wide block inside the sum; mag scaled
alike),  x = ref + bias (+ resid),  B = 2^-12 (mag + |bias| + |resid|).

Why 2^-12: an fp32 sum of K exact products plus two addends, in any order, errs by at most about K u mag with u = 2^-24
(2^-23 if the matrix unit truncates): below 2^-12 mag for K <= 2048 (the table's one longer K, 3072, stays inside with u =
2^-24 in the worst case and far inside at the sqrt(K) u of random signs).  The scale multiplies of the e4m3 epilogue add 2 ulp.
It is the TN suite's constant (tests/wgrad_cases.py) for the same reason.  None of the bounds is fitted to the kernels.

Per epilogue:
    F32, BIAS_F32, BIAS_RESID_F32      |got - x| <= B.
    BF16, BIAS_BF16, BIAS_RESID_F16    rounding is monotone: RNE(x - B) <= got <= RNE(x + B) in the output type (fp16: the
                                       ends clamped to +-65504 first; the ends are rounded through fp32).  Passes the kernel's
                                       own rounding exactly, fails one ulp off.
    GELUGRAD_BF16 out                  between the bf16 roundings of (ref -+ B') aux, ordered by the sign of aux;
                                       B' = B (1 + 2^-20) covers the fp32 product.
    GELUGRAD_BF16 column sums          added into a base of size sqrt(M): |(got - base) - sum_m ref aux| <= sum_m B' |aux| +
                                       2^-12 (sum_m |ref aux| + |base|); where the launch sums in a second pass (the 128^2
                                       kernel: ce_colsum_bf16 over the bf16 output actually stored, itself checked element-wise)
                                       |(got - base) - sum_m out| <= 2^-12 (sum_m |out| + |base|).  Eight all-zero aux columns
                                       leave the base bit-identical.
    BIAS_GELU, BIAS_QGELU_BF16         f = x sigmoid(1.702 x) (out2 / QGELU's out) or its derivative (BIAS_GELU's out), in
                                       fp64 at x; not monotone, so |got - f(x)| <= 2^-8 (|f(x)| + E) + E with E = L B + delta(x),
                                       L = sup |f'| (1.10 activation, 0.851 derivative), delta(x) = 2^-18 (1 + |x|) the fp32
                                       evaluation error of the kernels' sigmoid (one rounding of the argument = 1.7 |x| 2^-24
                                       relative in the exponential, v_exp_f32 and v_rcp_f32 at 1 ulp each, three more
                                       roundings; the cancellation in 1 - s makes the derivative's error absolute).  2^-8 is
                                       bf16's unit roundoff.
On top of each: the relative-L2 limits of the older tests (REL_L2).

Layouts.  Every buffer has three more rows than its matrix.  Outputs: every element outside [M, N] (rows >= M, columns >= N,
the 8 floats behind the column sums) holds a sentinel that must come back bit-identical, the [M, N] block of an overwritten
output starts as NaN.  Inputs: NaN everywhere outside the operand but inside the allocation (rows >= M of A, aux, resid, sa;
rows >= N of B, sb; columns outside the K slice; bias[N .. N + 8)).
    dense   lda = ldb = K, ldo = ldo2 = ldaux = ldr = N (rounded up to 8 where the epilogue demands it)
    wide    A, B column slices of wider buffers (bf16: ld = K + 24 from column 8; e4m3: ld = K + 32 from column 16);
            out, out2, aux, resid with ld = N + 8 (e4m3: N + 32)
    plus4   dense but ldo = N + 4 (fp32 outputs; the planner sends it to the 128^2 kernel)"""
import math
import os
from ctypes import byref, c_double, c_int, c_long, c_void_p

import torch

(BF16, F32, BIAS_BF16, BIAS_F32, BIAS_RESID_F32, BIAS_GELU, GELUGRAD_BF16, BIAS_RESID_F16, BIAS_QGELU_BF16) = range(9)
EPI_NAMES = ("BF16", "F32", "BIAS_BF16", "BIAS_F32", "BIAS_RESID_F32", "BIAS_GELU", "GELUGRAD_BF16", "BIAS_RESID_F16",
             "BIAS_QGELU_BF16")
ELEM = 2.0 ** -12
BP = 1.0 + 2.0 ** -20                   # B' / B of the GELUGRAD product
U_BF16 = 2.0 ** -8
L_ACT, L_DER = 1.10, 0.851              # sup |f'| of the activation and of its derivative
REL_L2 = {F32: 1e-5, BIAS_F32: 1e-5, BIAS_RESID_F32: 1e-5, BF16: 3e-3, BIAS_BF16: 3e-3, BIAS_GELU: 3e-3, GELUGRAD_BF16: 3e-3,
          BIAS_QGELU_BF16: 3e-3, BIAS_RESID_F16: 4e-4}
REL_L2_MX_F32 = 3e-5                    # block scales 2^14 apart inside one fp32 sum (the older MX test's figure)
REL_L2_COLSUM = 3e-3
SENTINEL, SENTINEL_F16 = -2.0 ** 30, -61440.0     # finite, exact in the buffer's type, far from any result
GUARD = 3
ALL9 = tuple(range(9))
SEVEN = (BF16, BIAS_BF16, BIAS_RESID_F32, BIAS_GELU, GELUGRAD_BF16, BIAS_RESID_F16, BIAS_QGELU_BF16)   # the e4m3 forms' epilogues
FOUR = (BIAS_RESID_F32, BIAS_GELU, GELUGRAD_BF16, BIAS_RESID_F16)
OUT_DTYPE = {F32: torch.float32, BIAS_F32: torch.float32, BIAS_RESID_F32: torch.float32, BIAS_RESID_F16: torch.float16}


def out_dtype(epi):
    return OUT_DTYPE.get(epi, torch.bfloat16)


# ---------------------------------------------------------------------------------------------------------------
# checker: pure torch on fp64 tensors, runs anywhere

def gelu_act(x):
    return x * torch.sigmoid(1.702 * x)


def gelu_der(x):
    s = torch.sigmoid(1.702 * x)
    return s * (1 + 1.702 * x * (1 - s))


def _verdict(err, bound, got, ref):
    """(elements over their bound, largest err / bound, relative L2); NaN counts as over."""
    over = int((~(err <= bound)).sum())
    ratio = torch.where((bound == 0) & (err == 0), torch.zeros_like(err), err / bound)
    worst = float(ratio.nan_to_num(float("inf"), posinf=float("inf")).max()) if err.numel() else 0.0
    rel = float((got - ref).norm() / ref.norm().clamp_min(1e-300))
    return over, worst, rel


def check_f32(got, x, B):
    got = got.double()
    return _verdict((got - x).abs(), B, got, x)


def _rounded(v, dtype):
    if dtype == torch.float16:
        v = v.clamp(-65504.0, 65504.0)
    return v.float().to(dtype).double()


def _implied(got, want, bits):
    """The least |d| with RNE(want + d) = got in a type of `bits` significand bits: how far off the value that was rounded must
    have been (half an ulp of got is allowed for; below a power of two the true allowance is half of that, so this can only
    understate)."""
    _, e = torch.frexp(got)
    if bits == 11:
        e = e.clamp_min(-13)            # fp16 subnormals are 2^-24 apart, whatever their own exponent
    half = torch.ldexp(torch.ones_like(got), e - bits - 1)
    return ((got - want).abs() - half).clamp_min(0.0)


def _interval_verdict(got, lo, hi, want, implied, bound):
    over = int((~((lo <= got) & (got <= hi))).sum())
    ratio = torch.where(implied == 0, torch.zeros_like(implied), implied / bound)
    worst = float(ratio.nan_to_num(float("inf"), posinf=float("inf")).max()) if got.numel() else 0.0
    return over, worst, float((got - want).norm() / want.norm().clamp_min(1e-300))


def check_rounded(got, x, B, dtype):
    """Monotone rounding: RNE(x - B) <= got <= RNE(x + B).  The reported ratio is the implied error before rounding over B."""
    got = got.double()
    lo, hi = _rounded(x - B, dtype), _rounded(x + B, dtype)
    xc = x.clamp(-65504.0, 65504.0) if dtype == torch.float16 else x
    return _interval_verdict(got, lo, hi, xc, _implied(got, xc, 11 if dtype == torch.float16 else 8), B)


def check_gelugrad(got, ref, B, aux):
    got = got.double()
    a, b = _rounded((ref - B * BP) * aux, torch.bfloat16), _rounded((ref + B * BP) * aux, torch.bfloat16)
    lo, hi = torch.minimum(a, b), torch.maximum(a, b)
    want = ref * aux
    return _interval_verdict(got, lo, hi, want, _implied(got, want, 8), B * BP * aux.abs())


def check_colsum(got, base, ref, B, aux, stored=None):
    """Column sums added into `base`.  stored = the bf16 output the launch wrote, where a second pass summed it."""
    d = got.double() - base.double()
    if stored is None:
        want = (ref * aux).sum(0)
        bound = (B * BP * aux.abs()).sum(0) + ELEM * ((ref * aux).abs().sum(0) + base.double().abs())
    else:
        s = stored.double()
        want = s.sum(0)
        bound = ELEM * (s.abs().sum(0) + base.double().abs())
    return _verdict((d - want).abs(), bound, d, want)


def check_gelu(got, x, B, derivative):
    got = got.double()
    f = gelu_der(x) if derivative else gelu_act(x)
    E = (L_DER if derivative else L_ACT) * B + 2.0 ** -18 * (1 + x.abs())
    return _verdict((got - f).abs(), U_BF16 * (f.abs() + E) + E, got, f)


def passes(res, rel_limit):
    over, _, rel = res
    return over == 0 and rel < rel_limit


# ---------------------------------------------------------------------------------------------------------------
# operand values: one set per (shape, kind, seed), shared by every layout and epilogue of a case

def _e4m3(x):
    """fp32 -> e4m3 bytes (saturating at 448: torch's conversion does not saturate)."""
    return x.clamp(-448.0, 448.0).to(torch.float8_e4m3fn).view(torch.uint8)


def _e4m3_values(q):
    return q.view(torch.float8_e4m3fn).float().double()


class Values:
    """Random operands of one problem, generated on the host from `seed` and kept on `dev`, with the fp64 reference.

    A ~ N(0, 1), B ~ N(0, 1 / K).  kind "bf16": rounded to bf16.  "e4m3": divided by a per-row power-of-two scale (2^-7 .. 2^-5
    for A, K^-1/2 times that for B: bytes of N(0, 32^2 .. 128^2)) and rounded to e4m3, saturating.  "mx": one E8M0 byte per row
    and 32 values drawn from [120, 134] (one all-127 row each), the values divided by that block's power of two and rounded to
    e4m3, saturating (a block at 134 holds little more than e4m3's subnormals, one at 120 saturates its tail).
    special "zeros": bias = 0 and one all-zero row of A (exact zeros must come back as zeros);  "zero_row": the zero row
    alone (e4m3: with bias = 0 the matrix unit's own error, 1.5e-5 of the product, would meet the 1e-5 limit undiluted);  "clamp": the fp16 residual
    holds 65000 in one row and -65000 in the next, and two bias columns hold +-600, so that the saturating store clamps at
    both ends (the reference clamps too)."""

    def __init__(self, M, N, K, kind="bf16", seed=0, dev="cpu", special=None):
        self.M, self.N, self.K, self.kind, self.dev, self.special = M, N, K, kind, dev, special
        g = torch.Generator().manual_seed(seed * 1000003 + M * 7919 + N * 31 + K)
        rn = lambda *s: torch.randn(*s, generator=g)
        zero_row = M // 2 if special in ("zeros", "zero_row") else None
        self.sa = self.sb = self.sa8 = self.sb8 = None
        if kind == "bf16":
            a, b = rn(M, K).bfloat16(), (rn(N, K) * K ** -0.5).bfloat16()
            if zero_row is not None:
                a[zero_row] = 0
            self.a, self.b = a.to(dev), b.to(dev)
            Ad, Bd = self.a.double(), self.b.double()
        else:
            a, b = rn(M, K), rn(N, K) * K ** -0.5
            if zero_row is not None:
                a[zero_row] = 0
            if kind == "e4m3":
                ek = round(math.log2(K ** -0.5))
                sa = torch.ldexp(torch.ones(M), torch.randint(-1, 2, (M,), generator=g) - 6)
                sb = torch.ldexp(torch.ones(N), torch.randint(-1, 2, (N,), generator=g) - 6 + ek)
                self.sa, self.sb = sa.to(dev), sb.to(dev)
                a, b = _e4m3(a / sa[:, None]), _e4m3(b / sb[:, None])
            else:
                sa8 = torch.randint(120, 135, (M, K // 32), generator=g).to(torch.uint8)
                sb8 = torch.randint(120, 135, (N, K // 32), generator=g).to(torch.uint8)
                sa8[M // 3] = 127
                sb8[N // 3] = 127
                self.sa8, self.sb8 = sa8.to(dev), sb8.to(dev)
                a = _e4m3(a * torch.exp2(127 - sa8.float()).repeat_interleave(32, dim=1))
                b = _e4m3(b * torch.exp2(127 - sb8.float()).repeat_interleave(32, dim=1))
            self.a, self.b = a.to(dev), b.to(dev)
            Ad, Bd = _e4m3_values(self.a), _e4m3_values(self.b)
            if kind == "mx":
                Ad = Ad * torch.exp2(self.sa8.double() - 127).repeat_interleave(32, dim=1)
                Bd = Bd * torch.exp2(self.sb8.double() - 127).repeat_interleave(32, dim=1)
        self.ref, self.mag = Ad @ Bd.t(), Ad.abs() @ Bd.abs().t()
        if kind == "e4m3":
            s = self.sa.double()[:, None] * self.sb.double()[None, :]
            self.ref, self.mag = self.ref * s, self.mag * s
        del Ad, Bd
        bias = torch.zeros(N) if special == "zeros" else rn(N)
        self.resid = rn(M, N).to(dev)
        r16 = (rn(M, N) * 3).half()
        if special == "clamp":      # 65000 + N(0, 1) alone stays below 65520, where fp16 starts to overflow: two columns of
            r16[M // 3], r16[M // 3 + 1] = 65000.0, -65000.0      # bias +-600 take the sums of those rows past it, both ways
            bias[N // 2], bias[N // 2 + 1] = 600.0, -600.0
        self.bias, self.resid16 = bias.to(dev), r16.to(dev)
        # aux = what the tower feeds: the bf16 QuickGELU derivative of other random pre-activations; 8 all-zero columns
        aux = gelu_der(rn(M, N).double()).float().bfloat16()
        if N >= 16:
            aux[:, 8:16] = 0
        self.aux = aux.to(dev)
        self.colbase = (rn(N) * M ** 0.5).to(dev)
        self._cache = {}

    def x_and_B(self, epi):
        """(x, B) of an epilogue: the exact pre-activation / output and its error magnitude bound, fp64 [M, N]."""
        key = "plain" if epi in (BF16, F32, GELUGRAD_BF16) else "r32" if epi == BIAS_RESID_F32 else "r16" if epi == BIAS_RESID_F16 else "bias"
        if key not in self._cache:
            x, m = self.ref, self.mag
            if key != "plain":
                bias = self.bias.double()[None, :]
                x, m = x + bias, m + bias.abs()
            if key in ("r32", "r16"):
                r = (self.resid if key == "r32" else self.resid16).double()
                x, m = x + r, m + r.abs()
            self._cache[key] = (x, ELEM * m)
        return self._cache[key]


# ---------------------------------------------------------------------------------------------------------------
# layouts: guarded, poisoned buffers of one launch

def _up8(n):
    return (n + 7) // 8 * 8


def _poisoned(values, ld, col0, fill):
    """[rows + GUARD, ld] buffer of values' dtype holding `fill` everywhere but values at [0:rows, col0:col0 + cols]."""
    rows, cols = values.shape
    buf = torch.full((rows + GUARD, ld), fill, dtype=values.dtype, device=values.device)
    buf[:rows, col0:col0 + cols] = values
    return buf


def leading_dims(N, K, kind, layout, epi):
    """(ld and first column of the A / B slices, ldo, ld of out2 / aux / resid, the ldo2 argument of GELUGRAD) of a layout."""
    f8 = kind != "bf16"
    wide = layout == "wide"
    ld, c0 = ((K + 32, 16) if f8 else (K + 24, 8)) if wide else (K, 0)
    extra = (32 if f8 else 8) if wide else 0
    # fp16 rows must be 16-byte multiples (the launcher refuses others), the e4m3 launchers want 8-element rows throughout
    n_ld = _up8(N) if (epi == BIAS_RESID_F16 or f8) else N
    return ld, c0, (N + 4 if layout == "plus4" else n_ld + extra), n_ld + extra, n_ld


def plan_lds(N, K, kind, layout, epi):
    """The leading dimensions of a launch as ``ce_gemm_nt_plan`` takes them (0: an operand the epilogue does not have)."""
    ld, _, ldo, ld2, n_ld = leading_dims(N, K, kind, layout, epi)
    return dict(lda=ld, ldb=ld, ldo=ldo, ldo2=ld2 if epi == BIAS_GELU else n_ld if epi == GELUGRAD_BF16 else 0,
                ldaux=ld2 if epi == GELUGRAD_BF16 else 0, ldr=ld2 if epi in (BIAS_RESID_F32, BIAS_RESID_F16) else 0)


class Launch:
    """Buffers of one (values, layout, epilogue) launch, the call, and the checks of what came back."""

    def __init__(self, v, layout, epi, out2_null=False):
        self.v, self.layout, self.epi, self.out2_null = v, layout, epi, out2_null
        M, N, K, dev = v.M, v.N, v.K, v.dev
        f8 = v.kind != "bf16"
        nan = float("nan")
        ld, c0, self.ldo, self.ld2, n_ld = leading_dims(N, K, v.kind, layout, epi)
        poison = 0x7F if f8 else nan            # 0x7f: NaN in e4m3fn
        self.A, self.B = _poisoned(v.a, ld, c0, poison), _poisoned(v.b, ld, c0, poison)
        self.lda, self.a_off = ld, c0
        self.sa = self.sb = None
        if v.kind == "e4m3":
            self.sa = torch.cat([v.sa, torch.full((GUARD,), nan, device=dev)])
            self.sb = torch.cat([v.sb, torch.full((GUARD,), nan, device=dev)])
        elif v.kind == "mx":        # scale rows are K / 32 bytes apart by contract; 0xff: NaN in E8M0
            self.sa = _poisoned(v.sa8, K // 32, 0, 0xFF)
            self.sb = _poisoned(v.sb8, K // 32, 0, 0xFF)
        dt = out_dtype(epi)
        self.sentinel = SENTINEL_F16 if dt == torch.float16 else SENTINEL
        self.out = torch.full((M + GUARD, self.ldo), self.sentinel, dtype=dt, device=dev)
        self.out[:M, :N] = nan
        self.bias = torch.cat([v.bias, torch.full((8,), nan, device=dev)])
        self.resid = self.aux = self.out2 = self.colsum = None
        self.ldr = self.ldaux = self.ldo2 = 0
        if epi == BIAS_RESID_F32:
            self.resid, self.ldr = _poisoned(v.resid, self.ld2, 0, nan), self.ld2
        elif epi == BIAS_RESID_F16:
            self.resid, self.ldr = _poisoned(v.resid16, self.ld2, 0, nan), self.ld2
        elif epi == BIAS_GELU:
            self.out2 = torch.full((M + GUARD, self.ld2), SENTINEL, dtype=torch.bfloat16, device=dev)
            self.out2[:M, :N] = nan
            self.ldo2 = self.ld2
        elif epi == GELUGRAD_BF16:
            self.aux, self.ldaux = _poisoned(v.aux, self.ld2, 0, nan), self.ld2
            if not out2_null:
                self.colsum = torch.cat([v.colbase, torch.full((8,), SENTINEL, device=dev)])
            self.ldo2 = n_ld
        self.lds = plan_lds(N, K, v.kind, layout, epi)
        assert self.lds == dict(lda=ld, ldb=ld, ldo=self.ldo, ldo2=self.ldo2, ldaux=self.ldaux, ldr=self.ldr)

    def call(self, **override):
        """The C call on the current stream; returns its return code.  `override` replaces arguments by name (the refusal
        tests): pointers as integers, 0 = NULL."""
        from clip_event_amd import _lib as L
        v = self.v
        P = lambda t, off=0: 0 if t is None else t.data_ptr() + off
        es = self.A.element_size()
        a = dict(A=P(self.A, self.a_off * es), lda=self.lda, sa=P(self.sa), B=P(self.B, self.a_off * es), ldb=self.lda, sb=P(self.sb),
                 M=v.M, N=v.N, K=v.K, epi=self.epi, bias=P(self.bias if self.epi not in (BF16, F32, GELUGRAD_BF16) else None),
                 resid=P(self.resid), ldr=self.ldr, out=P(self.out), ldo=self.ldo,
                 out2=P(self.out2 if self.epi == BIAS_GELU else self.colsum), ldo2=self.ldo2, aux=P(self.aux), ldaux=self.ldaux)
        assert set(override) <= set(a), override
        a.update(override)
        V = c_void_p
        tail = (c_int(a["M"]), c_int(a["N"]), c_int(a["K"]), c_int(a["epi"]), V(a["bias"]), V(a["resid"]), c_long(a["ldr"]),
                V(a["out"]), c_long(a["ldo"]), V(a["out2"]), c_long(a["ldo2"]), V(a["aux"]), c_long(a["ldaux"]), L.stream())
        if v.kind == "bf16":
            return L.lib().ce_gemm_nt(V(a["A"]), c_long(a["lda"]), V(a["B"]), c_long(a["ldb"]), *tail)
        fn = L.lib().ce_gemm_nt_fp8 if v.kind == "e4m3" else L.lib().ce_gemm_nt_mx8
        return fn(V(a["A"]), c_long(a["lda"]), V(a["sa"]), V(a["B"]), c_long(a["ldb"]), V(a["sb"]), *tail)

    def guards_intact(self):
        M, N = self.v.M, self.v.N
        ok = bool((self.out[M:] == self.sentinel).all()) and bool((self.out[:M, N:] == self.sentinel).all())
        if self.out2 is not None:
            ok = ok and bool((self.out2[M:] == SENTINEL).all()) and bool((self.out2[:M, N:] == SENTINEL).all())
        if self.colsum is not None:
            ok = ok and bool((self.colsum[N:] == SENTINEL).all())
        return ok

    def untouched(self):
        """After a refused call: guards intact, the NaN blocks still NaN, the column sums still the base."""
        M, N = self.v.M, self.v.N
        ok = self.guards_intact() and bool(self.out[:M, :N].isnan().all())
        if self.out2 is not None:
            ok = ok and bool(self.out2[:M, :N].isnan().all())
        if self.colsum is not None:
            ok = ok and torch.equal(self.colsum[:N], self.v.colbase)
        return ok

    def check(self, colsum_pass=False):
        """{output name: (over, worst ratio, rel_l2, rel_l2 limit)} of the launch's outputs, and whether all of it is fine."""
        v, epi = self.v, self.epi
        M, N = v.M, v.N
        got = self.out[:M, :N]
        x, B = v.x_and_B(epi)
        res = {}
        if epi in (F32, BIAS_F32, BIAS_RESID_F32):
            res["out"] = check_f32(got, x, B) + (REL_L2_MX_F32 if v.kind == "mx" else REL_L2[epi],)
        elif epi in (BF16, BIAS_BF16, BIAS_RESID_F16):
            res["out"] = check_rounded(got, x, B, out_dtype(epi)) + (REL_L2[epi],)
        elif epi == BIAS_QGELU_BF16:
            res["out"] = check_gelu(got, x, B, False) + (REL_L2[epi],)
        elif epi == BIAS_GELU:
            res["out"] = check_gelu(got, x, B, True) + (REL_L2[epi],)
            res["out2"] = check_gelu(self.out2[:M, :N], x, B, False) + (REL_L2[epi],)
        else:
            aux = v.aux.double()
            res["out"] = check_gelugrad(got, x, B, aux) + (REL_L2[epi],)
            if self.colsum is not None:
                res["colsum"] = check_colsum(self.colsum[:N], v.colbase, x, B, aux, got if colsum_pass else None) + (REL_L2_COLSUM,)
                if N >= 16 and not torch.equal(self.colsum[8:16], v.colbase[8:16]):
                    res["colsum zero columns"] = (8, float("inf"), 0.0, REL_L2_COLSUM)
        return res


# ---------------------------------------------------------------------------------------------------------------
# case table

class Case:
    """One problem under one setting of the knobs: every (layout, epilogue) is a launch.

    expect = (kernel, tm, ts) the planner must pick (kernel as in _lib.NT_KERNELS; "NT8" = the e4m3 launcher falls back to
    gemm_nt8_kernel), `expect_by_epi` where the epilogue changes it; queue = the plan's wants_tile_queue.
    budget: ce_gemm_set_cu_budget (256 = the whole chip), dynamic: ce_gemm_set_dynamic_tiles, code / walk: ce_gemm_nt_tune,
    f8tune: ce_gemm_nt_fp8_tune."""

    def __init__(self, name, shape, expect, epis=FOUR, kind="bf16", budget=256, dynamic=0, code=0, walk=1001, f8tune=0,
                 layouts=("dense", "wide"), expect_by_epi=None, queue=False, special=None, null_out2=False):
        self.name, self.shape, self.expect, self.epis, self.kind = name, shape, expect, epis, kind
        self.budget, self.dynamic, self.code, self.walk, self.f8tune = budget, dynamic, code, walk, f8tune
        self.layouts, self.expect_by_epi, self.queue, self.special, self.null_out2 = layouts, expect_by_epi or {}, queue, special, null_out2

    def expected(self, epi):
        return self.expect_by_epi.get(epi, self.expect)


def _c(shape, expect, **kw):
    M, N, K = shape
    tag = "_".join(f"{k}{v}" for k, v in kw.items() if k in ("budget", "dynamic", "code", "walk", "f8tune", "kind", "special"))
    return Case(f"{M}x{N}x{K}" + ("_" + tag if tag else ""), shape, expect, **kw)


S192, P192 = (1100, 520, 192), (2100, 520, 192)
NT128, SKINNY = ("NT128", 4, 0), ("SKINNY", 2, 0)

BF16_CASES = [
    # 128^2, register staged: the smallest problems, ragged K / N, and (M > 512, or N < 256) everything the wide kernels refuse
    _c((1, 4, 8), NT128), _c((8, 8, 8), NT128), _c((20, 64, 128), NT128),
    _c((130, 132, 72), NT128, epis=ALL9, null_out2=True),
    _c((513, 264, 256), NT128), _c((1023, 256, 64), NT128), _c((1024, 248, 64), NT128),       # GELUGRAD: separate column-sum pass
    _c((1025, 264, 192), NT128, epis=(F32, BIAS_F32, BIAS_RESID_F32), layouts=("plus4",)),     # 9 x 3 tiles
    # skinny, M <= 512
    _c((37, 264, 256), SKINNY, epis=ALL9, null_out2=True), _c((512, 264, 256), SKINNY), _c((512, 64, 256), SKINNY),
    _c((8, 3072, 768), SKINNY), _c((256, 768, 3072), SKINNY),
    # loader waves, one round
    _c((1025, 264, 64), ("LW", 3, 0)), _c((1024, 256, 64), ("LW", 3, 0)),                  # a single K tile
    _c(S192, ("LW", 4, 0), budget=32, epis=ALL9, null_out2=True),                            # 9 x 3 tiles
    _c((1500, 520, 192), ("LW", 5, 0), budget=32),
    _c(S192, ("LW", 4, 0), budget=32, special="zeros"), _c(S192, ("LW", 4, 0), budget=32, special="clamp", epis=(BIAS_RESID_F16,)),
    # persistent, 32 workgroups: one height
    _c((1900, 520, 192), ("PERSIST", 3, 0), budget=32),                                     # 60 tiles
    _c(P192, ("PERSIST", 4, 0), budget=32, epis=ALL9, null_out2=True,
       expect_by_epi={e: ("PERSIST", 5, 2) for e in SEVEN}),                                 # two heights: 10 tall panels
    _c(P192, ("PERSIST", 5, 2), budget=32, special="zeros"), _c(P192, ("PERSIST", 5, 2), budget=32, special="clamp", epis=(BIAS_RESID_F16,)),
    _c((2500, 520, 192), ("PERSIST", 4, 0), budget=32), _c((3300, 520, 192), ("PERSIST", 5, 0), budget=32),
    _c((3375, 520, 256), ("PERSIST", 5, 3), budget=32), _c((2700, 520, 192), ("PERSIST", 5, 4), budget=32),
    _c((5377, 520, 192), ("PERSIST", 5, 1), budget=32),                                     # 32 tall panels + 9 of 32 rows
    # tile queue
    _c(P192, ("PERSIST", 5, 2), budget=32, dynamic=1, queue=True),
    _c((2100, 520, 128), ("PERSIST", 5, 2), budget=32, dynamic=1),                          # K < 192: queue off
    _c((2100, 520, 64), ("NT32", 5, 0), budget=32),                                         # multi-round with K < 128
    # forced walks of the persistent kernel
    _c(P192, ("PERSIST", 4, 0), budget=32, walk=1000), _c(P192, ("PERSIST", 5, 2), budget=32, walk=1001),
    _c(P192, ("PERSIST", 4, 0), budget=32, walk=1004),
]
# forced codes at 1100 x 520 x 192
BF16_CASES += [_c(S192, ("NT256x4", tm, 0), code=tm, **(dict(epis=ALL9, null_out2=True) if tm == 5 else {})) for tm in range(3, 9)]
BF16_CASES += [_c(S192, ("NT32", 5, 0), code=32, epis=ALL9, null_out2=True),
               _c(S192, ("NT256x2", 5, 0), code=104, epis=ALL9, null_out2=True),
               _c(S192, ("NT256x2", 3, 0), code=203), _c(S192, ("NT256x2", 4, 0), code=204), _c(S192, ("NT256x2", 5, 0), code=205),
               _c(S192, ("NT160_RING", 5, 0), code=160, epis=ALL9, null_out2=True), _c(S192, ("LW", 3, 0), code=161)]
BF16_CASES += [_c(S192, ("PERSIST", tm, 0), code=code) for code, tm in ((162, 3), (163, 3), (164, 4), (165, 5))]
BF16_CASES += [_c(P192, ("PERSIST", tm, 0), code=code, budget=32) for code, tm in ((162, 4), (163, 3), (164, 4), (165, 5))]
BF16_CASES += [_c(P192, ("PERSIST", 3, 0), code=163, budget=32, dynamic=1, queue=True)]

NT8 = ("NT8", 0, 0)
E4M3_CASES = [
    _c((1100, 520, 256), ("LW", 3, 0), kind="e4m3", budget=256),
    _c((1100, 520, 256), ("LW", 4, 0), kind="e4m3", budget=32, epis=SEVEN, null_out2=True),
    _c((1100, 520, 256), ("LW", 4, 0), kind="e4m3", budget=32, special="zero_row"),
    _c((1700, 520, 256), ("LW", 5, 0), kind="e4m3", budget=32),
    _c((2900, 520, 256), ("PERSIST", 3, 0), kind="e4m3", budget=32),
    _c((2500, 520, 256), ("PERSIST", 4, 0), kind="e4m3", budget=32, epis=SEVEN, null_out2=True),
    _c((2100, 520, 256), ("PERSIST", 4, 3), kind="e4m3", budget=32),
    _c((1537, 1032, 256), ("PERSIST", 4, 2), kind="e4m3", budget=32), _c((4353, 520, 256), ("PERSIST", 4, 1), kind="e4m3", budget=32),
    _c((1100, 520, 128), NT8, kind="e4m3"), _c((1000, 520, 256), NT8, kind="e4m3", epis=SEVEN, null_out2=True),
    _c((130, 136, 256), NT8, kind="e4m3"),
]
E4M3_CASES += [_c((1000, 520, 256), NT8, kind="e4m3", f8tune=t) for t in (4, 5, 6, 8, 105)]
MX_CASES = [_c((130, 136, 128), NT8, kind="mx"), _c((300, 520, 256), NT8, kind="mx", epis=SEVEN, null_out2=True),
            _c((1100, 520, 256), NT8, kind="mx")]

# Dispatch entries the table does not reach: none.  The three two-height forms that need a long tail of short panels -- bf16
# ts = 1, e4m3 ts = 1 and ts = 2 -- come from a search of the planner over budgets 32 .. 256 in steps of 8, M = 1024 .. 6000,
# N in {264, 520, 776, 1032}, K in {192, 256} with BIAS_GELU; the rows above hold the smallest M x N found for each (all at
# budget 32).  tests/test_nt_ops.py checks the table against the dispatch switch of csrc/gemm.hip.
UNREACHED_BF16 = set()
UNREACHED_E4M3 = set()

CASES = BF16_CASES + E4M3_CASES + MX_CASES

# the environment forms run a reduced table each (one child process per form): the budget-32 persistent, LW and NT32 rows.
# budget / dynamic None: the environment's (CE_GEMM_CUS / CE_NT_DYNAMIC) where the form sets it, else 32 / off.
CHILD_CASES = [Case(f"{M}x{N}x{K}", (M, N, K), None, budget=None, dynamic=None)
               for M, N, K in [S192, (1500, 520, 192), (1900, 520, 192), P192, (2500, 520, 192), (3300, 520, 192), (3375, 520, 256),
                               (2700, 520, 192), (2100, 520, 128), (2100, 520, 64)]]


# ---------------------------------------------------------------------------------------------------------------
# runner

class knobs:
    """The case's process-wide knobs for the duration of a with block; restored whatever happens."""

    def __init__(self, case):
        self.case = case

    def __enter__(self):
        from clip_event_amd._lib import lib
        c, cl = self.case, lib()
        budget = c.budget if c.budget is not None else (0 if "CE_GEMM_CUS" in os.environ else 32)
        dynamic = c.dynamic if c.dynamic is not None else -1
        assert cl.ce_gemm_set_cu_budget(budget) == 0 and cl.ce_gemm_set_dynamic_tiles(dynamic) == 0
        if c.walk != 1001 or c.expect is not None:          # (the child leaves the walk to CE_NT_CHUNK)
            cl.ce_gemm_nt_tune(c.walk)
        cl.ce_gemm_nt_tune(c.code)
        cl.ce_gemm_nt_fp8_tune(c.f8tune)
        return self

    def __exit__(self, *exc):
        from clip_event_amd._lib import lib
        cl = lib()
        cl.ce_gemm_nt_tune(0)
        if self.case.expect is not None:
            cl.ce_gemm_nt_tune(1001)
        cl.ce_gemm_set_cu_budget(0)
        cl.ce_gemm_set_dynamic_tiles(-1)
        cl.ce_gemm_nt_fp8_tune(0)
        return False


def planned(case, epi, lds=None):
    """((kernel, tm, ts), wants_tile_queue, plan) under the process's current knobs; dense leading dimensions unless given."""
    from clip_event_amd import _lib as L
    M, N, K = case.shape
    if case.kind == "mx":
        return NT8, False, None
    p = L.gemm_nt_plan(M, N, K, epi, case.kind == "e4m3", **(lds or {}))
    if not p.taken:
        return NT8, False, p
    return (L.NT_KERNELS[p.kernel], p.tm, p.ts), bool(p.wants_tile_queue), p


_FAMILY = {"NT128": "gemm_nt_kernel<%d>", "NT256x2": "gemm_nt256_kernel<%d,*,2>", "NT256x4": "gemm_nt256_kernel<%d,*,4>",
           "NT160_RING": "gemm_nt256_kernel<%d,*,4>",           # the ring reports the 8-wave tile's class
           "NT32": "gemm_nt32_kernel<%d>", "LW": "gemm_nt160lw_kernel<%d,*>", "PERSIST": "gemm_nt160p_kernel<%d,*>",
           "SKINNY": "gemm_nt_skinny_kernel<%d>", "NT8": "gemm_nt8_kernel<%d,*,*>"}


def class_name(kernel, epi, f8):
    """The profiler's name of the class a launch of `kernel` reports (every e4m3 launch reports gemm_nt8_kernel's)."""
    return f"{_FAMILY['NT8' if f8 else kernel] % epi} {EPI_NAMES[epi]}"


def launched():
    """{profiler class name: launches} since the last call (the library's event profiler)."""
    from clip_event_amd._lib import lib
    cl = lib()
    n = cl.ce_profile_num_classes()
    buf = (c_double * (4 * n))()
    cl.ce_profile_collect(buf, c_int(n))
    return {cl.ce_profile_class_name(c).decode(): int(buf[4 * c]) for c in range(n) if buf[4 * c] > 0}


def last_plan():
    from clip_event_amd._lib import lib
    tall, ts = c_int(-1), c_int(-1)
    lib().ce_gemm_nt_last_plan(byref(tall), byref(ts))
    return tall.value, ts.value


def run_case(case, seed=0, dev="cuda:0", log=print):
    """Every (layout, epilogue) launch of a case, checked against fp64.  Returns one record per launch; rec["ok"] says it all:
    rc 0, no element over its bound, relative L2 inside the older limit, guards intact, the kernel form the plan names (and, for
    a case with `expect`, the table names) under the profiler class that form reports."""
    from clip_event_amd._lib import lib
    M, N, K = case.shape
    f8 = case.kind != "bf16"
    v = Values(M, N, K, case.kind, seed, dev, case.special)
    recs = []
    lib().ce_profile_enable(1)
    launched()
    try:
        with knobs(case):
            for layout in case.layouts:
                gelu_out2 = {}
                # (N % 8 != 0: the 128^2 kernel's column-sum pass refuses, so GELUGRAD runs without column sums there;
                #  tests/test_nt_ops.py holds the refusal to writing nothing)
                todo = [(e, e == GELUGRAD_BF16 and N % 8 != 0) for e in case.epis] + ([(GELUGRAD_BF16, True)] if case.null_out2 else [])
                for epi, null2 in dict.fromkeys(todo):
                    ln = Launch(v, layout, epi, out2_null=null2)
                    form, queue, plan = planned(case, epi, ln.lds)
                    rc = ln.call()
                    torch.cuda.synchronize()
                    ran = launched()
                    colsum_pass = form[0] == "NT128" and epi == GELUGRAD_BF16
                    want_classes = {class_name(form[0], epi, f8): 1}
                    if colsum_pass and not null2:
                        want_classes["colsum_bf16"] = 1
                    form_ok = ran == want_classes
                    if plan is not None and plan.taken:
                        form_ok = form_ok and last_plan() == (plan.tall_panels, plan.ts)
                    if case.expect is not None:
                        form_ok = form_ok and form == case.expected(epi) and queue == case.queue
                    res = ln.check(colsum_pass) if rc == 0 else {}
                    guards = ln.guards_intact()
                    fine = rc == 0 and guards and form_ok and all(passes(r[:3], r[3]) for r in res.values())
                    if epi == BIAS_GELU:
                        gelu_out2[form] = ln.out2[:M, :N].clone()
                    if epi == BIAS_QGELU_BF16 and form in gelu_out2:      # the same tile variant: the same bits
                        same = torch.equal(ln.out[:M, :N].view(torch.int16), gelu_out2[form].view(torch.int16))
                        res["qgelu == gelu out2"] = (0 if same else 1, 0.0 if same else float("inf"), 0.0, 1.0)
                        fine = fine and same
                    rec = dict(case=case.name, kind=case.kind, layout=layout, epi=EPI_NAMES[epi] + (" out2=NULL" if null2 else ""),
                               rc=rc, form=list(form), queue=queue, classes=ran, form_ok=form_ok, guards=guards,
                               over=sum(r[0] for r in res.values()), worst=max([r[1] for r in res.values()] or [0.0]),
                               rel={k: r[2] for k, r in res.items()}, ok=fine)
                    log(f"[nt {case.kind} {case.name} {layout} {rec['epi']}] {form[0]} tm {form[1]} ts {form[2]}"
                        f"{' queue' if queue else ''} {'' if form_ok else 'FORM MISMATCH ' + str(ran) + ' '}: " +
                        ", ".join(f"{k}: {r[0]} over, ratio {r[1]:.4f}, rel_l2 {r[2]:.2e}" for k, r in res.items()) +
                        f", guards {'intact' if guards else 'WRITTEN'}" + ("" if rc == 0 else f", rc {rc}: {lib().ce_last_error().decode()}"))
                    recs.append(rec)
                    del ln
    finally:
        launched()
        lib().ce_profile_enable(0)
    return recs
