"""The attention kernels (``ce_attention_fwd`` / ``ce_attention_bwd``: short forward and backward, long forward, long dQ, long
dK / dV) against an fp64 reference of the same bf16 operands: reference, emulation, checker, guarded buffers, case tables and
``run_case``, shared by tests/test_attention_ops.py and the child process it starts per environment form (tests/attn_child.py).

Reference, per (sample, head), fp64 on the bf16-valued q, k, v, dO:
    s = q k^T / 8 (+ causal mask), p = softmax(s), lse = logsumexp(s), o = p v, delta_i = sum_c dO_ic o_ic, dP = dO v^T,
    dS = p (dP - delta) / 8, dq = dS k, dk = dS^T q, dv = p^T dO
and the magnitudes an element's rounding errors scale with:
    omag = p |v|, dvmag = p^T |dO|, dsmag = p (|dO| |v|^T + sum_c |dO_ic| omag_ic) / 8, dqmag = dsmag |k|, dkmag = dsmag^T |q|,
    smag_i = max_j sum_c |q_ic| |k_jc| / 8 (over the keys query i sees).

Emulation: the same formulas in fp64 with the kernels' bf16 roundings (bf = fp64 -> fp32 -> bf16, nearest even): P is packed
to bf16 before the second product (un-normalised, exp(s - rowmax), in the forward; normalised in the backward), dS is packed to
bf16, the outputs are bf16, delta comes from the bf16 o; everything else is fp32 in the kernels and exact here.  It supplies
the noise floor of a faithful kernel; a kernel is never compared with itself.

Criteria, with rho = |got - exact| / mag, per output and per (sample, head), NaN counting as over:
    E  every element: rho <= 2^-7 + 2^-14 (o, dv), 2^-6 + 2^-14 (dq, dk).  bf16 unit roundoff is 2^-8; o and dv take one P
       rounding and one output rounding; dq and dk add what the bf16 o puts into delta (<= 2^-7 of the delta part of dsmag);
       fp32 accumulation, v_exp and the fp32 lse sit inside the 2^-14.
    M  mean rho <= 2 mean rho_emul + 2^-14 (truncation instead of rounding raises the emulation's mean 2.5 - 3.5 x).
    R  max_i mean_c rho[i, :] <= 3 max_i mean_c rho_emul[i, :] + 2^-14 (one wrong row among right ones).
    lse  |lse - exact| <= 2^-14 (1 + smag_i).
    bias_grad  with x the kernel's own bf16 dqkv, per column: |(bias - base) - sum_i x_ic| <= (2^-8 + 2^-18) sum_i |x_ic|
       + 2^-20 |base_c| (the kernels sum their fp32 accumulators: half a bf16 ulp per summand, then fp32 adds and atomics)."""
import functools
from ctypes import c_int, c_long, c_void_p

import torch

E_BOUND = {"o": 2.0 ** -7 + 2.0 ** -14, "dv": 2.0 ** -7 + 2.0 ** -14, "dq": 2.0 ** -6 + 2.0 ** -14, "dk": 2.0 ** -6 + 2.0 ** -14}
FLOOR = 2.0 ** -14
M_FACTOR, R_FACTOR = 2.0, 3.0
LSE_BOUND = 2.0 ** -14
BIAS_REL, BIAS_BASE = 2.0 ** -8 + 2.0 ** -18, 2.0 ** -20
OUTPUTS = ("o", "dq", "dk", "dv")
MAGS = {"o": "omag", "dq": "dqmag", "dk": "dkmag", "dv": "dvmag"}
HD = 64
SENTINEL = -2.0 ** 30       # guard value: finite, exact in bf16 and fp32, far from any result
GUARD = 3                   # guard rows above and below every matrix, guard elements around every vector
KINDS = ("normal", "peaked", "rising", "falling")


def bf(x):
    """fp64 -> fp32 -> bf16 (round to nearest even) -> back to x's type."""
    return x.float().bfloat16().to(x.dtype)


def bf_trunc(x):
    """The same with truncation: what a kernel that drops the low 16 bits of an fp32 would store."""
    return (x.float().contiguous().view(torch.int32) & -65536).view(torch.float32).to(x.dtype)


# ---------------------------------------------------------------------------------------------------------------
# reference and emulation: q, k, v, do are [N, L, 64] (N = (sample, head) pairs of one length)

def causal_keep(L, causal):
    """[L, L] bool: key j visible to query i."""
    keep = torch.ones(L, L, dtype=torch.bool)
    return torch.tril(keep) if causal else keep


def exact(q, k, v, do, causal):
    """fp64 results and magnitudes (see the module docstring)."""
    L = q.shape[1]
    keep = causal_keep(L, causal)
    neg = torch.zeros(L, L, dtype=torch.float64).masked_fill(~keep, float("-inf"))
    s = q @ k.transpose(1, 2) / 8 + neg
    lse = torch.logsumexp(s, dim=-1)
    p = torch.exp(s - lse[..., None])
    o = p @ v
    delta = (do * o).sum(-1, keepdim=True)
    ds = p * (do @ v.transpose(1, 2) - delta) / 8
    omag = p @ v.abs()
    dsmag = p * (do.abs() @ v.abs().transpose(1, 2) + (do.abs() * omag).sum(-1, keepdim=True)) / 8
    smag = (q.abs() @ k.abs().transpose(1, 2) / 8).masked_fill(~keep, 0.0).amax(-1)
    return dict(o=o, lse=lse, dq=ds @ k, dk=ds.transpose(1, 2) @ q, dv=p.transpose(1, 2) @ do,
                omag=omag, dvmag=p.transpose(1, 2) @ do.abs(), dqmag=dsmag @ k.abs(), dkmag=dsmag.transpose(1, 2) @ q.abs(),
                smag=smag)


def emulate(q, k, v, do, causal, rnd=bf, keep=None, scale=0.125, dtype=torch.float64):
    """The formulas with the kernels' rounding points, evaluated in `dtype`.  `keep` ([L, L] bool) replaces the mask and `scale`
    the 1/8 (the self-test's corrupted kernels); returns o, lse, dq, dk, dv and the P / dS the second products used."""
    q, k, v, do = (t.to(dtype) for t in (q, k, v, do))
    L = q.shape[1]
    keep = causal_keep(L, causal) if keep is None else keep
    neg = torch.zeros(L, L, dtype=dtype).masked_fill(~keep, float("-inf"))
    s = q @ k.transpose(1, 2) * scale + neg
    mx = s.amax(-1, keepdim=True)
    pt = torch.exp(s - mx)
    l = pt.sum(-1, keepdim=True)
    o = rnd((rnd(pt) @ v) / l)
    lse = (mx + torch.log(l)).squeeze(-1)
    p = pt / l
    delta = (do * o).sum(-1, keepdim=True)
    ds = rnd(p * (do @ v.transpose(1, 2) - delta) * scale)
    pb = rnd(p)
    return dict(o=o, lse=lse, dq=rnd(ds @ k), dk=rnd(ds.transpose(1, 2) @ q), dv=rnd(pb.transpose(1, 2) @ do), p=pb, ds=ds)


# ---------------------------------------------------------------------------------------------------------------
# checker

def rho(got, ref, mag):
    """|got - ref| / mag; 0 where both vanish, inf where got is NaN or off a zero magnitude."""
    err = (got.double() - ref).abs()
    r = err / mag
    r = torch.where((mag == 0) & (err == 0), torch.zeros_like(r), r)
    return r.nan_to_num(float("inf"), posinf=float("inf"))


def check_output(name, got, ex, em):
    """E, M, R of one output, [N, L, 64] each, decided per (sample, head).  Returns a record with the worst of each figure."""
    r, re_ = rho(got, ex[name], ex[MAGS[name]]), rho(em[name], ex[name], ex[MAGS[name]])
    n = r.shape[0]
    mean, mean_e = r.reshape(n, -1).mean(1), re_.reshape(n, -1).mean(1)
    row, row_e = r.mean(2).amax(1), re_.mean(2).amax(1)
    over = int((~(r <= E_BOUND[name])).sum())
    m_ok = bool((mean <= M_FACTOR * mean_e + FLOOR).all())
    r_ok = bool((row <= R_FACTOR * row_e + FLOOR).all())
    tiny = 2.0 ** -20       # (L = 1: the emulation is exact and the ratios would be x / 0)
    return dict(out=name, over=over, worst=float(r.max()), worst_emul=float(re_.max()),
                mean_ratio=float((mean / mean_e.clamp_min(tiny)).max()), row_ratio=float((row / row_e.clamp_min(tiny)).max()),
                E=over == 0, M=m_ok, R=r_ok, ok=over == 0 and m_ok and r_ok)


def check_all(got, ex, em):
    return [check_output(name, got[name], ex, em) for name in OUTPUTS]


def tripped(recs):
    """{output: 'EMR' letters that failed} of a list of check_output records."""
    return {r["out"]: "".join(c for c in "EMR" if not r[c]) for r in recs}


def check_lse(got, ex):
    """(ok, worst |lse - exact| / (2^-14 (1 + smag)))."""
    ratio = ((got.double() - ex["lse"]).abs() / (LSE_BOUND * (1 + ex["smag"]))).nan_to_num(float("inf"))
    return bool((ratio <= 1).all()), float(ratio.max())


def check_bias(delta, x, base):
    """`delta` = bias - base (fp64 [C]) against the column sums of x ([R, C], the kernel's own bf16 dqkv as fp64).
    Returns (ok, worst error / bound)."""
    err = (delta - x.sum(0)).abs()
    bound = BIAS_REL * x.abs().sum(0) + BIAS_BASE * base.abs()
    ratio = torch.where((err == 0) & (bound == 0), torch.zeros_like(err), err / bound).nan_to_num(float("inf"))
    return bool((err <= bound).all()), float(ratio.max())


# ---------------------------------------------------------------------------------------------------------------
# inputs

def make_inputs(lens, H, kind, seed):
    """Per sample [len, H, 64] bf16 q, k, v, dO (CPU).  Depends on (lens, H, kind, seed) only, so a packed batch and the dense
    batch of the same lengths hold the same values."""
    assert kind in KINDS
    g = torch.Generator().manual_seed(seed)
    out = []
    for n in lens:
        q, k, v, do = (torch.randn(n, H, HD, generator=g) for _ in range(4))
        if kind == "peaked":
            q = q * 8
        elif kind in ("rising", "falling") and n:
            # the scaled score gains 24 j / n (rising) along the keys: in the long kernels the running maximum changes at every
            # key block; falling is the mirror image
            j = torch.arange(n, dtype=torch.float32)
            q[:, :, 0] = 8.0
            k[:, :, 0] = (24.0 * (j if kind == "rising" else n - 1 - j) / n)[:, None]
        out.append(tuple(t.to(torch.bfloat16) for t in (q, k, v, do)))
    return out


class Case:
    """Dense: lens = [L] * B and packed = False; packed: lens as given, L = Lmax."""

    def __init__(self, B, L, H, causal, kind="normal", lens=None, wide=False, seed=None):
        self.B, self.L, self.H, self.causal, self.kind, self.wide = B, L, H, int(causal), kind, wide
        self.packed = lens is not None
        self.lens = list(lens) if self.packed else [L] * B
        assert len(self.lens) == B and max(self.lens) <= L
        self.seed = seed if seed is not None else 7919 * L + 131 * B + 17 * H + 2 * KINDS.index(kind) + self.causal
        shape = "packed" + "_".join(map(str, self.lens)) if self.packed else f"B{B}_L{L}"
        self.name = f"{shape}_H{H}_{'causal' if causal else 'full'}_{kind}_{'wide' if wide else 'dense'}"

    @property
    def key(self):
        return (tuple(self.lens), self.H, self.causal, self.kind, self.seed)


@functools.lru_cache(maxsize=4)
def _reference(key):
    lens, H, causal, kind, seed = key
    samples = make_inputs(lens, H, kind, seed)
    refs = {}
    for n in sorted(set(lens)):
        if n == 0:
            continue
        idx = [b for b, m in enumerate(lens) if m == n]
        # [(sample, head), n, 64] of every sample of this length
        ops = [torch.cat([samples[b][t].double().permute(1, 0, 2) for b in idx]) for t in range(4)]
        refs[n] = (idx, exact(*ops, causal), emulate(*ops, causal))
    return samples, refs


def reference(case):
    """(per-sample bf16 inputs, {length: (sample indices, exact, emulated)}), computed once per case and left unchanged."""
    return _reference(case.key)


# ---------------------------------------------------------------------------------------------------------------
# case tables

def _alternate(cases):
    for i, c in enumerate(cases):
        c.wide = i % 2 == 1
        c.name = c.name.rsplit("_", 1)[0] + ("_wide" if c.wide else "_dense")
    return cases


SHORT_LS = (1, 15, 16, 17, 31, 32, 33, 50, 63, 64, 65, 77, 96, 97, 127, 128)
SHORT_CASES = _alternate([Case(2, L, 3, c) for L in SHORT_LS for c in (0, 1)] +
                         [Case(2, L, 3, c, kind) for L in (33, 77, 128) for kind in KINDS[1:] for c in (0, 1)])
# (B, H) = (1, 3): plain block order; (2, 4): B H a multiple of 8, the XCD-owned order
LONG_CASES = _alternate([Case(1, L, 3, c) for L in (129, 191, 192, 193, 197, 256, 257, 577) for c in (0, 1)] +
                        [Case(2, L, 4, c) for L in (129, 192, 257, 577) for c in (0, 1)] +
                        [Case(1, L, 3, c, kind) for L in (197, 577) for kind in KINDS[1:] for c in (0, 1)])
PACKED_CASES = _alternate([Case(9, 128, 2, 1, lens=[1, 128, 0, 33, 32, 97, 16, 5, 0]),
                           Case(8, 77, 3, 1, lens=[77, 10, 0, 33, 1, 64, 77, 17]),
                           Case(5, 50, 2, 0, lens=[50, 5, 49, 31, 32])])
BITS_CASES = [Case(2, 77, 3, 1, wide=True), Case(2, 257, 4, 0)]
# one process per environment form (tests/attn_child.py): every long kernel, both block orders
CHILD_CASES = _alternate([Case(B, L, H, c) for B, H in ((1, 3), (2, 4)) for L in (129, 192, 257, 577) for c in (0, 1)] +
                         [Case(B, 577, H, c, "rising") for B, H in ((1, 3), (2, 4)) for c in (0, 1)])


def self_test_keys():
    """Every (L, causal, input kind) of the tables above, once."""
    seen = {}
    for c in SHORT_CASES + LONG_CASES + CHILD_CASES:
        seen.setdefault((c.L, c.causal, c.kind), None)
    for c in PACKED_CASES:
        for n in c.lens:
            if n:
                seen.setdefault((n, c.causal, c.kind), None)
    return sorted(seen)


# ---------------------------------------------------------------------------------------------------------------
# GPU side: guarded buffers and the calls

class Buffers:
    """Every operand and output inside a taller (GUARD rows above and below) and, in the wide layout, wider (+ 8 columns) buffer
    filled with SENTINEL.  Dense: ld = lddq = 3 D, ldo = lddo = D; wide: each + 8.  The live part of an output starts as NaN:
    an element the kernel leaves unwritten fails the element bound; lse ([B, H, L] fp32) and bias ([3 D] fp32, N(0, 1) base
    values) sit between GUARD / 8 sentinel elements."""

    def __init__(self, case, dev):
        samples, _ = reference(case)
        self.case, D = case, case.H * HD
        self.D, self.rows = D, sum(case.lens)
        pad = 8 if case.wide else 0
        self.ld, self.ldo, self.lddo, self.lddq = 3 * D + pad, D + pad, D + pad, 3 * D + pad
        R = self.rows
        cat = lambda t: torch.cat([s[t].reshape(-1, D) for s in samples]) if R else torch.zeros(0, D, dtype=torch.bfloat16)
        self.qkv = self._matrix(R, self.ld, torch.cat([cat(0), cat(1), cat(2)], dim=1), dev)
        self.dout = self._matrix(R, self.lddo, cat(3), dev)
        self.inputs = (self.qkv.clone(), self.dout.clone())
        self.cu = None
        if case.packed:
            self.cu = torch.tensor([sum(case.lens[:b]) for b in range(case.B + 1)], dtype=torch.int32, device=dev)
        self.n_lse = case.B * case.H * case.L
        g = torch.Generator().manual_seed(case.seed + 1)
        self.bias_base = torch.randn(3 * D, generator=g).to(dev)
        self.dev = dev
        self.fresh()

    @staticmethod
    def _matrix(R, ld, live, dev):
        buf = torch.full((R + 2 * GUARD, ld), SENTINEL, dtype=torch.bfloat16, device=dev)
        buf[GUARD:GUARD + R, :live.shape[1]] = live.to(dev)
        return buf

    def fresh(self):
        """New outputs: NaN where the kernels must write, SENTINEL elsewhere."""
        R, D, dev = self.rows, self.D, self.dev
        nan = lambda cols: torch.full((R, cols), float("nan"), dtype=torch.bfloat16)
        self.o = self._matrix(R, self.ldo, nan(D), dev)
        self.dqkv = self._matrix(R, self.lddq, nan(3 * D), dev)
        self.lse = torch.full((self.n_lse + 2 * GUARD,), SENTINEL, device=dev)
        self.lse[GUARD:GUARD + self.n_lse] = float("nan")
        self.bias = torch.full((3 * D + 8,), SENTINEL, device=dev)
        self.bias[:3 * D] = self.bias_base

    def forward(self, ld=None, B=None, cu="own"):
        from clip_event_amd._lib import lib, ptr, stream
        c = self.case
        return lib().ce_attention_fwd(ptr(self.qkv[GUARD:]), c_long(self.ld if ld is None else ld), ptr(self.o[GUARD:]),
                                      c_long(self.ldo), ptr(self.lse[GUARD:]), ptr(self.cu if cu == "own" else cu),
                                      c_int(c.B if B is None else B), c_int(c.L), c_int(c.H), c_int(c.causal), stream())

    def backward(self, bias=True, ld=None, B=None, cu="own"):
        from clip_event_amd._lib import lib, ptr, stream
        c = self.case
        return lib().ce_attention_bwd(ptr(self.qkv[GUARD:]), c_long(self.ld if ld is None else ld), ptr(self.o[GUARD:]),
                                      c_long(self.ldo), ptr(self.dout[GUARD:]), c_long(self.lddo), ptr(self.lse[GUARD:]),
                                      ptr(self.dqkv[GUARD:]), c_long(self.lddq), ptr(self.bias) if bias else c_void_p(0),
                                      ptr(self.cu if cu == "own" else cu), c_int(c.B if B is None else B), c_int(c.L),
                                      c_int(c.H), c_int(c.causal), stream())

    # -- what came back --------------------------------------------------------------------------------------
    def live(self, buf, cols):
        return buf[GUARD:GUARD + self.rows, :cols]

    def _matrix_guards(self, buf, cols):
        R = self.rows
        return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + R:] == SENTINEL).all()) and \
            bool((buf[GUARD:GUARD + R, cols:] == SENTINEL).all())

    def guards(self):
        """{buffer: untouched} of everything around the outputs, and the inputs bit for bit."""
        n = self.n_lse
        return {"o": self._matrix_guards(self.o, self.D), "dqkv": self._matrix_guards(self.dqkv, 3 * self.D),
                "lse": bool((self.lse[:GUARD] == SENTINEL).all()) and bool((self.lse[GUARD + n:] == SENTINEL).all()),
                "bias": bool((self.bias[3 * self.D:] == SENTINEL).all()),
                "inputs": torch.equal(self.qkv, self.inputs[0]) and torch.equal(self.dout, self.inputs[1])}

    def untouched(self):
        """Nothing written at all (a refused call, a length-0 batch): outputs as fresh() left them."""
        nan_or = lambda buf, cols: bool(torch.isnan(self.live(buf, cols).float()).all())
        n = self.n_lse
        return all(self.guards().values()) and nan_or(self.o, self.D) and nan_or(self.dqkv, 3 * self.D) and \
            bool(torch.isnan(self.lse[GUARD:GUARD + n]).all()) and torch.equal(self.bias[:3 * self.D], self.bias_base)

    def bits(self):
        """o, lse, dqkv as integers (bit-for-bit comparisons, NaN included)."""
        return (self.o.view(torch.int16).clone(), self.lse.view(torch.int32).clone(), self.dqkv.view(torch.int16).clone())

    def sample_rows(self, b):
        r0 = sum(self.case.lens[:b])
        return slice(r0, r0 + self.case.lens[b])

    def gather(self, idx, n):
        """The kernels' o, dq, dk, dv as fp64 [(sample, head), n, 64] and lse [(sample, head), n] of the samples `idx` of
        length n (CPU)."""
        c, D = self.case, self.D
        o, dqkv = self.live(self.o, D).cpu().double(), self.live(self.dqkv, 3 * D).cpu().double()
        lse = self.lse[GUARD:GUARD + self.n_lse].cpu().double().view(c.B, c.H, c.L)
        heads = lambda m, b: m[self.sample_rows(b)].reshape(n, c.H, HD).permute(1, 0, 2)
        got = {"o": torch.cat([heads(o, b) for b in idx]), "lse": torch.cat([lse[b, :, :n] for b in idx])}
        for t, name in enumerate(("dq", "dk", "dv")):
            got[name] = torch.cat([heads(dqkv[:, t * D:(t + 1) * D], b) for b in idx])
        return got


def run_case(case, dev="cuda:0", log=print, bufs=None):
    """Forward, then backward on the kernel's own o and lse (as the tower gives them), everything checked against fp64.
    Returns (record, buffers); record['ok'] is the verdict."""
    import torch.cuda
    _, refs = reference(case)
    bufs = Buffers(case, dev) if bufs is None else bufs
    bufs.fresh()
    rc_f = bufs.forward()
    rc_b = bufs.backward() if rc_f == 0 else -1
    torch.cuda.current_stream().synchronize()
    rec = dict(case=case.name, rc=(rc_f, rc_b), outputs=[], lse_ok=True, lse_worst=0.0)
    worst = {name: dict(out=name, over=0, worst=0.0, worst_emul=0.0, mean_ratio=0.0, row_ratio=0.0, E=True, M=True, R=True, ok=True)
             for name in OUTPUTS}
    if rc_f == 0 and rc_b == 0:
        for n, (idx, ex, em) in refs.items():
            got = bufs.gather(idx, n)
            for r in check_all(got, ex, em):
                w = worst[r["out"]]
                w["over"] += r["over"]
                for f in ("worst", "worst_emul", "mean_ratio", "row_ratio"):
                    w[f] = max(w[f], r[f])
                for f in ("E", "M", "R", "ok"):
                    w[f] = w[f] and r[f]
            ok, ratio = check_lse(got["lse"], ex)
            rec["lse_ok"], rec["lse_worst"] = rec["lse_ok"] and ok, max(rec["lse_worst"], ratio)
    rec["outputs"] = list(worst.values())
    x = bufs.live(bufs.dqkv, 3 * bufs.D).cpu().double()
    rec["bias_ok"], rec["bias_worst"] = check_bias(bufs.bias[:3 * bufs.D].cpu().double() - bufs.bias_base.cpu().double(), x,
                                                   bufs.bias_base.cpu().double())
    rec["guards"] = bufs.guards()
    # a length-0 sample has nothing written for it: its lse rows are as fresh() left them
    lse = bufs.lse[GUARD:GUARD + bufs.n_lse].view(case.B, case.H, case.L)
    rec["guards"]["empty samples"] = all(bool(torch.isnan(lse[b]).all()) for b, n in enumerate(case.lens) if n == 0)
    rec["ok"] = (rc_f == 0 and rc_b == 0 and all(w["ok"] for w in rec["outputs"]) and rec["lse_ok"] and rec["bias_ok"] and
                 all(rec["guards"].values()))
    for w in rec["outputs"]:
        log(f"[attn {case.name}] {w['out']}: worst rho {w['worst']:.3e} (bound {E_BOUND[w['out']]:.3e}, emulation "
            f"{w['worst_emul']:.3e}), {w['over']} over, mean rho / emulation's {w['mean_ratio']:.2f}, worst row / emulation's "
            f"{w['row_ratio']:.2f}" + ("" if w["ok"] else f"  FAILED {tripped([w])[w['out']]}"))
    log(f"[attn {case.name}] lse {rec['lse_worst']:.3f} of its bound, bias_grad {rec['bias_worst']:.3f} of its bound, guards "
        + ("untouched" if all(rec["guards"].values()) else f"WRITTEN {[k for k, v in rec['guards'].items() if not v]}")
        + ("" if (rc_f, rc_b) == (0, 0) else f", rc {rc_f} / {rc_b}"))
    return rec, bufs


def summarise(recs):
    """{output: largest worst rho, mean ratio, worst-row ratio} over a list of run_case records."""
    out = {}
    for name in OUTPUTS:
        ws = [w for r in recs for w in r["outputs"] if w["out"] == name]
        out[name] = {f: max((w[f] for w in ws), default=0.0) for f in ("worst", "mean_ratio", "row_ratio")}
    out["lse"] = max((r["lse_worst"] for r in recs), default=0.0)
    out["bias"] = max((r["bias_worst"] for r in recs), default=0.0)
    return out
