"""Op-level checks of the low-rank adapter kernels (csrc/lora.hip): ``ce_lora_merge`` and ``ce_lora_grad`` against fp64
restatements with per-element bounds, in the style of tests/test_partial_ops.py: sentinel guards around every buffer, NaN in what a
kernel must write, ``U = 2^-24``.

Shapes ``(out, in, rank, scale)``: the smallest at which a ragged tile (72 x 40, 200 x 136), a ragged strip (72, 200, 520 rows), a
rank that is no multiple of the instruction's k (1, 3), the largest rank (64: the second rank tile of the gradient kernel) and a fold
over several strips (200, 256, 520 rows) can go wrong; ``PAIR`` puts two matrices of different shape and rank into one table, which
exercises ``tile_start`` / ``strip_start`` / ``ws_start``."""
from ctypes import c_int, c_size_t, c_void_p

import pytest
import torch

DEV = "cuda:0"
U = 2.0 ** -24          # fp32 unit roundoff
BF = 2.0 ** -8          # the bf16 term of the merge bound
GUARD = 64              # sentinel elements on either side of every buffer (256 / 128 bytes: the data stays 16-byte aligned)
gpu = pytest.mark.gpu

GRID = [(64, 64, 4, 2.0), (72, 40, 1, 1.0), (96, 32, 8, 2.0), (200, 136, 3, 16.0 / 3.0), (256, 64, 64, 0.25), (520, 72, 16, 1.0)]
PAIR = [(200, 136, 3, 16.0 / 3.0), (96, 32, 8, 2.0)]
CASES = [[g] for g in GRID] + [PAIR]
IDS = ["x".join(str(v) for v in g[:3]) for g in GRID] + ["pair"]


def _lib():
    from clip_event_amd._lib import lib, ptr, stream
    return lib(), ptr, stream


def _gen(seed):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return g


def _bits(t):
    return t.contiguous().view(torch.int16) if t.element_size() == 2 else t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


class _Guarded:
    """A buffer between two runs of a sentinel; ``.t`` is the data, ``intact()`` says whether the sentinels still stand."""

    def __init__(self, data: torch.Tensor, sentinel: float = -7.25):
        n = data.numel()
        self.full = torch.full((n + 2 * GUARD,), sentinel, dtype=data.dtype, device=DEV)
        self.t = self.full[GUARD:GUARD + n].view(data.shape)
        self.t.copy_(data)
        self.sentinel = sentinel

    def intact(self):
        s = torch.full((GUARD,), self.sentinel, dtype=self.full.dtype, device=DEV)
        return _same_bits(self.full[:GUARD], s) and _same_bits(self.full[-GUARD:], s)


def _scale32(s):
    return float(torch.tensor(s, dtype=torch.float32))


class _Mat:
    """The eight buffers of one adapted matrix, guarded; outputs start as NaN (fp32) or 4.0 / -4.0 (bf16)."""

    def __init__(self, shape, seed, exact=False):
        out, inn, r, s = shape
        self.out, self.inn, self.r, self.s = out, inn, r, _scale32(s)
        g = _gen(seed)
        if exact:
            w0 = torch.randint(-4095, 4096, (out, inn), generator=g, device=DEV).float() / 4096
            a = torch.randint(-1, 2, (r, inn), generator=g, device=DEV).float() / 32
            b = torch.randint(-1, 2, (out, r), generator=g, device=DEV).float() / 32
            gw = torch.randint(-2, 3, (out, inn), generator=g, device=DEV).float() / 4
        else:
            w0 = torch.randn(out, inn, generator=g, device=DEV) * 0.05
            a = torch.randn(r, inn, generator=g, device=DEV) * 0.1
            b = torch.randn(out, r, generator=g, device=DEV) * 0.1
            gw = torch.randn(out, inn, generator=g, device=DEV)
        nan = float("nan")
        self.w0, self.a, self.b, self.gw = _Guarded(w0), _Guarded(a), _Guarded(b), _Guarded(gw)
        self.w16 = _Guarded(torch.full((out, inn), 4.0, dtype=torch.bfloat16, device=DEV))
        self.wt = _Guarded(torch.full((inn, out), -4.0, dtype=torch.bfloat16, device=DEV))
        self.ga = _Guarded(torch.full((r, inn), nan, device=DEV))
        self.gb = _Guarded(torch.full((out, r), nan, device=DEV))
        self.w0_before, self.gw_before = w0.clone(), gw.clone()

    def spec(self, wt=True):
        p = lambda g: g.t.data_ptr()          # noqa: E731
        return (p(self.w0), p(self.w16), p(self.wt) if wt else 0, p(self.a), p(self.b), p(self.gw), p(self.ga), p(self.gb),
                self.out, self.inn, self.r, self.s)

    def guards_intact(self):
        return all(b.intact() for b in (self.w0, self.a, self.b, self.gw, self.w16, self.wt, self.ga, self.gb))

    # ---- fp64 restatements ----
    def merged64(self):
        """``(W0 + s B A, |W0| + s |B| |A|)`` in fp64."""
        w0, a, b = self.w0_before.double(), self.a.t.double(), self.b.t.double()
        return w0 + self.s * (b @ a), w0.abs() + self.s * (b.abs() @ a.abs())

    def grads64(self):
        """``(dA, bound of dA, dB, bound of dB)`` in fp64 from the dW in the buffer."""
        gw, a, b = self.gw.t.double(), self.a.t.double(), self.b.t.double()
        da, db = self.s * (b.t() @ gw), self.s * (gw @ a.t())
        return (da, (self.out + 2) * U * self.s * (b.abs().t() @ gw.abs()), db, (self.inn + 2) * U * self.s * (gw.abs() @ a.abs().t()))


def _table(mats, wt=True):
    from clip_event_amd._lib import lora_job_table
    host, tiles, strips = lora_job_table([m.spec(wt) for m in mats])
    dev = torch.frombuffer(bytearray(bytes(host)), dtype=torch.uint8).to(DEV)
    return host, dev, tiles, strips


def _merge(mats, write_master=0, wt=True):
    cl, ptr, stream = _lib()
    host, dev, tiles, _ = _table(mats, wt)
    rc = cl.ce_lora_merge(host, ptr(dev), c_int(len(mats)), c_int(tiles), c_int(write_master), stream())
    torch.cuda.synchronize()
    assert rc == 0, cl.ce_last_error()


def _grad(mats, slack=0):
    """Runs ``ce_lora_grad``; returns the guarded workspace (NaN before the call)."""
    cl, ptr, stream = _lib()
    host, dev, _, strips = _table(mats)
    need = cl.ce_lora_grad_workspace_bytes(host, c_int(len(mats)))
    assert need == 4 * sum(((m.out + 63) // 64) * m.r * m.inn for m in mats), (need, cl.ce_last_error())
    ws = _Guarded(torch.full((need // 4 + slack,), float("nan"), device=DEV))
    rc = cl.ce_lora_grad(host, ptr(dev), c_int(len(mats)), c_int(strips), ptr(ws.t), c_size_t(need), stream())
    torch.cuda.synchronize()
    assert rc == 0, cl.ce_last_error()
    return ws


def _ratio(err, bound):
    return float((err / bound.clamp_min(1e-300)).nan_to_num(float("inf")).max())


# ---- merge ---------------------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("shapes", CASES, ids=IDS)
def test_merge_against_fp64(shapes):
    """``ce_lora_merge``: per element ``|mirror - ref64| <= 2^-8 |ref64| + (r + 2) U mag (1 + 2^-8)`` with ``mag = |W0| + s |B| |A|``
    (bf16's rounding, then the fp32 chain of r products, the scale and the add); every W^T bit is its mirror bit transposed; W0
    keeps its bits; the guards stand.  Then ``write_master=1``: W0 within the second term of the bound, and the mirror is W0's RNE
    cast bit for bit."""
    mats = [_Mat(s, 300 + i) for i, s in enumerate(shapes)]
    _merge(mats)
    for m in mats:
        ref, mag = m.merged64()
        chain = (m.r + 2) * U * mag
        err = (m.w16.t.double() - ref).abs()
        bound = BF * ref.abs() + chain * (1 + BF)
        print(f"[merge {m.out}x{m.inn} r{m.r}] worst |err| / bound {_ratio(err, bound):.3f}")
        assert bool((err <= bound).all())
        assert _same_bits(m.wt.t, m.w16.t.t())
        assert _same_bits(m.w0.t, m.w0_before)
        assert m.guards_intact()
    _merge(mats, write_master=1)
    for m in mats:
        ref, mag = m.merged64()
        err = (m.w0.t.double() - ref).abs()
        bound = (m.r + 2) * U * mag
        print(f"[merge master {m.out}x{m.inn} r{m.r}] worst |err| / bound {_ratio(err, bound):.3f}")
        assert bool((err <= bound).all())
        assert _same_bits(m.w16.t, m.w0.t.to(torch.bfloat16))
        assert _same_bits(m.wt.t, m.w16.t.t())
        assert m.guards_intact()


@gpu
def test_merge_without_a_transposed_copy():
    """``wt`` NULL: the mirror is what it is with one, and nothing else is written."""
    a, b = _Mat(GRID[3], 310), _Mat(GRID[3], 310)
    _merge([a])
    _merge([b], wt=False)
    assert _same_bits(a.w16.t, b.w16.t)
    assert _same_bits(b.wt.t, torch.full_like(b.wt.t, -4.0)) and b.guards_intact()


@gpu
@pytest.mark.parametrize("shapes", CASES, ids=IDS)
def test_exactly_summable(shapes):
    """W0 in multiples of 2^-12 below 1, A and B in {0, +-2^-5}, s a power of two: every product and partial sum of the merge is
    exact in fp32, so the mirror EQUALS bf16(W0 + s B A) computed in fp64.  With dW in {0, +-1/4, +-1/2} the same holds for the
    gradients in any summation order: dA and dB equal the fp64 results -- a dropped, doubled or misplaced term shows."""
    pow2 = {16.0 / 3.0: 4.0}
    mats = [_Mat((o, i, r, pow2.get(s, s)), 320 + k, exact=True) for k, (o, i, r, s) in enumerate(shapes)]
    _merge(mats)
    _grad(mats)
    for m in mats:
        ref, _ = m.merged64()
        assert _same_bits(m.w16.t, ref.float().to(torch.bfloat16))
        assert _same_bits(m.wt.t, m.w16.t.t())
        da, _, db, _ = m.grads64()
        assert torch.equal(m.ga.t.double(), da) and torch.equal(m.gb.t.double(), db)
        assert m.guards_intact()


# ---- gradients -----------------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("shapes", CASES, ids=IDS)
def test_grad_against_fp64(shapes):
    """``ce_lora_grad``: ``|dA - ref| <= (out + 2) U s |B|^T |dW|`` and ``|dB - ref| <= (in + 2) U s |dW| |A|^T`` per element (the
    dot-product bound, valid in any order); dW keeps its bits; the guards stand, the workspace's too (one float more than needed is
    given and stays NaN); a second call on the same buffers, which finds the first call's results in them, and a run on fresh
    buffers both give the same bits."""
    mats = [_Mat(s, 340 + i) for i, s in enumerate(shapes)]
    ws = _grad(mats, slack=4)
    assert ws.intact() and bool(ws.t[-4:].isnan().all())
    first = [(m.ga.t.clone(), m.gb.t.clone()) for m in mats]
    for m in mats:
        da, bound_a, db, bound_b = m.grads64()
        ra, rb = _ratio((m.ga.t.double() - da).abs(), bound_a), _ratio((m.gb.t.double() - db).abs(), bound_b)
        print(f"[grad {m.out}x{m.inn} r{m.r}] worst |err| / bound: dA {ra:.3f}, dB {rb:.3f}")
        assert ra <= 1.0 and rb <= 1.0
        assert _same_bits(m.gw.t, m.gw_before)
        assert m.guards_intact()
    _grad(mats)                                             # stores, does not accumulate
    again = [_Mat(s, 340 + i) for i, s in enumerate(shapes)]
    _grad(again)                                            # run to run
    for m, n, (ga, gb) in zip(mats, again, first):
        assert _same_bits(m.ga.t, ga) and _same_bits(m.gb.t, gb)
        assert _same_bits(n.ga.t, ga) and _same_bits(n.gb.t, gb)


# ---- refusals ------------------------------------------------------------------------------------------------------------------

def _refused(rc, cl, *words):
    msg = cl.ce_last_error().decode()
    assert rc == -22, (rc, msg)
    for w in words:
        assert w in msg, msg


@gpu
def test_null_table_is_refused():
    cl, ptr, stream = _lib()
    ws = torch.zeros(64, device=DEV)
    _refused(cl.ce_lora_merge(None, None, c_int(1), c_int(1), c_int(0), stream()), cl, "ce_lora_merge", "NULL")
    _refused(cl.ce_lora_grad(None, None, c_int(1), c_int(1), ptr(ws), c_size_t(256), stream()), cl, "ce_lora_grad", "NULL")
    m = _Mat(GRID[0], 360)
    host, _, tiles, _ = _table([m])
    _refused(cl.ce_lora_merge(host, c_void_p(0), c_int(1), c_int(tiles), c_int(0), stream()), cl, "device copy")
    assert cl.ce_lora_grad_workspace_bytes(None, c_int(1)) == 0


@gpu
@pytest.mark.parametrize("rank", [0, 65])
def test_rank_out_of_range_is_refused(rank):
    cl, ptr, stream = _lib()
    m = _Mat(GRID[0], 361)
    host, dev, tiles, strips = _table([m])
    host[0].rank = rank
    _refused(cl.ce_lora_merge(host, ptr(dev), c_int(1), c_int(tiles), c_int(0), stream()), cl, f"rank {rank}", "1..64")
    ws = torch.zeros(1 << 16, device=DEV)
    _refused(cl.ce_lora_grad(host, ptr(dev), c_int(1), c_int(strips), ptr(ws), c_size_t(ws.numel() * 4), stream()), cl,
             f"rank {rank}", "1..64")
    assert cl.ce_lora_grad_workspace_bytes(host, c_int(1)) == 0


@gpu
@pytest.mark.parametrize("rows,cols", [(68, 40), (72, 36)])
def test_rows_and_cols_must_be_multiples_of_8(rows, cols):
    cl, ptr, stream = _lib()
    m = _Mat(GRID[1], 362)                                  # 72 x 40 buffers: the claimed shapes stay inside them
    host, dev, tiles, strips = _table([m])
    host[0].rows, host[0].cols = rows, cols
    _refused(cl.ce_lora_merge(host, ptr(dev), c_int(1), c_int(tiles), c_int(0), stream()), cl, "multiples of 8")
    ws = torch.zeros(1 << 16, device=DEV)
    _refused(cl.ce_lora_grad(host, ptr(dev), c_int(1), c_int(strips), ptr(ws), c_size_t(ws.numel() * 4), stream()), cl,
             "multiples of 8")


@gpu
def test_small_workspace_is_refused():
    cl, ptr, stream = _lib()
    m = _Mat(GRID[5], 363)
    host, dev, _, strips = _table([m])
    need = cl.ce_lora_grad_workspace_bytes(host, c_int(1))
    ws = torch.zeros(need // 4, device=DEV)
    _refused(cl.ce_lora_grad(host, ptr(dev), c_int(1), c_int(strips), ptr(ws), c_size_t(need - 4), stream()), cl, "too small",
             str(need))
    _refused(cl.ce_lora_grad(host, ptr(dev), c_int(1), c_int(strips), None, c_size_t(need), stream()), cl, "too small")
    torch.cuda.synchronize()
    assert bool(m.ga.t.isnan().all()) and bool(m.gb.t.isnan().all())      # nothing was launched
