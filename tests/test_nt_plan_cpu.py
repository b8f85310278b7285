"""CPU (no GPU): the NT GEMM launch policy (csrc/nt_plan.cpp) through ``ce_gemm_nt_plan`` -- pinned plans and the
preconditions the kernels rely on over a sweep of shapes and knobs.  Every test restores the process-wide knobs it sets."""
import contextlib
import random

import pytest

from clip_event_amd import _lib as L

COLS = {"NT128": 128, "NT256x2": 128, "SKINNY": 64}                 # tile width; every other family: 256
CODES = [0, 3, 4, 5, 6, 7, 8, 32, 104, 160, 161, 162, 163, 164, 165, 203, 204, 205]      # ce_gemm_nt_tune
F8_EPI = (L.EPI_BF16, L.EPI_BIAS_BF16, L.EPI_BIAS_RESID_F32, L.EPI_BIAS_RESID_F16, L.EPI_BIAS_GELU, L.EPI_BIAS_QGELU_BF16,
          L.EPI_GELUGRAD_BF16)
TWO_HEIGHTS = F8_EPI                                                # epilogues built with two tile heights (nt_plan.hpp)
# (kernel, tm, ts) the library can launch (dispatch in csrc/gemm.hip)
BF16_FORMS = ({("NT128", 4, 0), ("SKINNY", 2, 0), ("NT32", 5, 0), ("NT160_RING", 5, 0)} |
              {(k, tm, 0) for k in ("NT256x2", "LW", "PERSIST") for tm in (3, 4, 5)} |
              {("NT256x4", tm, 0) for tm in range(3, 9)} | {("PERSIST", 5, ts) for ts in (1, 2, 3, 4)})
F8_FORMS = {("LW", 3, 0), ("LW", 4, 0), ("LW", 5, 0), ("PERSIST", 3, 0), ("PERSIST", 4, 0)} | {("PERSIST", 4, ts) for ts in (1, 2, 3)}


@pytest.fixture(scope="module")
def lib():
    from clip_event_amd import build
    build.build()
    return L.lib()


@contextlib.contextmanager
def knobs(lib, budget=256, dynamic=0, code=0, walk=1001):
    try:
        assert lib.ce_gemm_set_cu_budget(budget) == 0 and lib.ce_gemm_set_dynamic_tiles(dynamic) == 0
        lib.ce_gemm_nt_tune(walk)
        lib.ce_gemm_nt_tune(code)
        yield
    finally:
        lib.ce_gemm_nt_tune(0)
        lib.ce_gemm_nt_tune(1001)
        assert lib.ce_gemm_set_cu_budget(0) == 0 and lib.ce_gemm_set_dynamic_tiles(-1) == 0


def _plan(M, N, K, epi=L.EPI_BF16, fp8=False, **ld):
    p = L.gemm_nt_plan(M, N, K, epi, fp8, **ld)
    return p, L.NT_KERNELS[p.kernel]


@pytest.mark.parametrize("M,N,K,kernel,tm,ts,tall,tiles_m,wgs", [
    (12800, 3072, 768, "PERSIST", 5, 4, 64, 84, 256),
    (12800, 2304, 768, "PERSIST", 5, 0, 0, 80, 256),
    (12800, 768, 768, "LW", 5, 0, 0, 80, 240),
    (11137, 512, 512, "LW", 3, 0, 0, 117, 234),
    (11137, 2048, 512, "PERSIST", 5, 3, 32, 95, 256),
    (10807, 1536, 512, "PERSIST", 4, 0, 0, 85, 256),
    (2900, 1032, 192, "LW", 3, 0, 0, 31, 155),
    (5000, 2304, 128, "PERSIST", 3, 0, 0, 53, 256)])
def test_pinned_bf16_plans_at_the_default_knobs(lib, M, N, K, kernel, tm, ts, tall, tiles_m, wgs):
    with knobs(lib):
        p, name = _plan(M, N, K)
    assert (name, p.tm, p.ts, p.tall_panels, p.tiles_m, p.workgroups, p.taken) == (kernel, tm, ts, tall, tiles_m, wgs, 1)


@pytest.mark.parametrize("M,N,K,tm,ts,tall,short", [(18464, 1024, 1024, 4, 3, 64, 107), (18464, 4096, 1024, 4, 3, 112, 43),
                                                    (9000, 2048, 512, 3, 0, 0, 94)])
def test_pinned_fp8_plans(lib, M, N, K, tm, ts, tall, short):
    with knobs(lib):
        p, name = _plan(M, N, K, fp8=True)
    assert (name, p.taken, p.tm, p.ts, p.tall_panels, p.tiles_m - p.tall_panels) == ("PERSIST", 1, tm, ts, tall, short)


def test_pinned_plans_under_a_cu_budget_of_97(lib):
    with knobs(lib, budget=97):
        p, name = _plan(12800, 768, 768)
        assert (name, p.tm, p.ts, p.tall_panels, p.tiles_m - p.tall_panels, p.workgroups) == ("PERSIST", 5, 4, 32, 60, 97)
        p, name = _plan(12800, 3072, 768)
        assert (name, p.tm, p.ts, p.workgroups) == ("PERSIST", 5, 0, 97)


def _check_preconditions(p, kernel, M, N, K, epi, fp8, budget, ld):
    """What the kernels rely on (none of them re-checks it)."""
    case = (M, N, K, epi, fp8, budget, ld, kernel, p.tm, p.ts)
    lda, ldb, ldo, ldo2, ldaux, ldr = ld
    aligned = N % 8 == 0 and ldo % 8 == 0 and ldo2 % 8 == 0 and ldaux % 8 == 0
    out_bytes = 4 if epi in (L.EPI_F32, L.EPI_BIAS_F32, L.EPI_BIAS_RESID_F32) else 2
    fits31 = max(M * ldo * out_bytes, M * ldo2 * 2, M * ldaux * 2, M * ldr * 4) < 2 ** 31
    if fp8:
        eligible = (M >= 1024 and N >= 256 and K % 128 == 0 and K >= 256 and aligned and lda % 16 == 0 and ldb % 16 == 0 and
                    fits31 and epi in F8_EPI)
        assert bool(p.taken) == eligible, case
        if not p.taken:
            return
    assert p.taken == 1 and (kernel, p.tm, p.ts) in (F8_FORMS if fp8 else BF16_FORMS), case
    assert p.ts == 0 or epi in TWO_HEIGHTS, case
    rows, short = 32 * p.tm, 32 * p.ts
    if p.ts == 0:
        assert p.tall_panels == 0 and p.tiles_m == -(-M // rows), case
    else:                                       # the panels cover M exactly once and the last short panel is not empty
        n_short = p.tiles_m - p.tall_panels
        assert p.tall_panels >= 1 and n_short >= 1, case
        assert p.tall_panels * rows + (n_short - 1) * short < M <= p.tall_panels * rows + n_short * short, case
        assert p.tall_panels * rows < M, case
    assert p.tiles_n == -(-N // COLS.get(kernel, 256)), case
    tiles = p.tiles_m * p.tiles_n
    assert 1 <= p.workgroups <= tiles and p.lds_bytes <= 160 * 1024 and 64 <= p.block <= 1024, case
    if kernel == "PERSIST":
        assert p.workgroups == min(tiles, budget) and K >= 128, case
    else:
        assert p.workgroups == tiles and p.tile_chunk == 0, case
    if kernel in ("LW", "PERSIST"):
        assert fits31, case
    if kernel not in ("NT128", "SKINNY"):       # the families with 64-column K tiles and 16-byte epilogue accesses
        assert K % 64 == 0 and aligned and M >= 1024 and N >= 256, case
    if kernel == "SKINNY":
        assert M <= 512 and K % 256 == 0 and aligned and ldr % 4 == 0, case
    if p.wants_tile_queue:
        assert kernel == "PERSIST" and not fp8 and tiles > p.workgroups and K >= 192 and p.tile_chunk == 0, case
    if fp8:
        assert kernel in ("LW", "PERSIST") and p.tile_chunk == 0 and p.tm <= (4 if kernel == "PERSIST" else 5), case


def test_preconditions_hold_over_a_sweep(lib):
    rng = random.Random(20)
    Ms = [1, 31, 320, 1023, 1024, 2900, 5000, 11137, 12800, 33000] + [rng.randrange(1025, 40000) for _ in range(3)]
    Ns = [256, 512, 768, 1032, 1536, 2048, 2304, 3072]
    Ks = [64, 128, 192, 256, 512, 768]
    epis = [L.EPI_BF16, L.EPI_F32, L.EPI_BIAS_RESID_F32, L.EPI_GELUGRAD_BF16, L.EPI_BIAS_GELU]
    shapes = [(M, N, K, epis[(i + j + k) % len(epis)]) for i, M in enumerate(Ms) for j, N in enumerate(Ns) for k, K in enumerate(Ks)]
    fields = [name for name, _ in L.NTPlan._fields_]
    points = 0
    try:
        for budget in (256, 224, 97, 61):
            assert lib.ce_gemm_set_cu_budget(budget) == 0
            for dynamic in (0, 1):
                assert lib.ce_gemm_set_dynamic_tiles(dynamic) == 0
                auto8 = {}
                for code in CODES + [1000, 1004]:         # the last two: XCD-owned walks at the automatic tile choice
                    lib.ce_gemm_nt_tune(code if code >= 1000 else 1001)
                    lib.ce_gemm_nt_tune(code if code < 1000 else 0)
                    for M, N, K, epi in shapes:
                        ld = (K, K, N, N if epi in (L.EPI_BIAS_GELU, L.EPI_GELUGRAD_BF16) else 0,
                              N if epi == L.EPI_GELUGRAD_BF16 else 0, N if epi == L.EPI_BIAS_RESID_F32 else 0)
                        p, kernel = _plan(M, N, K, epi)
                        _check_preconditions(p, kernel, M, N, K, epi, False, budget, ld)
                        if code >= 1000:
                            assert not p.wants_tile_queue and (kernel != "PERSIST" or p.tile_chunk > 0), (M, N, K, code)
                        p8, kernel8 = _plan(M, N, K, epi, True)
                        _check_preconditions(p8, kernel8, M, N, K, epi, True, budget, ld)
                        got8 = [getattr(p8, f) for f in fields]
                        assert auto8.setdefault((M, N, K, epi), got8) == got8      # forced codes and walks: not on the e4m3 path
                        points += 2
        # leading dimensions: an output row stride that breaks the 16-byte epilogue accesses, and operands that span >= 2 GiB
        lib.ce_gemm_nt_tune(0)
        assert lib.ce_gemm_set_cu_budget(256) == 0
        for M, N, K in [(33000, 768, 768), (33000, 3072, 512), (12800, 2304, 768), (2900, 1032, 192)]:
            for epi in (L.EPI_BF16, L.EPI_F32, L.EPI_BIAS_RESID_F32):
                for ldo, ldr in [(N + 4, N), (40000, N), (N, 40000), (N, N)]:
                    for code in (0, 161, 162):
                        lib.ce_gemm_nt_tune(code)
                        ld = (K, K, ldo, 0, 0, ldr if epi == L.EPI_BIAS_RESID_F32 else 0)
                        for fp8 in (False, True):
                            p, kernel = _plan(M, N, K, epi, fp8, ldo=ldo, ldr=ld[5])
                            _check_preconditions(p, kernel, M, N, K, epi, fp8, 256, ld)
                            points += 1
    finally:
        lib.ce_gemm_nt_tune(0)
        lib.ce_gemm_nt_tune(1001)
        assert lib.ce_gemm_set_cu_budget(0) == 0 and lib.ce_gemm_set_dynamic_tiles(-1) == 0
    assert points > 100000


def test_plan_query_reports_bad_arguments(lib):
    import ctypes
    plan = L.NTPlan()
    z = ctypes.c_long(0)
    assert lib.ce_gemm_nt_plan(0, 8, 8, 0, 0, z, z, z, z, z, z, ctypes.byref(plan)) == -22
    assert b"ce_gemm_nt_plan" in lib.ce_last_error()
    assert lib.ce_gemm_nt_plan(8, 8, 8, 99, 0, z, z, z, z, z, z, ctypes.byref(plan)) == -22
    assert lib.ce_gemm_nt_plan(8, 8, 8, 0, 0, z, z, z, z, z, z, None) == -22
