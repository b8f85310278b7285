"""CPU (no GPU): the TN (weight-gradient) GEMM launch policy (csrc/tn_plan.cpp) through ``ce_gemm_tn_plan`` and the tower's
grouping of blocks into launches through ``ce_tower_wgrad_cuts`` -- pinned plans (worked out from the launcher's arithmetic
before the planner existed), pinned cuts, and the preconditions the kernels rely on over a sweep of groups and knobs.  The
knobs go in by value, so nothing here touches the environment."""
import ctypes
import random

import pytest

from clip_event_amd import _lib as L
from tests.test_wgrad_ops import ENV_FORMS
from tests.wgrad_cases import block

KNOB_OF = {"CE_GEMM_TN": "variant", "CE_TN3_SPLITS": "force_splits", "CE_TN3_DEPTH": "depth", "CE_TN3_ROWS": "rows",
           "CE_TN3_LW": "loader_waves"}
KERNELS = {"gemm_tn_kernel", "gemm_tn2_kernel", "gemm_tn3_kernel<48,3>", "gemm_tn3_kernel<32,4>", "gemm_tn3lw_kernel<48,3>",
           "gemm_tn3lw_kernel<32,4>"}                                  # what the launcher's switch names (csrc/gemm.hip)


def knobs_of(env):
    return L.TNKnobs(**{KNOB_OF[name]: int(value) for name, value in env.items()})


@pytest.fixture(scope="module")
def lib():
    from clip_event_amd import build
    build.build()
    return L.lib()


def _summary(p):
    return L.TN_FORMS[p.form], p.tiles, p.splits, p.m_per_split, p.workgroups, p.kernel_overwrites, p.zero_fill_first


@pytest.mark.parametrize("shapes,M,call,expected", [
    (block(768), 12800, {}, ("v3", 108, 2, 6400, 216, 0, 0)),
    (block(768), 12800, dict(overwrite=True), ("v3", 108, 2, 6400, 216, 0, 1)),
    (block(768) * 7, 12800, dict(overwrite=True), ("v3", 756, 1, 12800, 756, 1, 0)),
    (block(768) * 4 + [(2304, 768)], 12800, dict(overwrite=True), ("v3", 459, 1, 12800, 459, 1, 0)),
    (block(512), 11137, {}, ("v3", 48, 5, 2240, 240, 0, 0)),
    (block(512) * 6, 11137, dict(overwrite=True), ("v3", 288, 1, 11200, 288, 1, 0)),
    (block(768), 2048, {}, ("v3", 108, 1, 2048, 108, 0, 0)),
    (block(768), 2049, dict(splits=33), ("v3", 108, 33, 64, 3564, 0, 0)),
    (block(768), 2047, {}, ("v2", 432, 1, 2048, 432, 0, 0)),
    (block(768), 256, dict(overwrite=True), ("v2", 432, 1, 256, 432, 0, 1)),
    ([(768, 768), (520, 264), (3072, 768)], 12800, dict(overwrite=True), ("v2", 195, 2, 6400, 390, 0, 1)),
    ([(256, 256)], 12800, {}, ("v3", 1, 16, 832, 16, 0, 0)),
    ([(8, 8)], 1, {}, ("v2", 1, 1, 64, 1, 0, 0)),
    (block(1024), 18464, {}, ("v3", 192, 1, 18496, 192, 0, 0))])
def test_pinned_plans_at_the_default_knobs(lib, shapes, M, call, expected):
    p = L.gemm_tn_plan(shapes, M, knobs=L.TNKnobs(), **call)
    assert _summary(p) == expected
    assert p.kernel == ("gemm_tn3lw_kernel<48,3>" if expected[0] == "v3" else "gemm_tn2_kernel")


def test_pinned_plans_with_explicit_knobs(lib):
    shapes, M = block(768), 10837
    assert _summary(L.gemm_tn_plan(shapes, M, overwrite=True, knobs=L.TNKnobs(force_splits=5))) == ("v3", 108, 5, 2176, 540, 0, 1)
    v2 = L.gemm_tn_plan(shapes, M, knobs=L.TNKnobs(variant=2))
    assert _summary(v2) == ("v2", 432, 1, 10880, 432, 0, 0)
    v1 = L.gemm_tn_plan(shapes, M, knobs=L.TNKnobs(variant=1))
    assert (L.TN_FORMS[v1.form], v1.kernel, v1.splits, v1.m_per_split) == ("v1", "gemm_tn_kernel", v2.splits, v2.m_per_split)
    for rows, lw, block_size, lds in [(48, 1, 768, 147456), (32, 1, 768, 131072), (48, 0, 1024, 147456), (32, 0, 1024, 131072)]:
        p = L.gemm_tn_plan(shapes, M, knobs=L.TNKnobs(rows=rows, loader_waves=lw))
        name = f"gemm_tn3{'lw' if lw else ''}_kernel<{rows},{3 if rows == 48 else 4}>"
        assert (p.kernel, p.rows, p.stages, p.block, p.lds_bytes) == (name, rows, 3 if rows == 48 else 4, block_size, lds)
    # a caller's split beats the forced one, the forced one beats the model
    assert L.gemm_tn_plan(shapes, M, splits=3, knobs=L.TNKnobs(force_splits=5)).splits == 3
    # today's parsing: any rows but exactly 32 mean 48; depth is clamped to 1..3
    odd = L.gemm_tn_plan(shapes, M, knobs=L.TNKnobs(rows=40, depth=9))
    assert (odd.rows, odd.depth, L.gemm_tn_plan(shapes, M, knobs=L.TNKnobs(depth=0)).depth) == (48, 3, 1)


def _check_preconditions(p, shapes, M, splits, overwrite, knobs):
    """What the kernels rely on (none of them re-checks it)."""
    case = (shapes, M, splits, overwrite, [getattr(knobs, f) for f, _ in L.TNKnobs._fields_])
    count, m_tiles = len(shapes), -(-M // 64)
    form = L.TN_FORMS[p.form]
    assert p.m_per_split % 64 == 0 and 1 <= p.splits <= m_tiles, case
    assert (p.splits - 1) * p.m_per_split < M <= p.splits * p.m_per_split, case
    assert p.workgroups == p.tiles * p.splits, case
    per_problem = [p.tiles_n[i] * p.tiles_k[i] for i in range(count)]
    assert sum(per_problem) == p.tile_end[count - 1] == p.tiles and all(t >= 1 for t in per_problem), case
    assert [p.tile_end[i] for i in range(count)] == [sum(per_problem[:i + 1]) for i in range(count)], case
    assert all(p.tile_end[i] == p.tiles for i in range(count, L.TN_MAX_GROUP)), case
    takes_256 = knobs.variant == 3 and M >= 2048 and all(n % 256 == 0 and k % 256 == 0 for n, k in shapes)
    assert (form == "v3") == takes_256 and (form == "v1") == (knobs.variant == 1), case
    edge = 256 if form == "v3" else 128
    assert all((p.tiles_n[i], p.tiles_k[i]) == (-(-n // edge), -(-k // edge)) for i, (n, k) in enumerate(shapes)), case
    if p.kernel_overwrites:
        assert form == "v3" and p.splits == 1 and overwrite, case
    assert p.zero_fill_first == int(bool(overwrite) and not p.kernel_overwrites), case
    assert 1 <= p.depth <= 3 and p.lds_bytes <= 160 * 1024 and p.kernel in KERNELS, case
    assert p.prof_class == (64 if form == "v3" else 71), case                       # CE_PROF_GEMM_TN / CE_PROF_GEMM_TN2
    if form == "v3":
        assert (p.rows, p.stages) in ((48, 3), (32, 4)) and p.lds_bytes == p.rows * p.stages * 1024, case
        assert p.block == (768 if knobs.loader_waves else 1024), case
        if splits <= 0 and knobs.force_splits <= 0:                                  # the model's choice
            assert p.tiles * p.splits <= 256 or p.splits == 1, case
    else:
        assert p.block == 256, case


def test_preconditions_hold_over_a_sweep(lib):
    rng = random.Random(21)
    widths = [8, 72, 136, 256, 512, 520, 768, 1024, 1280, 3072, 4096]
    Ms = [1, 63, 64, 65, 2047, 2048, 2049, 10837, 12800, 18464] + [rng.randrange(1, 40000) for _ in range(4)]
    groups = []
    for count in (1, 2, 3, 4, 5, 8, 13, 24, 35, 36):
        groups.append([(rng.choice(widths), rng.choice(widths)) for _ in range(count)])
        even = [w for w in widths if w % 256 == 0]                                 # a group the 256 x 256 kernels take
        groups.append([(rng.choice(even), rng.choice(even)) for _ in range(count)])
    forms = [L.TNKnobs()] + [knobs_of(env) for env in ENV_FORMS]
    points = 0
    for knobs in forms:
        for M in Ms:
            m_tiles = -(-M // 64)
            for shapes in groups:
                for splits in (0, 1, 3, m_tiles, m_tiles + 5):
                    for overwrite in (0, 1):
                        _check_preconditions(L.gemm_tn_plan(shapes, M, splits, overwrite, knobs), shapes, M, splits, overwrite, knobs)
                        points += 1
    assert points > 25000


def test_without_knobs_the_query_answers_for_the_process_environment(lib):
    import os
    env = knobs_of({name: os.environ[name] for name in KNOB_OF if name in os.environ})      # the defaults where none is set
    for shapes, M in [(block(768), 12800), (block(512), 11137), ([(520, 264)], 2048)]:
        assert bytes(L.gemm_tn_plan(shapes, M)) == bytes(L.gemm_tn_plan(shapes, M, knobs=env))


@pytest.mark.parametrize("n,width,M,queued,force,sizes", [
    (11, 768, 12800, 27, 0, [4, 7]),        # ViT-B/32 below the pruned block, whose in_proj is queued: 5 rounds
    (12, 768, 12800, 0, 0, [4, 8]),
    (12, 512, 11137, 0, 0, [4, 8]),
    (11, 512, 11137, 12, 0, [3, 8]),
    (24, 1024, 18464, 0, 0, [8, 8, 8]),
    (12, 768, 12800, 0, 5, [5, 7]),
    (3, 520, 4096, 0, 0, [3])])
def test_pinned_cuts(lib, n, width, M, queued, force, sizes):
    assert L.tower_wgrad_cuts(n, width, M, queued, force) == sizes


def test_cuts_cover_the_blocks_over_a_sweep(lib):
    for width, M in [(768, 12800), (512, 11137), (1024, 18464), (520, 4096), (768, 256), (136, 2048)]:
        for n in range(1, 65):
            for queued in (0, 3, 27, 48):
                for force in (0, 1, 5, 8, 9):
                    sizes = L.tower_wgrad_cuts(n, width, M, queued, force)
                    assert sum(sizes) == n and all(1 <= g <= 8 for g in sizes), (width, M, n, queued, force, sizes)
                    if force >= 1:                           # groups of `force` blocks (at most 8), the last one may differ
                        assert all(g == min(force, 8) for g in sizes[:-1]), (width, M, n, queued, force, sizes)


def test_queries_report_bad_arguments(lib):
    plan, knobs = L.TNPlan(), L.TNKnobs()
    one = (ctypes.c_int * 1)(256)
    zero = (ctypes.c_int * 1)(0)
    many = (ctypes.c_int * 37)(*[256] * 37)
    for args in [(0, one, one, 2048), (37, many, many, 2048), (1, one, one, 0), (1, zero, one, 2048), (1, one, zero, 2048),
                 (1, None, one, 2048)]:
        assert lib.ce_gemm_tn_plan(*args, 0, 0, ctypes.byref(knobs), ctypes.byref(plan)) == -22, args[0::3]
        assert b"ce_gemm_tn_plan" in lib.ce_last_error()
    assert lib.ce_gemm_tn_plan(1, one, one, 2048, 0, 0, None, None) == -22
    sizes = (ctypes.c_int * 64)()
    z = ctypes.c_long(0)
    for n, width, M, queued, out in [(0, 768, 12800, z, sizes), (65, 768, 12800, z, sizes), (12, 0, 12800, z, sizes),
                                     (12, 768, 0, z, sizes), (12, 768, 12800, ctypes.c_long(-1), sizes), (12, 768, 12800, z, None)]:
        assert lib.ce_tower_wgrad_cuts(n, width, M, queued, 0, out) == -22, (n, width, M)
        assert b"ce_tower_wgrad_cuts" in lib.ce_last_error()
