"""CPU (no GPU): the host side of the micro-batched train step and of the forward-only tower.

* ``ce_tower_infer_workspace_bytes``: the forward-only workspace does not grow with the number of blocks and is smaller
  than the training workspace of a ONE-block tower (by the layouts in csrc/tower.cpp: at most 30 x width bytes per row,
  fp8 scratch included, against one block's stash of 30 x width plus 162 x width of backward rings).
* argument errors of the new entry points and of the new epilogue are reported before any launch.
* ``GradSync.expect_passes``: with the forwards announced chunk by chunk, as ``engine.micro_batched_backward`` runs them,
  every element of the gradient buffer is exchanged exactly once per step, after its last write."""
import ctypes
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests.test_distributed_cpu import _FlatStandIn, _free_port

TOWERS = {"vit_b32": (768, 12, 50, 0), "text": (512, 8, 77, 1), "vit_l14_336": (1024, 16, 577, 0)}


def _desc(layers, width, heads, tokens, causal, stream16, fp8):
    from clip_event_amd.model import _BlockParams, _TowerDesc
    arr = (_BlockParams * layers)()
    d = _TowerDesc(layers, width, heads, tokens, causal, arr, fp8, stream16, 0, None)
    d._keep = arr
    return d


@pytest.mark.parametrize("fp8", [0, 3])
@pytest.mark.parametrize("stream16", [0, 1])
@pytest.mark.parametrize("tower", sorted(TOWERS))
def test_infer_workspace_is_independent_of_depth_and_below_one_block_of_stash(tower, stream16, fp8):
    from clip_event_amd._lib import lib
    cl = lib()
    cl.ce_tower_infer_workspace_bytes.restype = ctypes.c_size_t
    cl.ce_tower_workspace_bytes.restype = ctypes.c_size_t
    width, heads, tokens, causal = TOWERS[tower]
    for batch in (1, 8, 32):
        sizes = [int(cl.ce_tower_infer_workspace_bytes(ctypes.byref(_desc(layers, width, heads, tokens, causal, stream16, fp8)),
                                                       ctypes.c_int(batch))) for layers in (2, 24)]
        one_block = int(cl.ce_tower_workspace_bytes(ctypes.byref(_desc(1, width, heads, tokens, causal, stream16, fp8)), ctypes.c_int(batch)))
        full = int(cl.ce_tower_workspace_bytes(ctypes.byref(_desc(24, width, heads, tokens, causal, stream16, fp8)), ctypes.c_int(batch)))
        rows = batch * tokens
        print(f"[{tower} stream16={stream16} fp8={fp8} B={batch}] infer {sizes[0]} B = {sizes[0] / (rows * width):.1f} x width per row; "
              f"training: 1 block {one_block / (rows * width):.1f}, 24 blocks {full / (rows * width):.1f} x width per row")
        assert sizes[0] > 0 and sizes[0] == sizes[1]
        assert sizes[0] < one_block
        # the layout's own arithmetic: 2 stream buffers + h, qkv, o, g (18 bytes) per row and column, + 4 of fp8 scratch,
        # + per-row statistics / lse / the pruned block's compact buffers / alignment
        per_row = 2 * (2 if stream16 else 4) + 18 + (4 if fp8 else 0)
        assert sizes[0] >= rows * width * per_row
        assert sizes[0] <= rows * width * (per_row + 1) + batch * width * 32 + 64 * 1024


def test_new_entry_points_report_argument_errors_without_a_gpu():
    from clip_event_amd._lib import EPI_BIAS_QGELU_BF16, lib
    cl = lib()
    cl.ce_tower_infer_workspace_bytes.restype = ctypes.c_size_t
    c_long, c_int = ctypes.c_long, ctypes.c_int
    assert EPI_BIAS_QGELU_BF16 == 8
    assert cl.ce_tower_infer_workspace_bytes(None, c_int(4)) == 0
    assert b"null descriptor" in cl.ce_last_error()
    rc = cl.ce_tower_forward_infer(None, c_int(4), c_int(4), None, None, None, None, None, None)
    assert rc == -22 and b"null descriptor" in cl.ce_last_error()
    d = _desc(2, 128, 2, 10, 0, 1, 0)
    assert cl.ce_tower_infer_workspace_bytes(ctypes.byref(d), c_int(0)) == 0
    assert b"empty batch" in cl.ce_last_error()
    rc = cl.ce_tower_forward_infer(ctypes.byref(d), c_int(4), c_int(40), None, None, None, None, None, None)
    assert rc == -22 and b"ce_tower_forward_infer: null buffer" in cl.ce_last_error()
    rc = cl.ce_tower_forward_infer(ctypes.byref(d), c_int(4), c_int(39), None, None, None, None, None, None)
    assert rc == -22 and b"dense batch" in cl.ce_last_error()
    bad = _desc(2, 100, 2, 10, 0, 1, 0)
    assert cl.ce_tower_infer_workspace_bytes(ctypes.byref(bad), c_int(4)) == 0
    assert b"width" in cl.ce_last_error()
    # the forward-only QuickGELU epilogue needs its bias: refused before anything is launched (host memory is never touched)
    host = (ctypes.c_char * 4096)()
    p = ctypes.cast(host, ctypes.c_void_p)
    rc = cl.ce_gemm_nt(p, c_long(64), p, c_long(64), c_int(8), c_int(8), c_int(64), c_int(8), None, None, c_long(0), p,
                       c_long(8), None, c_long(0), None, c_long(0), None)
    assert rc == -22 and b"QuickGELU epilogue without bias" in cl.ce_last_error()
    rc = cl.ce_gemm_nt_fp8(p, c_long(128), p, p, c_long(128), p, c_int(8), c_int(8), c_int(128), c_int(8), None, None,
                           c_long(0), p, c_long(8), None, c_long(0), None, c_long(0), None)
    assert rc == -22 and b"QuickGELU epilogue without bias" in cl.ce_last_error()
    rc = cl.ce_gemm_nt(p, c_long(64), p, c_long(64), c_int(8), c_int(8), c_int(64), c_int(9), None, None, c_long(0), p,
                       c_long(8), None, c_long(0), None, c_long(0), None)
    assert rc == -22 and b"unknown epilogue" in cl.ce_last_error()


def test_profiler_classes_keep_their_ids_and_name_the_new_epilogue():
    from clip_event_amd._lib import lib
    cl = lib()
    cl.ce_profile_class_name.restype = ctypes.c_char_p
    assert cl.ce_profile_num_classes() == 80
    assert cl.ce_profile_class_name(64) in (b"gemm_tn3lw_kernel", b"gemm_tn3_kernel")
    assert cl.ce_profile_class_name(71) == b"gemm_tn2_kernel"
    assert cl.ce_profile_class_name(5 * 8 + 6) == b"gemm_nt160p_kernel<5,*> BIAS_GELU"
    assert cl.ce_profile_class_name(72 + 6) == b"gemm_nt160p_kernel<8,*> BIAS_QGELU_BF16"


# ---------------------------------------------------------------------------------------------------------------
# GradSync under the announcement order of a micro-batched step

CHUNKS = 3


def _chunked_worker(rank, W, port, auto_finish, sharded, out):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=W)
    from clip_event_amd import distributed as D
    m = _FlatStandIn(tail=4 if sharded else 3)
    sync = D.GradSync(m, pieces_per_tower=3, auto_finish=auto_finish, sharded=sharded)
    assert (sync.plan is not None) == sharded
    reduced = []
    inner = sync._reduce_range

    def counting(a, b, async_op):
        if b > a:
            reduced.append(b - a)
        return inner(a, b, async_op)

    sync._reduce_range = counting
    results = []
    for step in range(2):                     # two steps: the announcement must reset
        m._flat_grad.zero_()
        del reduced[:]
        g = torch.Generator().manual_seed(100 * step + rank)
        contrib = {t: [torch.randn(m._ranges[t][1] - m._ranges[t][0], generator=g) for _ in range(CHUNKS)] for t in ("visual", "text")}
        sync.expect_passes({"visual": CHUNKS, "text": CHUNKS})
        m._flat_grad[0] += float(rank + 1)     # logit_scale: written by the head's backward, before any tower backward
        cuts_seen = {"visual": [], "text": []}
        for k in range(CHUNKS):
            for t in ("visual", "text"):       # this chunk's forward is announced ...
                sync.note_forward(t)
            for t in ("text", "visual"):       # ... and its backward runs before the next chunk is announced
                cuts_seen[t].append(len(sync.layer_cuts(t, m.LAYERS)))
                m.backward_pass(t, contrib[t][k])
            if auto_finish:                    # where autograd's final callback fires: at the end of this chunk's backward()
                sync._finish_callback()
            if k + 1 < CHUNKS:
                assert not reduced, f"exchange before the last chunk (chunk {k}): {reduced}"
        sync.finish()                          # the engine's explicit call; a no-op when the callback has done it
        assert not sync.dirty and not sync.pending and not sync.announced
        for t in ("visual", "text"):
            assert cuts_seen[t] == [0] * (CHUNKS - 1) + [2], cuts_seen
        assert sum(reduced) == m._flat_grad.numel(), (reduced, m._flat_grad.numel())
        results.append((m._flat_grad.clone(), {t: torch.stack(contrib[t]).sum(0) for t in contrib}))
    gathered = [None] * W
    dist.all_gather_object(gathered, results)
    if rank == 0:
        torch.save(gathered, out)
    dist.destroy_process_group()


@pytest.mark.timeout(120)
@pytest.mark.parametrize("sharded", [False, True])
@pytest.mark.parametrize("auto_finish", [True, False])
def test_gradsync_interleaved_chunks_exchange_once_after_the_last(tmp_path, auto_finish, sharded):
    """Three chunks whose forwards are announced one by one (forward, backward, next forward ...): every element ends as
    the rank mean of the summed contributions, only the last chunk's backward is cut into eager pieces, and the elements
    handed to ``_reduce_range`` over the step add up to the buffer length once.  Counting announcements alone takes the
    FIRST chunk for the last pass (off by 2.4 from the mean here)."""
    W = 2
    out = str(tmp_path / "g.pt")
    mp.spawn(_chunked_worker, args=(W, _free_port(), auto_finish, sharded, out), nprocs=W, join=True)
    gathered = torch.load(out, weights_only=False)          # written by this test
    m = _FlatStandIn(tail=4 if sharded else 3)
    for step in range(2):
        want = torch.zeros_like(m._flat_grad)
        for r in range(W):
            tot = gathered[r][step][1]
            for t in ("visual", "text"):
                a, b = m._ranges[t]
                want[a:b] += tot[t] / W
            want[0] += (r + 1) / W
        for r in range(W):
            err = float((gathered[r][step][0] - want).abs().max())
            print(f"[auto_finish={auto_finish} sharded={sharded}] step {step} rank {r}: max |got - mean of sums| = {err:.3e}")
            assert torch.allclose(gathered[r][step][0], want, atol=1e-6), (step, r)


def test_expect_passes_is_validated_and_reset():
    from clip_event_amd import distributed as D
    m = _FlatStandIn()
    sync = D.GradSync(m)
    with pytest.raises(ValueError):
        sync.expect_passes({"head": 2})
    with pytest.raises(ValueError):
        sync.expect_passes({"visual": 0})
    sync.expect_passes({"visual": 2})
    assert not sync._is_last_pass("visual") and sync._passes_outstanding()
    sync.finish()                              # no process group: nothing to exchange, bookkeeping reset
    assert sync.announced == {} and not sync._passes_outstanding()


def test_train_step_signature_and_refusals():
    """``micro_batch`` is an argument of ``train_step``; with ``train_arg`` / ``criterion_ot`` a chunking value is refused
    before anything runs (no GPU needed to say so)."""
    import inspect
    from clip_event_amd import engine

    class _M(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.zeros(1))
            self.alignment = False

    p = inspect.signature(engine.train_step).parameters["micro_batch"]
    assert p.default is None
    img, txt = torch.zeros(4, 3, 8, 8), torch.zeros(4, 5, dtype=torch.long)
    with pytest.raises(NotImplementedError, match="micro_batch"):
        engine.train_step(_M(), None, None, img, txt, None, None, None, train_arg=object(), micro_batch=2)
    with pytest.raises(NotImplementedError, match="micro_batch"):
        engine.train_step(_M(), None, None, img, txt, None, None, None, criterion_ot=object(), micro_batch=2)
