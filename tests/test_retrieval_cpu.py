"""CPU: the host side of scoring without the logits matrix -- the fp64 reference the GPU tests compare against, the metrics,
argument validation of ``ce_score_topk`` and its workspace size."""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests import retrieval_ref as RR


def test_reference_tie_rule_and_padding_against_a_python_sort():
    """4 x 9 with repeated scores (duplicated key rows and small integer entries): the reference's order is the brute-force
    ``sorted`` by (-score, index); k = 12 > nk pads with -inf / -1."""
    rng = np.random.default_rng(0)
    q = rng.integers(-1, 2, size=(4, 6)).astype(np.float32)
    keys = rng.integers(-1, 2, size=(9, 6)).astype(np.float32)
    keys[5] = keys[1]
    keys[8] = keys[1]
    keys[7] = keys[2]
    target = np.array([8, 0, -1, 9])
    S = RR.scores64(q, keys)
    assert any(len(set(row)) < 9 for row in S.tolist()), "the case has no ties"
    for k in (1, 3, 9, 12):
        ref = RR.reference(q, keys, k, target=target)
        for r in range(4):
            brute = sorted(range(9), key=lambda c: (-S[r, c], c))
            assert ref.order[r].tolist() == brute
            n = min(k, 9)
            assert ref.top_idx[r, :n].tolist() == brute[:n] and ref.top_idx[r, n:].tolist() == [-1] * (k - n)
            assert ref.top_val[r, :n].tolist() == [S[r, c] for c in brute[:n]]
            assert all(v == -math.inf for v in ref.top_val[r, n:])
            want = brute.index(target[r]) if 0 <= target[r] < 9 else -1
            assert ref.rank[r] == want
            assert abs(ref.lse[r] - math.log(sum(math.exp(v) for v in S[r]))) < 1e-12
    # keys 5 and 8 are copies of key 1: for every query the copies come lowest index first
    for r in range(4):
        pos = {c: RR.reference(q, keys, 9).order[r].tolist().index(c) for c in (1, 5, 8)}
        assert pos[1] < pos[5] < pos[8]
    lo, hi = RR.rank_bounds(S, target, 0.0)
    ref = RR.reference(q, keys, 1, target=target)
    assert all(lo[r] <= ref.rank[r] <= hi[r] for r in range(4)) and lo[2] == hi[2] == -1 and lo[3] == hi[3] == -1


def test_metrics_from_ranks_against_numpy():
    from clip_event_amd.inference import metrics_from_ranks
    rng = np.random.default_rng(1)
    rank = rng.integers(0, 40, size=101)
    rank[::7] = -1
    got = metrics_from_ranks(torch.from_numpy(rank), ks=(1, 5, 10))
    valid = rank[rank >= 0]
    assert got["n"] == len(valid)
    for k in (1, 5, 10):
        assert got[f"R@{k}"] == pytest.approx(float((valid < k).mean()), abs=1e-12)
    assert got["median_rank"] == pytest.approx(float(np.median(valid + 1)), abs=1e-12)
    assert got["mean_rank"] == pytest.approx(float((valid + 1).mean()), abs=1e-12)
    even = metrics_from_ranks(torch.tensor([0, 3, 9, 4]), ks=(5,))            # even count: the median is the mean of the middle two
    assert even == {"R@5": 0.75, "median_rank": 4.5, "mean_rank": 5.0, "n": 4}
    for empty in (torch.tensor([], dtype=torch.int64), torch.tensor([-1, -1])):
        out = metrics_from_ranks(empty)
        assert out["n"] == 0 and set(out) == {"R@1", "R@5", "R@10", "median_rank", "mean_rank", "n"}
        assert all(math.isnan(out[key]) for key in out if key != "n")


def _call(cl, *, nq=8, nk=8, E=128, k=1, splits=0, q=64, keys=64, target=0, top_val=64, top_idx=64, lse=0, rank=0, ws=64):
    P = ctypes.c_void_p                     # never dereferenced: validation comes before any launch
    return cl.ce_score_topk(P(q), ctypes.c_long(E), nq, P(keys), ctypes.c_long(E), nk, E, None, P(target), k, splits, P(top_val),
                            P(top_idx), P(lse), P(rank), P(ws), None)


@pytest.mark.parametrize("kwargs,message", [
    (dict(k=0), b"k must be in 1..16"), (dict(k=17), b"k must be in 1..16"),
    (dict(E=64), b"E must be a multiple of 128"), (dict(E=192), b"E must be a multiple of 128"),
    (dict(E=1152), b"E must be a multiple of 128"),
    (dict(nq=0), b"empty problem"), (dict(nk=0), b"empty problem"),
    (dict(top_val=0), b"null output"), (dict(top_idx=0), b"null output"),
    (dict(rank=64), b"rank needs target"),
    (dict(splits=65), b"splits must be"),
])
def test_score_topk_argument_errors_are_reported_without_a_gpu(kwargs, message):
    from clip_event_amd._lib import lib
    cl = lib()
    assert _call(cl, **kwargs) == -22
    assert message in cl.ce_last_error()


def test_score_topk_workspace_grows_with_the_problem():
    from clip_event_amd._lib import lib
    fn = lib().ce_score_topk_workspace_bytes
    fn.restype = ctypes.c_size_t
    for splits in (0, 1, 3, 64):
        for k in (1, 5, 16):
            sizes = [int(fn(nq, 50000, k, splits)) for nq in (1, 31, 32, 33, 256, 300, 352, 1000, 8192, 50000)]
            assert sizes[0] > 0 and sizes == sorted(sizes), (splits, k, sizes)
    for nq in (1, 300, 50000):
        by_k = [int(fn(nq, 50000, k, 0)) for k in range(1, 17)]
        assert by_k[0] > 0 and by_k == sorted(by_k)
        by_s = [int(fn(nq, 50000, 5, s)) for s in range(1, 65)]
        assert by_s[0] > 0 and by_s == sorted(by_s)
    # the launcher's own choice (splits = 0) stays far below the matrix it replaces
    assert int(fn(50000, 50000, 10, 0)) < 50000 * 50000 * 4 // 100
