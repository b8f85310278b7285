"""GPU: ``ce_score_topk`` (retrieval.hip) against the fp64 reference of tests/retrieval_ref.py.

* exact case: features with entries in {-1, 0, 1}, no logit scale -- every dot product is an integer below 2^24, so fp32
  is exact and ``top_idx`` / ``top_val`` / ``rank`` must equal the reference with no tolerance; the many natural ties (and
  a few duplicated key rows) exercise the index rule.
* real-valued case: normalised Gaussian features, ``logit_scale = ln(1 / 0.07)``; tol = s (E + 2) 2^-24 is the worst-case
  bound of an fp32 dot product of unit vectors plus the scaling.
* ``splits`` changes nothing in ``top_val`` / ``top_idx`` / ``rank``."""
import math

import numpy as np
import pytest
import torch

from tests import retrieval_ref as RR

pytestmark = pytest.mark.gpu

DEV = "cuda:0"

EXACT_CASES = [(5, 7, 128, 1, 0), (37, 333, 128, 5, 0), (33, 1000, 512, 10, 3), (64, 96, 768, 16, 1), (70, 40, 256, 16, 7),
               (3, 9, 1024, 16, 0)]
REAL_CASES = [(37, 333, 128, 5), (33, 1000, 512, 10), (40, 96, 768, 16)]


def _run(q, keys, k, logit_scale=None, target=None, splits=0):
    from clip_event_amd import ops
    ls = None if logit_scale is None else torch.tensor([logit_scale], dtype=torch.float32, device=DEV)
    tg = None if target is None else torch.from_numpy(np.asarray(target, dtype=np.int64)).to(DEV)
    val, idx, lse, rank = ops.score_topk(torch.from_numpy(q).to(DEV), torch.from_numpy(keys).to(DEV), k, logit_scale=ls,
                                         target=tg, splits=splits)
    torch.cuda.synchronize()
    return (val.cpu().numpy(), idx.cpu().numpy(), lse.cpu().numpy(), None if rank is None else rank.cpu().numpy())


def _targets(ref_order, nq, nk, k, rng):
    """Target vectors that together put every kind on some query: key 0, key nk-1, a key inside the top-k, one outside
    (where nk > k), -1 and an out-of-range index; the other queries get random keys.  Several vectors where nq < 6."""
    vectors = []
    for shift in range(0, 6, min(nq, 6)):
        t = rng.integers(0, nk, size=nq)
        for r in range(nq):
            kind = r + shift
            if kind == 0:
                t[r] = 0
            elif kind == 1:
                t[r] = nk - 1
            elif kind == 2:
                t[r] = ref_order[r, (min(k, nk) - 1) // 2]
            elif kind == 3 and nk > k:
                t[r] = ref_order[r, k + (nk - k) // 2]
            elif kind == 4:
                t[r] = -1
            elif kind == 5:
                t[r] = nk + 3
        vectors.append(t)
    return vectors


@pytest.mark.parametrize("nq,nk,E,k,splits", EXACT_CASES)
def test_score_topk_exact(nq, nk, E, k, splits):
    rng = np.random.default_rng(nq * 1000 + nk)
    q = rng.integers(-1, 2, size=(nq, E)).astype(np.float32)
    keys = rng.integers(-1, 2, size=(nk, E)).astype(np.float32)
    for dst, src in ((nk - 1, 0), (nk // 2, 1), (2, nk - 2)):            # duplicated key rows: exact ties, index decides
        keys[dst] = keys[src]
    order = RR.order_of(RR.scores64(q, keys))
    for target in _targets(order, nq, nk, k, rng):
        ref = RR.reference(q, keys, k, target=target)
        val, idx, lse, rank = _run(q, keys, k, target=target, splits=splits)
        ties = sum(len(row) - len(set(row)) for row in ref.scores.tolist())
        print(f"[exact {nq}x{nk} E={E} k={k} splits={splits}] tied scores {ties}; idx mismatches {int((idx != ref.top_idx).sum())}; "
              f"val mismatches {int((val != ref.top_val).sum())}; rank mismatches {int((rank != ref.rank).sum())}; "
              f"max lse err {float(np.abs(lse - ref.lse).max()):.3e}")
        assert np.array_equal(idx, ref.top_idx)
        assert np.array_equal(val.astype(np.float64), ref.top_val)
        assert np.array_equal(rank, ref.rank)
        assert np.all(np.abs(lse - ref.lse) <= 1e-5 * np.maximum(1.0, np.abs(ref.lse)))
        for r in range(nq):
            if 0 <= rank[r] < k:
                assert idx[r, rank[r]] == target[r]


def _real_inputs(nq, nk, E):
    rng = np.random.default_rng(nq + nk + E)
    q = rng.standard_normal((nq, E))
    keys = rng.standard_normal((nk, E))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    keys /= np.linalg.norm(keys, axis=1, keepdims=True)
    target = rng.integers(0, nk, size=nq)
    target[0], target[1], target[2], target[3] = 0, nk - 1, -1, nk
    return q.astype(np.float32), keys.astype(np.float32), target


@pytest.mark.parametrize("nq,nk,E,k", REAL_CASES)
def test_score_topk_real_valued(nq, nk, E, k):
    ls = float(np.float32(math.log(1 / 0.07)))
    q, keys, target = _real_inputs(nq, nk, E)
    ref = RR.reference(q, keys, k, logit_scale=ls, target=target)
    target[4] = ref.order[4, k // 2]                      # one target inside the top-k
    ref = RR.reference(q, keys, k, logit_scale=ls, target=target)
    val, idx, lse, rank = _run(q, keys, k, logit_scale=ls, target=target)
    tol = math.exp(ls) * (E + 2) * 2.0 ** -24
    own = np.take_along_axis(ref.scores, idx, axis=1)
    lo, hi = RR.rank_bounds(ref.scores, target, 2 * tol)
    print(f"[real {nq}x{nk} E={E} k={k}] tol {tol:.3e}; max |val - fp64 score of its idx| {float(np.abs(val - own).max()):.3e}; "
          f"idx that differ from the fp64 order {int((idx != ref.top_idx).sum())}; ranks that differ {int((rank != ref.rank).sum())}; "
          f"max lse err {float(np.abs(lse - ref.lse).max()):.3e}")
    assert idx.min() >= 0 and idx.max() < nk
    assert np.all(np.abs(val - own) <= tol)
    assert all(len(set(row)) == k for row in idx.tolist())
    assert np.all(val[:, 1:] <= val[:, :-1])
    assert np.all(own >= ref.top_val[:, k - 1:k] - 2 * tol)
    assert np.all((lo <= rank) & (rank <= hi))
    assert rank[2] == -1 and rank[3] == -1
    assert np.all(np.abs(lse - ref.lse) <= 1e-5 * np.maximum(1.0, np.abs(ref.lse)))
    for r in range(nq):
        if 0 <= rank[r] < k:
            assert idx[r, rank[r]] == target[r]
    assert 0 <= rank[4] < k


def test_score_topk_does_not_depend_on_splits():
    nq, nk, E, k = 33, 1000, 512, 10
    ls = float(np.float32(math.log(1 / 0.07)))
    q, keys, target = _real_inputs(nq, nk, E)
    keys[nk - 1] = keys[5]
    runs = [_run(q, keys, k, logit_scale=ls, target=target, splits=s) for s in (1, 3, 7)]
    for val, idx, lse, rank in runs[1:]:
        assert np.array_equal(val.view(np.int32), runs[0][0].view(np.int32))
        assert np.array_equal(idx, runs[0][1])
        assert np.array_equal(rank, runs[0][3])
        assert np.allclose(lse, runs[0][2], rtol=1e-5, atol=1e-5)
