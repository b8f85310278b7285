"""fp64 reference of ``ce_score_topk`` (include/clip_event_hip.h): scores, the (score descending, key index ascending)
order, top-k with padding, log-sum-exp and the rank of a target.  numpy only."""
from typing import NamedTuple, Optional

import numpy as np


class Ref(NamedTuple):
    scores: np.ndarray            # [nq, nk] f64
    order: np.ndarray             # [nq, nk] key indices, best first
    top_val: np.ndarray           # [nq, k] f64, -inf past nk
    top_idx: np.ndarray           # [nq, k] int64, -1 past nk
    lse: np.ndarray               # [nq] f64
    rank: Optional[np.ndarray]    # [nq] int64, -1 for a target outside 0..nk-1


def scores64(q, keys, logit_scale=None) -> np.ndarray:
    s = 1.0 if logit_scale is None else float(np.exp(np.float64(logit_scale)))
    return s * (np.asarray(q, dtype=np.float64) @ np.asarray(keys, dtype=np.float64).T)


def order_of(scores: np.ndarray) -> np.ndarray:
    """Per row: key indices sorted by score descending, ties by index ascending (a total order)."""
    nq, nk = scores.shape
    idx = np.arange(nk)
    return np.stack([np.lexsort((idx, -scores[r])) for r in range(nq)])          # lexsort: the LAST key is the primary one


def reference(q, keys, k: int, logit_scale=None, target=None) -> Ref:
    S = scores64(q, keys, logit_scale)
    nq, nk = S.shape
    order = order_of(S)
    top_idx = np.full((nq, k), -1, dtype=np.int64)
    top_val = np.full((nq, k), -np.inf)
    n = min(k, nk)
    top_idx[:, :n] = order[:, :n]
    top_val[:, :n] = np.take_along_axis(S, order[:, :n], axis=1)
    m = S.max(axis=1)
    lse = m + np.log(np.exp(S - m[:, None]).sum(axis=1))
    rank = None
    if target is not None:
        target = np.asarray(target, dtype=np.int64)
        rank = np.full(nq, -1, dtype=np.int64)
        for r in range(nq):
            if 0 <= target[r] < nk:
                rank[r] = int(np.nonzero(order[r] == target[r])[0][0])
    return Ref(S, order, top_val, top_idx, lse, rank)


def rank_bounds(scores: np.ndarray, target, band: float):
    """``(lo, hi)`` per query: every rank an implementation whose scores are within ``band / 2`` of ``scores`` may report
    for ``target``: lo = #{c : S_c > S_t + band}, hi = #{c != t : S_c >= S_t - band}; (-1, -1) for a target outside 0..nk-1."""
    nq, nk = scores.shape
    target = np.asarray(target, dtype=np.int64)
    lo = np.full(nq, -1, dtype=np.int64)
    hi = np.full(nq, -1, dtype=np.int64)
    for r in range(nq):
        t = target[r]
        if 0 <= t < nk:
            st = scores[r, t]
            lo[r] = int((scores[r] > st + band).sum())
            hi[r] = int((scores[r] >= st - band).sum()) - 1          # the target itself is always in that set
    return lo, hi
