"""Rank fusion of the hit lists of several retrievers (host only, no GPU): reciprocal rank fusion.

``rrf(rankings)`` fuses id lists; ``fuse_hits(*results)`` fuses the per-query ``(ids, scores)`` lists that ``Indexer.search_knn``, ``SparseIndexer.search_knn``,
``SpladeModel.retrieve`` and ``BGEM3Model.retrieve`` return — only the order of each list enters, so retrievers whose scores live on different scales (a
cosine, a lexical matching score) meet without a normalisation.

Definition.  With systems ``s = 0, 1, ...`` in the order given, weights ``w_s`` (1 when not given) and ``rank_s(id)`` the 1-based position of ``id`` in system
``s``'s list,

    score(id) = sum over the systems that list id, in system order, of  w_s / (k + rank_s(id))          (float64, summed in that order)

and the result is ordered by (score descending, best rank over the systems ascending, index of the first system that gives that best rank ascending).  One
system gives one rank to one id, so the order is total.
"""
from __future__ import annotations

import math
from typing import List, Optional, Sequence, Tuple

import numpy as np


def rrf(rankings: Sequence[Sequence], k: float = 60.0, weights: Optional[Sequence[float]] = None, top_k: Optional[int] = None) -> Tuple[list, np.ndarray]:
    """``(ids, float64 scores)`` of the fused ranking, the best ``top_k`` (all when ``None``).  ``rankings``: one id list per system, best first; ids are any
    hashable values and come back as given.  ``ValueError``: an id twice in one ranking, ``k <= 0`` (or NaN / Inf), a weight that is negative, NaN or Inf, a
    weight count other than the number of systems."""
    rankings = [list(r) for r in rankings]
    k = float(k)
    if not (k > 0.0) or math.isinf(k):
        raise ValueError(f"k={k}: a finite number > 0")
    if weights is None:
        weights = [1.0] * len(rankings)
    weights = [float(w) for w in weights]
    if len(weights) != len(rankings):
        raise ValueError(f"{len(weights)} weights for {len(rankings)} rankings")
    for s, w in enumerate(weights):
        if not (w >= 0.0) or math.isinf(w):
            raise ValueError(f"weights[{s}]={w}: finite and >= 0")
    score, best = {}, {}             # id -> float64 sum; id -> (best rank, first system giving it)
    for s, ranking in enumerate(rankings):
        seen = set()
        for rank, i in enumerate(ranking, start=1):
            if i in seen:
                raise ValueError(f"rankings[{s}]: id {i!r} occurs twice")
            seen.add(i)
            score[i] = score.get(i, 0.0) + weights[s] / (k + rank)
            if i not in best or rank < best[i][0]:
                best[i] = (rank, s)
    order = sorted(score, key=lambda i: (-score[i], best[i][0], best[i][1]))
    if top_k is not None:
        order = order[:max(int(top_k), 0)]
    return order, np.array([score[i] for i in order], np.float64)


def fuse_hits(*results, k: float = 60.0, weights: Optional[Sequence[float]] = None, top_k: Optional[int] = 10) -> List[Tuple[list, np.ndarray]]:
    """Each ``result``: a per-query list of ``(ids, scores)`` of one retriever, best first (the scores are not read).  Per query ``(ids, float32 scores)`` of
    ``rrf`` over the systems' id lists.  ``ValueError`` when the results do not hold the same number of queries."""
    if not results:
        raise ValueError("fuse_hits: at least one result")
    results = [list(r) for r in results]
    nq = len(results[0])
    for s, r in enumerate(results):
        if len(r) != nq:
            raise ValueError(f"results[{s}] holds {len(r)} queries, results[0] holds {nq}")
    out = []
    for q in range(nq):
        ids, scores = rrf([list(r[q][0]) for r in results], k=k, weights=weights, top_k=top_k)
        out.append((ids, scores.astype(np.float32)))
    return out
