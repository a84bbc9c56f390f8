"""fp64 numpy restatement of the neighbour search (imt_knn_rows) and of the mining rules (imagetranslate_amd/mine_pairs.py),
written from the rules' text with plain loops: test infrastructure, nothing here is shared with the code under test."""
import numpy as np


def knn_from_sim(sim, k):
    """(val [N, k] fp64, idx [N, k] int64) of a full similarity matrix: by value descending, then index ascending (a stable
    argsort of the negated row); places past the M columns hold -inf / -1."""
    sim = np.asarray(sim, dtype=np.float64)
    N, M = sim.shape
    val = np.full((N, k), -np.inf)
    idx = np.full((N, k), -1, dtype=np.int64)
    order = np.argsort(-sim, axis=1, kind="stable")[:, :k]
    n = order.shape[1]
    idx[:, :n] = order
    val[:, :n] = np.take_along_axis(sim, order, axis=1)
    return val, idx


def similarities(x, y):
    """The full [N, M] matrix in fp64 from the given values."""
    return np.asarray(x, dtype=np.float64) @ np.asarray(y, dtype=np.float64).T


def knn_reference(x, y, k):
    return knn_from_sim(similarities(x, y), k)


def rule_scores(sim, k, margin):
    """(score [N, M] fp64 of every pair under the rule, candidate mask of the forward lists [N, M], of the backward lists [N, M]).
    margin "none": the score is the cosine and only the first neighbour is a candidate.  margin "ratio": cos / ((a(s) + b(t)) / 2)
    with a, b the mean similarity to the min(k, other side) nearest neighbours; a pair whose denominator is <= 1e-6 is no
    candidate; the k neighbours of either list are the candidates."""
    sim = np.asarray(sim, dtype=np.float64)
    N, M = sim.shape
    fv, fi = knn_from_sim(sim, k)
    bv, bi = knn_from_sim(sim.T, k)
    fwd = np.zeros((N, M), dtype=bool)
    bwd = np.zeros((N, M), dtype=bool)
    if margin == "none":
        for s in range(N):
            fwd[s, fi[s, 0]] = True
        for t in range(M):
            bwd[bi[t, 0], t] = True
        return sim.copy(), fwd, bwd
    assert margin == "ratio"
    a = fv[:, :min(k, M)].mean(axis=1)
    b = bv[:, :min(k, N)].mean(axis=1)
    den = (a[:, None] + b[None, :]) / 2
    ok = den > 1e-6
    score = np.where(ok, sim / np.where(ok, den, 1.0), -np.inf)
    for s in range(N):
        for t in fi[s]:
            if t >= 0 and ok[s, t]:
                fwd[s, t] = True
    for t in range(M):
        for s in bi[t]:
            if s >= 0 and ok[s, t]:
                bwd[s, t] = True
    return score, fwd, bwd


def mine_reference(sim, k, margin, min_score):
    """[(s, t, score)] kept by the rule, by score descending, then (s, t) ascending.  s's best: the highest-scoring of its forward
    candidates, ties to the lowest t; t's best likewise, ties to the lowest s; keep (s, t) iff each is the other's best and
    score >= min_score."""
    score, fwd, bwd = rule_scores(sim, k, margin)
    N, M = score.shape

    def best(cands, scores):
        top, at = None, -1
        for j in cands:                      # ascending index: the first of equal scores stays
            if top is None or scores[j] > top:
                top, at = scores[j], j
        return at

    s_best = [best(np.flatnonzero(fwd[s]), score[s]) for s in range(N)]
    t_best = [best(np.flatnonzero(bwd[:, t]), score[:, t]) for t in range(M)]
    out = []
    for s in range(N):
        t = s_best[s]
        if t >= 0 and t_best[t] == s and score[s, t] >= min_score:
            out.append((s, int(t), float(score[s, t])))
    out.sort(key=lambda r: (-r[2], r[0], r[1]))
    return out
