"""float64 oracle of the gallery clustering (vnf_gallery_cluster, csrc/gallery_cluster.hip), written from the contract in
include/vnface.h; no reference code exists for this feature.

    s = gallery_oracle.scores(rows, rows); N(i) = { j != i : s[i,j] >= t } (a NaN never); degree = |N(i)|
    core: degree + 1 >= min_samples; clusters: connected components of the core rows (union-find), numbered in ascending
    order of their smallest row; border: a non-core row with a core neighbour joins the best one's cluster under
    (score descending, index ascending) -- a stable argsort; everything else is noise, -1.

Exact equality with the device is only meaningful when no decision sits within rounding of a boundary, so the oracle also
returns the two margins a test asserts first: the smallest |s - t| over the off-diagonal pairs, and the smallest lead of
a border's best core neighbour over its best core neighbour in any OTHER cluster."""
import numpy as np

import gallery_oracle as go


class Result:
    pass


def _find(parent, x):
    while parent[x] != x:
        parent[x] = parent[parent[x]]
        x = parent[x]
    return x


def cluster_scores(s, t, min_samples):
    """(N,N) float64 scores -> Result with cluster, degree, core, border (bool), n_clusters, nn_idx, nn_score,
    margin_t, margin_border."""
    s = np.asarray(s, np.float64)
    n = s.shape[0]
    off = ~np.eye(n, dtype=bool)
    with np.errstate(invalid="ignore"):
        adj = (s >= t) & off
    res = Result()
    res.degree = adj.sum(axis=1).astype(np.int64)
    res.core = res.degree + 1 >= min_samples
    parent = list(range(n))
    for i in np.flatnonzero(res.core):
        for j in np.flatnonzero(adj[i] & res.core):
            a, b = _find(parent, int(i)), _find(parent, int(j))
            if a != b:
                parent[max(a, b)] = min(a, b)          # the root is the component's smallest row
    root = np.full(n, -1, np.int64)
    for i in np.flatnonzero(res.core):
        root[i] = _find(parent, int(i))
    res.border = np.zeros(n, bool)
    res.margin_border = np.inf
    key = np.where(np.isnan(s), np.inf, -s)
    for i in np.flatnonzero(~res.core):
        cand = np.flatnonzero(adj[i] & res.core)       # ascending, so a stable sort by -score breaks ties by index
        if cand.size == 0:
            continue
        best = cand[np.argsort(key[i, cand], kind="stable")[0]]
        res.border[i] = True
        root[i] = root[best]
        other = cand[root[cand] != root[best]]
        if other.size:
            res.margin_border = min(res.margin_border, float(s[i, best] - s[i, other].max()))
    roots = np.unique(root[root >= 0])                 # ascending smallest rows
    res.cluster = np.where(root >= 0, np.searchsorted(roots, root), -1).astype(np.int64)
    res.n_clusters = int(roots.size)
    d = np.abs(s - t)[off]
    d = d[~np.isnan(d)]
    res.margin_t = float(d.min()) if d.size else np.inf
    res.nn_idx = np.full(n, -1, np.int64)
    res.nn_score = np.full(n, -np.inf, np.float64)
    for i in range(n):
        others = np.delete(np.arange(n), i)
        if others.size:
            res.nn_idx[i] = others[np.argsort(key[i, others], kind="stable")[0]]     # NaN scores (key +inf) come last
            res.nn_score[i] = s[i, res.nn_idx[i]]
    return res


def cluster(rows, t, min_samples):
    return cluster_scores(go.scores(rows, rows), t, min_samples)


def check_nearest(nn_idx, nn_score, s, tol):
    """gallery_oracle.check_ranks' tolerant rule at k = 1 on the scores with each row's own column taken out: the score
    within tol of the oracle's best, the oracle's score of the returned row within tol of it too; (-1, -inf) when N == 1."""
    s = np.asarray(s, np.float64)
    n = s.shape[0]
    s_off = np.stack([np.delete(s[i], i) for i in range(n)]) if n else np.zeros((0, 0))
    idx = np.asarray(nn_idx, np.int64)
    assert n == 1 or (idx != np.arange(n)).all(), "a row is its own nearest neighbour"
    mapped = np.where(idx > np.arange(n), idx - 1, idx)
    return go.check_ranks(mapped[:, None], np.asarray(nn_score)[:, None], s_off, 1, tol)
