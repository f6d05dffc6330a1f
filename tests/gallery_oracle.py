"""float64 oracle of the gallery search (vn_celeb_face_recognition_amd/gallery.py, csrc/gallery.hip): normalise with
F.normalize's rule, q^ @ g^T, then a stable sort by (-score, index) with NaN scores last.  Written from the contract;
no reference code exists for this feature."""
import numpy as np

EPS = 1e-12


def tol(dim):
    """An fp32 dot of `dim` products of unit vectors (sum |q_i g_i| <= 1) plus the two normalisations: about
    (dim + 4) 2^-23 absolute.  6.2e-5 at dim 512."""
    return (dim + 4) * 2.0 ** -23


def normalize(x):
    x = np.asarray(x, np.float64)
    n = np.sqrt((x * x).sum(axis=1, keepdims=True))
    return x / np.maximum(n, EPS)      # a NaN norm stays NaN, as torch's clamp_min leaves it


def scores(q, g):
    """(F,dim), (G,dim) of any norm -> (F,G) float64 cosines."""
    with np.errstate(invalid="ignore"):
        return normalize(q) @ normalize(g).T


def topk(s, labels, k):
    """(F,G) scores -> idx (F,k) int64, label (F,k) int64, score (F,k) float64 under (score descending, index ascending),
    NaN below every number; slots beyond G hold -1, -1, -inf."""
    s = np.asarray(s, np.float64)
    f, g = s.shape
    idx = np.full((f, k), -1, np.int64)
    lab = np.full((f, k), -1, np.int64)
    sc = np.full((f, k), -np.inf, np.float64)
    labels = np.asarray(labels, np.int64)
    for i in range(f):
        row = s[i]
        key = np.where(np.isnan(row), np.inf, -row)          # NaN last; -0.0 and 0.0 compare equal
        order = np.argsort(key, kind="stable")
        nan = np.isnan(row[order])
        order = np.concatenate([order[~nan], order[nan]])     # +inf keys of real -inf scores cannot occur for finite rows
        m = min(k, g)
        idx[i, :m] = order[:m]
        lab[i, :m] = labels[order[:m]]
        sc[i, :m] = row[order[:m]]
    return idx, lab, sc


def search(q, g, labels, k):
    return topk(scores(q, g), labels, k)


def check_ranks(idx, score, s64, k, t):
    """The tolerant rank comparison: at each rank r, |score_r - oracle_score_r| <= t, and the oracle's float64 score of
    the returned index is >= oracle_score_r - t.  Slots beyond G must be (-1, -inf) exactly.  Returns the largest
    |score - oracle score| seen."""
    f, g = s64.shape
    oi, _, osc = topk(s64, np.zeros((g,), np.int64), k)
    worst = 0.0
    for i in range(f):
        seen = set()
        for r in range(k):
            if r >= g:
                assert idx[i, r] == -1 and score[i, r] == -np.inf, (i, r, idx[i, r], score[i, r])
                continue
            j = int(idx[i, r])
            assert 0 <= j < g and j not in seen, (i, r, j)
            seen.add(j)
            if np.isnan(osc[i, r]):
                assert np.isnan(score[i, r]), (i, r, score[i, r])
                continue
            err = abs(float(score[i, r]) - osc[i, r])
            worst = max(worst, err)
            assert err <= t, (i, r, float(score[i, r]), osc[i, r])
            assert s64[i, j] >= osc[i, r] - t, (i, r, j, s64[i, j], osc[i, r])
    return worst


def class_sums(rows, labels, classes):
    """float64 sums of the normalised rows per class of `classes` (ascending), and their counts."""
    n = normalize(rows)
    labels = np.asarray(labels, np.int64)
    sums = np.stack([n[labels == c].sum(axis=0) for c in classes]) if len(classes) else np.zeros((0, n.shape[1]))
    counts = np.array([(labels == c).sum() for c in classes], np.int64)
    return sums, counts
