"""float64 oracle of gallery calibration (csrc/gallery_mated.hip, vn_celeb_face_recognition_amd/calibration.py): the mate /
non-mate selection over gallery_oracle.scores under (score descending, index ascending, NaN last), and the threshold,
FAR, DIR and per-class rules.  Written from the contract, in plain loops; no reference code exists for this feature."""
import math

import numpy as np

import gallery_oracle as go


def _before(s, i, best_s, best_i):
    """Is candidate (s, i) before the best so far under the total order?  best_i < 0: nothing yet."""
    if best_i < 0:
        return True
    a_nan, b_nan = math.isnan(s), math.isnan(best_s)
    if a_nan or b_nan:
        return (b_nan and not a_nan) or (a_nan and b_nan and i < best_i)
    return s > best_s or (s == best_s and i < best_i)


def mated(s, labels, qlabels, exclude=None):
    """(F,G) scores -> idx (F,2) int64, label (F,2) int64, score (F,2) float64: column 0 the best row of the probe's label
    other than exclude[f], column 1 the best row of another label; absent: -1, -1, -inf."""
    s = np.asarray(s, np.float64)
    f, g = s.shape
    idx = np.full((f, 2), -1, np.int64)
    lab = np.full((f, 2), -1, np.int64)
    sc = np.full((f, 2), -np.inf, np.float64)
    for p in range(f):
        for j in range(g):
            if labels[j] == qlabels[p]:
                if exclude is not None and exclude[p] == j:
                    continue
                col = 0
            else:
                col = 1
            if _before(float(s[p, j]), j, float(sc[p, col]), int(idx[p, col])):
                idx[p, col], lab[p, col], sc[p, col] = j, labels[j], s[p, j]
    return idx, lab, sc


def mated_search(q, g, labels, qlabels, exclude=None):
    return mated(go.scores(q, g), labels, qlabels, exclude)


def next32(x):
    return np.nextafter(np.float32(x), np.float32(np.inf))


def threshold(nonmate_scores, far):
    """next32 of the (floor(far n + 1e-9) + 1)-th largest score; -1.0 for no scores."""
    vals = sorted((float(v) for v in nonmate_scores), reverse=True)
    if not vals:
        return np.float32(-1.0)
    a = int(math.floor(far * len(vals) + 1e-9))
    return next32(np.float32(vals[a]))


def outranks(ms, mi, ns, ni):
    return mi >= 0 and (ni < 0 or _before(float(ms), int(mi), float(ns), int(ni)))


def calibrate(idx, label, score, probe_labels, far, num_classes):
    """-> dict(thr, Fm, Fn, far, dir, rank1, local) from (F,2) arrays, the scores taken as float32."""
    score = np.asarray(score, np.float32)
    f = len(probe_labels)
    non = [p for p in range(f) if idx[p, 1] >= 0]
    mat = [p for p in range(f) if idx[p, 0] >= 0]
    thr = threshold([score[p, 1] for p in non], far)
    local = {}
    for c in range(num_classes):
        mine = [score[p, 1] for p in non if label[p, 1] == c]
        local[str(c)] = float(max(threshold(mine, far), thr)) if mine else float(thr)
    passed = sum(1 for p in non if score[p, 1] >= thr)
    r1 = [p for p in mat if outranks(score[p, 0], idx[p, 0], score[p, 1], idx[p, 1])]
    det = [p for p in r1 if score[p, 0] >= np.float32(local[str(int(probe_labels[p]))])]
    return {"thr": float(thr), "Fm": len(mat), "Fn": len(non), "far": passed / len(non) if non else 0.0,
            "dir": len(det) / len(mat) if mat else None, "rank1": len(r1) / len(mat) if mat else None, "local": local}
