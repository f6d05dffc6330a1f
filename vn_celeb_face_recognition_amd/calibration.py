"""Gallery calibration: where "Unknown" begins (calibrate.py).  Host code: NumPy on the 2F scores of
GalleryModel.mated_search, no device work.

Per probe p of known label: the mate score m_p (its best cosine against rows of its own label) and the non-mate score n_p
(its best against every other label: what the face would score if its owner were not enrolled), both float32.  Fn probes
have a non-mate, Fm have a mate.  A face is accepted iff score >= threshold (pipeline.identify_names), so for a target
false-accept rate `far` in [0, 1)

    a   = floor(far * Fn + 1e-9)                        impostor probes that may pass
    thr = next32((a + 1)-th largest n_p)                the smallest float32 above it: #{n_p >= thr} <= a, ties included

and Fn == 0 gives thr = -1.0 (every cosine passes; the report says so).  The threshold of class c applies the same rule
to the non-mate scores whose non-mate LABEL is c -- the strangers c attracted -- and is never below thr; a class that
attracted nobody gets thr.

"Outranks" is the search's total order: score descending, then row index ascending; NaN below every number (scores are
finite when the probes are, and calibrate.py refuses probes that are not)."""
import json

import numpy as np

FAR_POINTS = (0.1, 0.01, 0.001)


def next32(x):
    """The smallest float32 above x."""
    return np.nextafter(np.float32(x), np.float32(np.inf))


def check_far(far):
    far = float(far)
    if not 0.0 <= far < 1.0:      # a NaN fails both
        raise ValueError("far must lie in [0, 1), got %r" % (far,))
    return far


def accepted_impostors(n, far):
    """a = floor(far * n + 1e-9): the 1e-9 keeps a product that is an integer in exact arithmetic (0.01 * 300) on it."""
    return int(np.floor(far * n + 1e-9))


def threshold_at_far(nonmate_scores, far):
    """float32 threshold of the rule above for these non-mate scores; -1.0 when there are none."""
    far = check_far(far)
    s = np.asarray(nonmate_scores, np.float32).reshape(-1)
    if s.size == 0:
        return np.float32(-1.0)
    s = np.sort(np.where(np.isnan(s), np.float32(-np.inf), s))[::-1]
    a = min(accepted_impostors(s.size, far), s.size - 1)
    return next32(s[a])


def _outranks(ms, mi, ns, ni):
    """mate (score, idx) before non-mate (score, idx) under the key order; an absent one (idx < 0) is last."""
    ms = np.where(np.isnan(ms), -np.inf, ms)
    ns = np.where(np.isnan(ns), -np.inf, ns)
    return (mi >= 0) & ((ni < 0) | (ms > ns) | ((ms == ns) & (mi < ni)))


class Scores:
    """The (F,2) idx / label / score arrays of mated_search with the probes' labels, as host arrays."""

    def __init__(self, idx, label, score, probe_labels):
        self.idx = np.asarray(idx, np.int64).reshape(-1, 2)
        self.label = np.asarray(label, np.int64).reshape(-1, 2)
        self.score = np.asarray(score, np.float32).reshape(-1, 2)
        self.probe_labels = np.asarray(probe_labels, np.int64).reshape(-1)
        if not self.idx.shape == self.label.shape == self.score.shape == (self.probe_labels.shape[0], 2):
            raise ValueError("idx, label and score must be (F,2) with F probe labels")
        self.has_mate = self.idx[:, 0] >= 0
        self.has_nonmate = self.idx[:, 1] >= 0
        self.Fm, self.Fn = int(self.has_mate.sum()), int(self.has_nonmate.sum())
        self.rank1 = _outranks(self.score[:, 0], self.idx[:, 0], self.score[:, 1], self.idx[:, 1])


def global_threshold(sc, far):
    return threshold_at_far(sc.score[sc.has_nonmate, 1], far)


def class_thresholds(sc, far, num_classes, thr=None):
    """{str(c): float for c in range(num_classes)}: what statistics.build_thresholds reads and identify_names indexes."""
    thr = global_threshold(sc, far) if thr is None else np.float32(thr)
    n, nl = sc.score[sc.has_nonmate, 1], sc.label[sc.has_nonmate, 1]
    order = np.argsort(nl, kind="stable")
    n, nl = n[order], nl[order]
    lo, hi = np.searchsorted(nl, np.arange(num_classes), "left"), np.searchsorted(nl, np.arange(num_classes), "right")
    out = {}
    for c in range(num_classes):
        t = thr if lo[c] == hi[c] else max(threshold_at_far(n[lo[c]:hi[c]], far), thr)
        out[str(c)] = float(np.float32(t))
    return out


def achieved_far(sc, thr):
    """#{n_p >= thr} / Fn; 0.0 when no probe has a non-mate."""
    if sc.Fn == 0:
        return 0.0
    return float((sc.score[sc.has_nonmate, 1] >= np.float32(thr)).sum()) / sc.Fn


def detection_rate(sc, local):
    """DIR: the share of the Fm probes whose mate reaches its class's threshold and outranks their non-mate; None
    without mated probes."""
    if sc.Fm == 0:
        return None
    m = sc.has_mate
    lt = np.array([local[str(int(l))] for l in sc.probe_labels[m]], np.float32)
    return float(((sc.score[m, 0] >= lt) & sc.rank1[m]).sum()) / sc.Fm


def rank1_accuracy(sc):
    """Closed-set rank-1: the share of the Fm probes whose mate outranks their non-mate; None without mated probes."""
    return None if sc.Fm == 0 else float(sc.rank1[sc.has_mate].sum()) / sc.Fm


def operating_point(sc, far, num_classes):
    thr = global_threshold(sc, far)
    local = class_thresholds(sc, far, num_classes, thr)
    return {"far": far, "thr": float(thr), "achieved_far": achieved_far(sc, thr), "dir": detection_rate(sc, local)}, local


def calibrate(sc, far, num_classes):
    """-> (thresholds dict, report dict) for the target `far`."""
    far = check_far(far)
    point, local = operating_point(sc, far, num_classes)
    report = {"far_target": far, "thr": point["thr"], "Fm": sc.Fm, "Fn": sc.Fn, "F": int(sc.probe_labels.shape[0]),
              "achieved_far": point["achieved_far"], "dir": point["dir"], "rank1": rank1_accuracy(sc), "operating_points": [], "notes": []}
    for f in FAR_POINTS:
        if accepted_impostors(sc.Fn, f) >= 1:
            report["operating_points"].append(operating_point(sc, f, num_classes)[0])
    if sc.Fn == 0:
        report["notes"].append("no probe has a non-mate (one label only): thr is -1.0, every cosine passes, nothing was calibrated")
    if sc.Fm == 0:
        report["notes"].append("no probe has a mate: DIR and rank-1 are undefined")
    return local, report


def write_thresholds(path, local):
    """repr(float(np.float32)) per value: json reads back the same double, so identify_names compares exactly."""
    with open(path, "w") as fp:
        fp.write("{" + ", ".join('"%s": %s' % (k, repr(float(v))) for k, v in local.items()) + "}\n")


def write_report(path, report):
    with open(path, "w") as fp:
        json.dump(report, fp, indent=1)
        fp.write("\n")
