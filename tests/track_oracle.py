"""float64 oracle of the face tracks (vnf_gallery_tracks / vnf_gallery_track_sums, csrc/gallery_tracks.hip), written from
the contract in include/vnface.h; no reference code exists for this feature.

    s = gallery_oracle.scores(rows, rows); f = the frame ordinals, non-decreasing
    j is a forward candidate of i:  0 < f[j] - f[i] <= max_gap,  s[i,j] >= t (a NaN never),  and with min_iou > 0
        inter >= min_iou * union of the two boxes; backward candidates are the mirror image
    next(i) / pred(j): the best candidate under (frame distance ascending, score descending, row ascending)
    link i -> j: next(i) == j and pred(j) == i; tracks: the chains, numbered by their first row

Exact equality with the device only means something when no decision sits within rounding of a boundary, so the oracle
also returns the three margins a test asserts first, each taken over the in-window pairs (0 < |f[j] - f[i]| <= max_gap):
margin_t, the smallest |s - t|; margin_iou, the smallest |inter - min_iou * union| / union (inf with min_iou <= 0);
margin_lead, the smallest lead of a chosen candidate over the best other candidate AT THE SAME FRAME DISTANCE.  With
`rows` given, candidates whose row is byte for byte the chosen one's are no runners-up: they score the same bits on the
device as well, and the contract lets the row index decide."""
import numpy as np

import gallery_oracle as go


class Result:
    pass


def overlap(a, b):
    """-> (inter, union) of two x1,y1,x2,y2 boxes in float64, by the header's formula"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    iw = max(0.0, min(a[2], b[2]) - max(a[0], b[0]))
    ih = max(0.0, min(a[3], b[3]) - max(a[1], b[1]))
    inter = iw * ih
    return inter, (a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1]) - inter


def link_scores(s, frame_ord, boxes, t, min_iou, max_gap, rows=None):
    """(G,G) float64 scores, (G) ordinals, (G,4) boxes or None -> Result with prev, next, track (int64), n_tracks,
    link_score (float64, -inf at a head), margin_t, margin_iou, margin_lead."""
    s = np.asarray(s, np.float64)
    f = np.asarray(frame_ord, np.int64)
    g = f.shape[0]
    assert s.shape == (g, g) and (g < 2 or (np.diff(f) >= 0).all())
    res = Result()
    res.margin_t = res.margin_iou = res.margin_lead = np.inf
    cand = np.zeros((g, g), bool)                     # cand[i, j]: j is a candidate of i (forward where f[j] > f[i])
    for i in range(g):
        for j in range(g):
            d = abs(int(f[j] - f[i]))
            if not 0 < d <= max_gap:
                continue
            ok = bool(s[i, j] >= t)                   # NaN: False
            if not np.isnan(s[i, j]):
                res.margin_t = min(res.margin_t, abs(s[i, j] - t))
            if min_iou > 0:
                inter, union = overlap(boxes[i], boxes[j])
                ok = ok and inter >= min_iou * union
                if union > 0:
                    res.margin_iou = min(res.margin_iou, abs(inter - min_iou * union) / union)
            cand[i, j] = ok

    def best(i, sign):
        """the best candidate of row i among later (sign +1) or earlier (-1) frames, -1 without one"""
        js = [j for j in range(g) if cand[i, j] and sign * (f[j] - f[i]) > 0]
        if not js:
            return -1
        js.sort(key=lambda j: (abs(int(f[j] - f[i])), -s[i, j], j))
        b = js[0]
        rivals = [j for j in js[1:] if f[j] == f[b] and (rows is None or rows[j].tobytes() != rows[b].tobytes())]
        if rivals:
            res.margin_lead = min(res.margin_lead, s[i, b] - max(s[i, j] for j in rivals))
        return b

    nxt = np.array([best(i, +1) for i in range(g)], np.int64).reshape(g)
    prd = np.array([best(i, -1) for i in range(g)], np.int64).reshape(g)
    res.next = np.array([n if n >= 0 and prd[n] == i else -1 for i, n in enumerate(nxt)], np.int64).reshape(g)
    res.prev = np.array([p if p >= 0 and nxt[p] == i else -1 for i, p in enumerate(prd)], np.int64).reshape(g)
    res.link_score = np.array([s[i, p] if p >= 0 else -np.inf for i, p in enumerate(res.prev)], np.float64).reshape(g)
    res.track = np.full(g, -1, np.int64)
    n = 0
    for i in range(g):                                # prev[i] < i: a head is met before the rest of its chain
        if res.prev[i] < 0:
            res.track[i] = n
            n += 1
        else:
            assert res.prev[i] < i and res.next[res.prev[i]] == i
            res.track[i] = res.track[res.prev[i]]
    res.n_tracks = n
    return res


def link(rows, frame_ord, boxes, t, min_iou, max_gap):
    rows = np.asarray(rows)
    return link_scores(go.scores(rows, rows), frame_ord, boxes, t, min_iou, max_gap, rows)


def sequential_sums(unit_rows, track, n_tracks):
    """Per track the fp32 sum of its STORED rows in row order, s = s + x from 0 -> (sums (n_tracks,dim) fp32, counts)."""
    unit_rows = np.asarray(unit_rows)
    assert unit_rows.dtype == np.float32
    sums = np.zeros((n_tracks, unit_rows.shape[1]), np.float32)
    counts = np.zeros((n_tracks,), np.int64)
    for x, k in zip(unit_rows, np.asarray(track, np.int64)):
        sums[k] = sums[k] + x
        counts[k] += 1
    return sums, counts
