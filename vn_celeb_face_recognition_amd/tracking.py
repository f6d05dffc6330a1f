"""Face tracks in video: the faces of consecutive processed frames linked into tracks on the GPU, one name per track
(csrc/gallery_tracks.hip).

    r = link_tracks(emb, frame_ord, boxes, threshold=t, min_iou=0.0, max_gap=1, device="cuda:0")
    pooled = pool_tracks(emb, r)
    names = name_tracks(pooled, classifier, label2name, threshold)

link_tracks stores the G embeddings (in frame order) as a temporary gallery whose labels are the frame ordinals and calls
vnf_gallery_tracks: face i of frame p and face j of a later frame at most max_gap frames on are linked when each is the
other's best candidate -- cosine >= threshold, boxes overlapping by min_iou where that is set -- under (nearest frame,
then best cosine, then first row).  The links form chains, the tracks, numbered by their first face.
vnf_gallery_track_sums adds the unit rows of each track in row order.  pool_tracks turns the sums into one embedding
per track, name_tracks names them the way video.run_stream names single faces.  There is no CPU path."""
import ctypes

import numpy as np
import torch

from . import _lib
from .pipeline import identify_names

MAX_GAP = 255
POOL_EPS = 1e-12


class TrackResult:
    """What link_tracks returns, host arrays: track, prev, next (G) int32 (-1: none), link_score (G) fp32 (the cosine of
    the link to prev, -inf at a track's first face), n_tracks, sums (n_tracks,dim) fp32 -- per track the fp32 sum of its
    unit rows in row order -- and counts (n_tracks) int32."""

    def __init__(self, track, prev, next, link_score, n_tracks, sums, counts):
        self.track, self.prev, self.next, self.link_score = track, prev, next, link_score
        self.n_tracks, self.sums, self.counts = int(n_tracks), sums, counts


def frame_first(frame_ord, n_frames):
    """(G) non-decreasing frame ordinals in [0, n_frames) -> (n_frames + 1) int32: the rows of frame p are
    [first[p], first[p + 1])."""
    return np.searchsorted(np.asarray(frame_ord, np.int64), np.arange(n_frames + 1), side="left").astype(np.int32)


def _check(emb, frame_ord, boxes, threshold, min_iou, max_gap):
    emb = np.asarray(emb)
    if emb.ndim != 2 or emb.shape[1] % 16 or not 16 <= emb.shape[1] <= 512:
        raise ValueError("expected (G,dim) embeddings with dim a multiple of 16 in 16..512, got %s" % (emb.shape,))
    g = emb.shape[0]
    f = np.asarray(frame_ord)
    if f.shape != (g,) or (g and f.dtype.kind not in "iu"):
        raise ValueError("expected %d integer frame ordinals, got %s %s" % (g, f.dtype, f.shape))
    f = f.astype(np.int64)
    if g and (int(f.min()) < 0 or int(f.max()) >= 2 ** 31 - 1):
        raise ValueError("frame ordinals must lie in [0, 2^31 - 1)")
    if g > 1 and (np.diff(f) < 0).any():
        raise ValueError("frame ordinals must be sorted: the faces come in frame order")
    threshold, min_iou = float(threshold), float(min_iou)
    if np.isnan(threshold):
        raise ValueError("threshold must be a cosine, got NaN")
    if np.isnan(min_iou):
        raise ValueError("min_iou must be a number, got NaN")
    if int(max_gap) != max_gap or not 1 <= int(max_gap) <= MAX_GAP:
        raise ValueError("max_gap must be an integer in 1..%d, got %r" % (MAX_GAP, max_gap))
    if boxes is not None:
        boxes = np.asarray(boxes, np.float32)
        if boxes.shape != (g, 4):
            raise ValueError("expected (%d,4) boxes, got %s" % (g, boxes.shape))
        if not np.isfinite(boxes).all():
            raise ValueError("boxes hold non-finite values")
    elif min_iou > 0:
        raise ValueError("min_iou > 0 needs the boxes")
    return np.ascontiguousarray(emb, np.float32), f, boxes, threshold, min_iou, int(max_gap)


def link_tracks(emb, frame_ord, boxes=None, *, threshold, min_iou=0.0, max_gap=1, device):
    """emb (G,dim) host embeddings of any norm in frame order, frame_ord (G) their frames' ordinals (the position of the
    frame among the processed frames), boxes (G,4) x1,y1,x2,y2 or None -> TrackResult.  threshold: a cosine, the value
    calibrate.py prints; min_iou <= 0: boxes play no part; max_gap: how many processed frames a link may span."""
    emb, f, boxes, threshold, min_iou, max_gap = _check(emb, frame_ord, boxes, threshold, min_iou, max_gap)
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("link_tracks runs on MI355X only: give it a cuda device (there is no CPU path)")
    g, dim = emb.shape
    if g == 0:
        z = np.zeros((0,), np.int32)
        return TrackResult(z, z.copy(), z.copy(), np.zeros((0,), np.float32), 0, np.zeros((0, dim), np.float32), z.copy())
    dev = device.index if device.index is not None else torch.cuda.current_device()
    cuda = torch.device("cuda:%d" % dev)
    n_frames = int(f[-1]) + 1
    lib = _lib.load()
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    h = ctypes.c_void_p()
    with torch.cuda.device(dev):
        _lib.check(lib.vnf_init(dev))
        _lib.check(lib.vnf_gallery_create(dim, g, ctypes.byref(h)))
        try:
            stream = _lib.current_stream_ptr()
            rows = torch.from_numpy(emb).to(cuda)
            labs = torch.from_numpy(f.astype(np.int32)).to(cuda)
            _lib.check(lib.vnf_gallery_add(h, P(rows), P(labs), g, stream))
            first = torch.from_numpy(frame_first(f, n_frames)).to(cuda)
            bx = torch.from_numpy(np.ascontiguousarray(boxes)).to(cuda) if (boxes is not None and min_iou > 0) else None
            prev, nxt, track = (torch.empty((g,), dtype=torch.int32, device=cuda) for _ in range(3))
            score = torch.empty((g,), dtype=torch.float32, device=cuda)
            n_dev = torch.empty((1,), dtype=torch.int32, device=cuda)
            ws = _lib.workspace(lib.vnf_gallery_tracks_workspace_bytes(g), cuda)
            _lib.check(lib.vnf_gallery_tracks(h, P(first), n_frames, P(bx) if bx is not None else None, threshold, min_iou, max_gap,
                                              P(prev), P(nxt), P(score), P(track), P(n_dev), P(ws), ws.numel(), stream))
            n = int(n_dev.item())
            sums = torch.empty((n, dim), dtype=torch.float32, device=cuda)
            counts = torch.empty((n,), dtype=torch.int32, device=cuda)
            _lib.check(lib.vnf_gallery_track_sums(h, P(prev), P(nxt), P(track), n, P(sums), P(counts), stream))
            out = TrackResult(track.cpu().numpy(), prev.cpu().numpy(), nxt.cpu().numpy(), score.cpu().numpy(), n,
                              sums.cpu().numpy(), counts.cpu().numpy())
        finally:
            lib.vnf_destroy(h)
    return out


def pool_tracks(emb, result):
    """One (dim) embedding per track -> (n_tracks,dim) fp32.  A track of one face keeps that face's embedding as it is,
    bit for bit.  A longer track gets the direction of its template and the length the classifier was trained on:
    sums / max(||sums||, 1e-12), scaled by the mean L2 norm of its members' raw embeddings (1 for InceptionResnetV1's
    unit embeddings, the typical feature length for iresnet100's)."""
    emb = np.asarray(emb, np.float32)
    track = np.asarray(result.track, np.int64)
    if emb.ndim != 2 or track.shape != (emb.shape[0],) or result.sums.shape != (result.n_tracks, emb.shape[1]):
        raise ValueError("pool_tracks: %s embeddings do not belong to this result" % (emb.shape,))
    out = np.empty((result.n_tracks, emb.shape[1]), np.float32)
    counts = np.bincount(track, minlength=result.n_tracks)
    norms = np.sqrt((emb.astype(np.float64) ** 2).sum(axis=1))
    mean_norm = np.bincount(track, weights=norms, minlength=result.n_tracks) / np.maximum(counts, 1)
    sums = result.sums.astype(np.float64)
    length = np.maximum(np.sqrt((sums * sums).sum(axis=1)), POOL_EPS)
    out[:] = (sums / length[:, None] * mean_norm[:, None]).astype(np.float32)
    single = np.flatnonzero(counts[track] == 1)
    out[track[single]] = emb[single]
    return out


def name_tracks(pooled, classifier, label2name, threshold):
    """One name per pooled row, the way video.run_stream names a face: classifier.classify(rows, want_logp=False), then
    identify_names with the same label2name and threshold (a float or the per-class dict).  `classifier`: an MLPModel or
    a GalleryModel on its device."""
    pooled = np.ascontiguousarray(pooled, np.float32)
    if pooled.shape[0] == 0:
        return []
    _, amax, prob = classifier.classify(torch.from_numpy(pooled).to(getattr(classifier, "device", "cpu")), want_logp=False)
    return identify_names(amax, prob, classifier.num_classes, label2name, threshold)
