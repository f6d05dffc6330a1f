"""GPU: vnf_gallery_tracks / vnf_gallery_track_sums (csrc/gallery_tracks.hip) and tracking.link_tracks against the float64
oracle tests/track_oracle.py.

The scenes are random: identities as tight blobs (a unit centre plus noise), a few of them per frame, with a noisier second
face of one identity in the larger frames so that candidates compete, boxes that follow the identity with a jitter and
now and then jump.  prev, next, track and n_tracks are compared EXACTLY, which only means something when no decision sits
within rounding of a boundary: every comparison first asserts on the CPU that the oracle's three margins exceed
4 * gallery_oracle.tol(dim); the seeds were chosen so that they do.  link_score is held to tol(dim) and, on a scene of
far-apart pairs, to the bits of vnf_gallery_cluster's score of the same pair; the sums to the bits of a sequential fp32 sum
of the stored rows.  Every raw call runs with guard bytes around its outputs and its workspace."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import gallery_oracle as go
import track_oracle as to
from test_gpu_gallery import DEV, Guarded, RawGallery
from test_gpu_gallery_cluster import cluster
from vn_celeb_face_recognition_amd import _lib, tracking

pytestmark = pytest.mark.gpu
INVALID, CAPACITY = -1, -4
T = 0.5
IOU = 0.3
# frame boundaries at rows 15|16, 16|17 and 31|32|33 (a frame straddles a wave's 16 rows and a 32-row step), an empty frame
# (9) between two frames of a track, two more (15, 16) that only max_gap 4 bridges; 70 rows
SIZES = (5, 6, 4, 1, 1, 7, 7, 1, 1, 0, 6, 5, 4, 3, 2, 0, 0, 4, 5, 8)
CROWD = (4, 40, 6, 40, 3)            # a window longer than a 32-row step, on both sides of a row
SEEDS = {(512, SIZES): 1, (32, SIZES): 1, (512, CROWD): 1}


def _unit(x):
    return x / np.linalg.norm(x, axis=-1, keepdims=True)


def scene(seed, dim, sizes, n_ids):
    """-> rows (G,dim) fp32 of norms 0.1 .. 30, frame ordinals (G) int64, boxes (G,4) fp32.  Identity 0 is in every frame
    that has a face; a frame of six or more ends with a second, noisier face of its first identity."""
    rng = np.random.default_rng(seed)
    centres = np.linalg.qr(rng.standard_normal((dim, dim)))[0][:n_ids]          # orthonormal: identities far apart
    rows, frames, boxes = [], [], []
    for p, size in enumerate(sizes):
        if size == 0:
            continue
        twin = size >= 6
        ids = [0] + list(1 + rng.permutation(n_ids - 1)[:size - 1 - twin])
        noise = [rng.uniform(0.3, 0.5) for _ in ids]
        if twin:
            ids.append(ids[0])
            noise.append(0.7)
        for k, r in zip(ids, noise):
            rows.append(_unit(centres[k] + r * _unit(rng.standard_normal(dim))))
            x0 = 40.0 * (k % 12) + rng.uniform(-3, 3) + (rng.uniform(20, 45) if rng.uniform() < 0.2 else 0.0)
            y0 = 30.0 * (k % 12) + 100.0 * (k // 12) + rng.uniform(-3, 3)
            boxes.append([x0, y0, x0 + 60.0, y0 + 80.0])
            frames.append(p)
    x = np.stack(rows) * rng.uniform(0.1, 30.0, (len(rows), 1))
    return x.astype(np.float32), np.array(frames, np.int64), np.array(boxes, np.float32)


@functools.lru_cache(maxsize=None)
def case(dim, sizes):
    x, f, b = scene(SEEDS[(dim, sizes)], dim, sizes, 10 if sizes == SIZES else 48)
    s = go.scores(x, x)
    for a in (x, f, b, s):
        a.setflags(write=False)
    return x, f, b, s


@functools.lru_cache(maxsize=None)
def oracle(dim, sizes, n, t, min_iou, max_gap):
    """The oracle of the case's first n rows, with its margins asserted."""
    x, f, b, s = case(dim, sizes)
    o = to.link_scores(s[:n, :n], f[:n], b[:n], t, min_iou, max_gap, x[:n])
    lim = 4 * go.tol(dim)
    assert o.margin_t > lim and o.margin_iou > lim and o.margin_lead > lim, (dim, n, t, min_iou, max_gap, o.margin_t, o.margin_iou, o.margin_lead)
    return o


def P(t, off=0):
    return ctypes.c_void_p(t.data_ptr() + off)


def tracks(rg, f, boxes, t, min_iou, max_gap):
    """Both entries of the C ABI with guards -> dict of numpy arrays; boxes None: a NULL pointer."""
    g, lib = rg.size, rg.lib
    n_frames = int(f[-1]) + 1 if g else 0
    first = torch.from_numpy(tracking.frame_first(f, n_frames)).to(DEV)
    bx = torch.from_numpy(np.array(boxes, np.float32)).to(DEV) if boxes is not None else None
    nbytes = lib.vnf_gallery_tracks_workspace_bytes(g)
    assert nbytes >= 16
    outs = [Guarded((g,), torch.int32), Guarded((g,), torch.int32), Guarded((g,), torch.float32), Guarded((g,), torch.int32),
            Guarded((1,), torch.int32)]
    ws = Guarded((nbytes,), torch.uint8)
    _lib.check(lib.vnf_gallery_tracks(rg.h, P(first), n_frames, P(bx) if bx is not None else None, t, min_iou, max_gap,
                                      *[P(o.t) for o in outs], P(ws.t), nbytes, _lib.current_stream_ptr()))
    torch.cuda.synchronize()
    assert all(o.intact() for o in outs) and ws.intact(), "guard bytes overwritten"
    n = int(outs[4].t.item())
    sums, counts = Guarded((n, rg.dim), torch.float32), Guarded((n,), torch.int32)
    _lib.check(lib.vnf_gallery_track_sums(rg.h, P(outs[0].t), P(outs[1].t), P(outs[3].t), n, P(sums.t), P(counts.t),
                                          _lib.current_stream_ptr()))
    torch.cuda.synchronize()
    assert sums.intact() and counts.intact() and all(o.intact() for o in outs), "guard bytes overwritten"
    names = ("prev", "next", "link_score", "track")
    d = {k: o.t.cpu().numpy() for k, o in zip(names, outs)}
    d.update(n_tracks=n, sums=sums.t.cpu().numpy(), counts=counts.t.cpu().numpy())
    return d


def _same_bits(a, b):
    """bit-equal, a NaN matching a NaN"""
    return a.shape == b.shape and bool(((a.view(np.int32) == b.view(np.int32)) | (np.isnan(a) & np.isnan(b))).all())


def check(got, o, unit, tol):
    """Exact links and tracks, link_score within tol, sums the bits of the sequential fp32 sum of the stored rows `unit`.
    The oracle's margins were asserted by the caller."""
    assert np.array_equal(got["prev"], o.prev), np.flatnonzero(got["prev"] != o.prev)[:10]
    assert np.array_equal(got["next"], o.next), np.flatnonzero(got["next"] != o.next)[:10]
    assert got["n_tracks"] == o.n_tracks and np.array_equal(got["track"], o.track)
    head = o.prev < 0
    assert (got["link_score"][head] == -np.inf).all()
    err = np.abs(got["link_score"][~head] - o.link_score[~head])
    assert (err <= tol).all(), err.max()
    sums, counts = to.sequential_sums(unit, o.track, o.n_tracks)
    assert np.array_equal(got["counts"], counts) and _same_bits(got["sums"], sums)
    return float(err.max()) if err.size else 0.0


def _gallery(x, f):
    return RawGallery(x.shape[1]).add(x, f)


@pytest.mark.parametrize("dim", [512, 32])
@pytest.mark.parametrize("G", [1, 2, 15, 16, 17, 33, 70])
def test_shapes_meet_the_oracle(dim, G):
    x, f, b, _ = case(dim, SIZES)
    rg = _gallery(x[:G], f[:G])
    unit = rg.rows(0, G)
    worst, links = 0.0, []
    for max_gap in (1, 2, 4):
        for min_iou in (0.0, IOU):
            o = oracle(dim, SIZES, G, T, min_iou, max_gap)                       # asserts the three margins on the CPU
            worst = max(worst, check(tracks(rg, f[:G], b[:G] if min_iou > 0 else None, T, min_iou, max_gap), o, unit, go.tol(dim)))
            links.append(int((o.prev >= 0).sum()))
    print("dim=%d G=%d: links per (gap, iou) %s; max |link_score - float64 oracle| = %.3g (tol %.3g)" % (dim, G, links, worst, go.tol(dim)))
    if G == 70:
        by = dict(zip([(g, i) for g in (1, 2, 4) for i in (0, 1)], links))
        assert by[(1, 0)] < by[(2, 0)] < by[(4, 0)]                              # the empty frames are bridged by the wider gaps only
        assert all(by[(g, 1)] < by[(g, 0)] for g in (1, 2, 4))                   # the boxes take links away
    rg.close()


def test_a_frame_of_forty_faces():
    x, f, b, _ = case(512, CROWD)
    g = x.shape[0]
    rg = _gallery(x, f)
    unit = rg.rows(0, g)
    for max_gap in (1, 2):
        for min_iou in (0.0, IOU):
            o = oracle(512, CROWD, g, T, min_iou, max_gap)
            check(tracks(rg, f, b, T, min_iou, max_gap), o, unit, go.tol(512))
    assert oracle(512, CROWD, g, T, 0.0, 2).n_tracks < oracle(512, CROWD, g, T, 0.0, 1).n_tracks
    rg.close()


def test_the_same_input_twice_gives_the_same_bytes():
    x, f, b, _ = case(512, CROWD)
    rg = _gallery(x, f)
    first = tracks(rg, f, b, T, IOU, 2)
    for run in range(3):
        again = tracks(rg, f, b, T, IOU, 2)
        assert all(np.array_equal(np.asarray(first[k]).view(np.int32), np.asarray(again[k]).view(np.int32))
                   for k in ("prev", "next", "link_score", "track", "sums", "counts")) and first["n_tracks"] == again["n_tracks"], run
    rg.close()


def test_a_duplicate_row_loses_to_the_lower_index():
    """frame 0: a; frame 1: b, c, then b and c again (rows 3, 4), where a prefers b: a links to row 1, the copies stay alone"""
    rng = np.random.default_rng(21)
    c = _unit(rng.standard_normal(512))
    a, b1, c1 = (_unit(c + r * _unit(rng.standard_normal(512))) for r in (0.3, 0.3, 0.6))
    x = np.stack([a, b1, c1, b1, c1]).astype(np.float32) * np.float32(3.0)
    f = np.array([0, 1, 1, 1, 1])
    o = to.link(x, f, None, T, 0.0, 1)
    assert o.margin_t > 4 * go.tol(512) and o.margin_lead > 4 * go.tol(512)
    assert o.next.tolist() == [1, -1, -1, -1, -1] and o.prev.tolist() == [-1, 0, -1, -1, -1] and o.n_tracks == 4
    rg = _gallery(x, f)
    check(tracks(rg, f, None, T, 0.0, 1), o, rg.rows(0, 5), go.tol(512))
    rg.close()


def test_a_nan_row_is_never_linked():
    x, f, b, _ = case(512, SIZES)
    g = 33
    clean = oracle(512, SIZES, g, T, 0.0, 2)
    at = int(np.flatnonzero((clean.prev >= 0) & (clean.next >= 0))[0])           # a row inside a track
    bad = x[:g].copy()
    bad[at, 100] = np.nan
    o = to.link(bad, f[:g], None, T, 0.0, 2)
    lim = 4 * go.tol(512)
    assert o.margin_t > lim and o.margin_lead > lim and o.prev[at] == o.next[at] == -1
    rg = _gallery(bad, f[:g])
    got = tracks(rg, f[:g], None, T, 0.0, 2)
    check(got, o, rg.rows(0, g), go.tol(512))
    assert got["counts"][got["track"][at]] == 1
    rg.close()


def test_a_threshold_nobody_meets_gives_singletons():
    x, f, b, _ = case(512, SIZES)
    rg = _gallery(x, f)
    got = tracks(rg, f, b, 2.0, IOU, 4)
    g = x.shape[0]
    assert got["n_tracks"] == g and np.array_equal(got["track"], np.arange(g)) and (got["prev"] == -1).all() and (got["next"] == -1).all()
    assert (got["link_score"] == -np.inf).all() and (got["counts"] == 1).all()
    assert np.array_equal(got["sums"].view(np.int32), rg.rows(0, g).view(np.int32))        # 0 + x: the stored row
    rg.close()


def test_through_link_tracks():
    x, f, b, _ = case(512, SIZES)
    rg = _gallery(x, f)
    unit = rg.rows(0, x.shape[0])
    for min_iou, boxes in ((0.0, None), (IOU, b)):
        r = tracking.link_tracks(x, f, boxes, threshold=T, min_iou=min_iou, max_gap=2, device=DEV)
        got = dict(prev=r.prev, next=r.next, link_score=r.link_score, track=r.track, n_tracks=r.n_tracks, sums=r.sums, counts=r.counts)
        assert all(got[k].dtype == np.int32 for k in ("prev", "next", "track", "counts")) and r.sums.dtype == r.link_score.dtype == np.float32
        check(got, oracle(512, SIZES, 70, T, min_iou, 2), unit, go.tol(512))
    empty = tracking.link_tracks(np.zeros((0, 512), np.float32), np.zeros((0,), np.int64), threshold=T, device=DEV)
    assert empty.n_tracks == 0 and empty.track.shape == (0,) and empty.sums.shape == (0, 512)
    with pytest.raises(RuntimeError, match="no CPU path"):
        tracking.link_tracks(x, f, threshold=T, device="cpu")
    rg.close()


def test_error_codes():
    x, f, b, _ = case(512, SIZES)
    g = 33
    rg = _gallery(x[:g], f[:g])
    lib = rg.lib
    n_frames = int(f[g - 1]) + 1
    first = torch.from_numpy(tracking.frame_first(f[:g], n_frames)).to(DEV)
    bx = torch.from_numpy(np.concatenate([b[:g], b[:1]])).to(DEV)
    out = [torch.empty((g,), dtype=dt, device=DEV) for dt in (torch.int32, torch.int32, torch.float32, torch.int32)]
    nt = torch.full((1,), 77, dtype=torch.int32, device=DEV)
    need = lib.vnf_gallery_tracks_workspace_bytes(g)
    assert need == 5 * 36 * 4                           # five arrays of 36 entries
    ws = torch.empty((need + 16,), dtype=torch.uint8, device=DEV)

    def call(h=rg.h, fp=P(first), nf=n_frames, bp=P(bx), t=T, iou=IOU, gap=2, o0=P(out[0]), o1=P(out[1]), o2=P(out[2]), o3=P(out[3]),
             np_=P(nt), wp=P(ws), nbytes=need):
        return lib.vnf_gallery_tracks(h, fp, nf, bp, t, iou, gap, o0, o1, o2, o3, np_, wp, nbytes, None)

    assert call() == 0
    torch.cuda.synchronize()
    o = oracle(512, SIZES, g, T, IOU, 2)
    assert int(nt.item()) == o.n_tracks and np.array_equal(out[3].cpu().numpy(), o.track)
    for kw in ("fp", "bp", "o0", "o1", "o2", "o3", "np_", "wp"):
        assert call(**{kw: None}) == INVALID, kw
    assert call(bp=None, iou=0.0) == 0                                           # without min_iou the boxes may be NULL
    assert call(wp=P(ws, 4)) == INVALID and call(wp=P(ws, 8)) == INVALID         # workspace not 16-byte aligned
    assert call(bp=P(bx, 4)) == INVALID                                          # nor the boxes
    assert call(nbytes=need - 4) == CAPACITY
    assert call(t=float("nan")) == INVALID and call(iou=float("nan")) == INVALID
    for gap in (0, -1, 256):
        assert call(gap=gap) == INVALID, gap
    assert call(gap=255) == 0
    assert call(nf=-1) == INVALID
    assert call(h=None) == INVALID
    assert lib.vnf_gallery_tracks_workspace_bytes(-1) == INVALID and lib.vnf_gallery_tracks_workspace_bytes(0) == 16
    sums = torch.empty((o.n_tracks, 512), dtype=torch.float32, device=DEV)
    counts = torch.empty((o.n_tracks,), dtype=torch.int32, device=DEV)

    def pool(h=rg.h, p0=P(out[0]), p1=P(out[1]), p3=P(out[3]), n=o.n_tracks, sp=P(sums), cp=P(counts)):
        return lib.vnf_gallery_track_sums(h, p0, p1, p3, n, sp, cp, None)

    assert call() == 0 and pool() == 0
    for kw in ("p0", "p1", "p3", "sp", "cp"):
        assert pool(**{kw: None}) == INVALID, kw
    assert pool(n=-1) == INVALID and pool(h=None) == INVALID and pool(sp=P(sums, 4)) == INVALID
    assert pool(n=0, sp=None, cp=None) == 0
    torch.cuda.synchronize()
    empty = RawGallery(512)                            # G == 0: a no-op that writes n_tracks = 0 and looks at no other pointer
    assert lib.vnf_gallery_tracks(empty.h, None, 0, None, T, 0.0, 1, None, None, None, None, P(nt), None, 0, None) == 0
    torch.cuda.synchronize()
    assert int(nt.item()) == 0
    empty.close(); rg.close()


@pytest.mark.parametrize("dim", [512, 32])
def test_link_score_is_the_clustering_score_bit_for_bit(dim):
    """a link's score is f-17's score of the pair, the same bits.  17 pairs of rows, pair k two noisy
    copies of centre k of an orthonormal set, row 2k in frame 2k and row 2k + 1 in frame 2k + 1: at max_gap 1 the only
    links are 2k -> 2k + 1, and each row's nearest other row under vnf_gallery_cluster is its mate."""
    rng = np.random.default_rng(7)
    centres = np.linalg.qr(rng.standard_normal((dim, dim)))[0][:17]
    x = _unit(np.repeat(centres, 2, axis=0) + 0.15 * _unit(rng.standard_normal((34, dim))))
    x = (x * rng.uniform(0.1, 30.0, (34, 1))).astype(np.float32)
    f = np.arange(34)
    s = go.scores(x, x)
    even, odd = np.arange(0, 34, 2), np.arange(1, 34, 2)
    within = s[even, odd]
    cross = s.copy()
    cross[np.arange(34), np.arange(34)] = -1.0
    cross[even, odd] = cross[odd, even] = -1.0
    lim = 4 * go.tol(dim)
    assert within.min() >= 0.8 and cross.max() <= 0.2, (within.min(), cross.max())
    assert within.min() - T > lim and T - cross.max() > lim
    rg = _gallery(x, f)
    got = tracks(rg, f, None, T, 0.0, 1)
    want_next, want_prev = np.full(34, -1), np.full(34, -1)
    want_next[even], want_prev[odd] = odd, even
    assert np.array_equal(got["next"], want_next) and np.array_equal(got["prev"], want_prev) and got["n_tracks"] == 17
    _, _, nn_idx, nn_score, _ = cluster(rg, T, 2)
    assert np.array_equal(nn_idx[even], odd) and np.array_equal(nn_idx[odd], even)
    link = got["link_score"][odd].view(np.int32)
    assert np.array_equal(link, nn_score[even].view(np.int32)) and np.array_equal(link, nn_score[odd].view(np.int32))
    assert (np.abs(got["link_score"][odd] - within) <= go.tol(dim)).all()
    rg.close()
