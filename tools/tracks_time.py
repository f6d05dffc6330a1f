#!/usr/bin/env python3
"""What linking face tracks costs: vnf_gallery_tracks and vnf_gallery_track_sums (csrc/gallery_tracks.hip) at dim 512 for
G in {1 000, 100 000} faces x {4, 32} faces per frame x max_gap in {1, 4}: microseconds per call (device events, after a
warm-up).  The scene: as many people as there are faces in a frame, each in every frame (a unit centre plus noise, mates
at a cosine of about 0.86), threshold 0.5, no boxes.  Beside each figure a torch stand-in, for comparison only: the same
links from a banded g[a:b] @ g[lo:hi].T per block of 4096 rows, masked by frame distance and threshold, an argmax per
direction and the mutual test.  A record (profiles/tracks_time.txt), not a gate; bench.py does not call this.

    python tools/tracks_time.py [--gs 1000,100000] [--per_frame 4,32] [--gaps 1,4] [--steps 20] [--warmup 3] --out profiles/tracks_time.txt
"""
import argparse
import ctypes
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
DIM = 512
T = 0.5
BLOCK = 4096


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps * 1e3     # us


def torch_links(g, frame, per_frame, gap):
    """next (G) int64, -1 without a link: best candidate per direction by (frame distance, score), then the mutual test.
    Ties between equal scores are not ordered by row as the kernel orders them: a comparison line, not an oracle."""
    G = g.shape[0]
    nxt = torch.full((G,), -1, dtype=torch.int64, device=g.device)
    prd = torch.full((G,), -1, dtype=torch.int64, device=g.device)
    for a in range(0, G, BLOCK):
        b = min(G, a + BLOCK)
        lo, hi = max(0, a - (gap + 1) * per_frame), min(G, b + (gap + 1) * per_frame)
        s = g[a:b] @ g[lo:hi].T
        d = frame[lo:hi][None, :] - frame[a:b][:, None]
        ok = s >= T
        for sign, out in ((1, nxt), (-1, prd)):
            valid = ok & (sign * d > 0) & (sign * d <= gap)
            key = torch.where(valid, s - 4.0 * (sign * d).float(), torch.full_like(s, -float("inf")))
            best, at = key.max(dim=1)
            out[a:b] = torch.where(best > -float("inf"), at + lo, torch.full_like(at, -1))
    rows = torch.arange(G, device=g.device)
    has = nxt >= 0
    return torch.where(has & (prd[nxt.clamp(min=0)] == rows), nxt, torch.full_like(nxt, -1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gs", default="1000,100000")
    ap.add_argument("--per_frame", default="4,32")
    ap.add_argument("--gaps", default="1,4")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    from vn_celeb_face_recognition_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    _lib.check(lib.vnf_init(0))
    gen = torch.Generator(device=dev).manual_seed(0)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    unit = torch.nn.functional.normalize
    lines = ["# vnf_gallery_tracks + vnf_gallery_track_sums, dim %d fp32, threshold %.1f, no boxes: us per call over %d calls after %d "
             "warm-up (device events)" % (DIM, T, args.steps, args.warmup),
             "# torch: banded g[a:b] @ g[lo:hi].T per %d rows + masks + argmax per direction + mutual test, comparison only" % BLOCK,
             "#       G | per frame | gap | tracks us | sums us | torch us | tracks | same links"]
    for G in [int(v) for v in args.gs.split(",")]:
        for per in [int(v) for v in args.per_frame.split(",")]:
            n_frames = (G + per - 1) // per
            centres = unit(torch.randn((per, DIM), generator=gen, device=dev))
            who = torch.arange(G, device=dev) % per
            rows = unit(centres[who] + 0.4 * unit(torch.randn((G, DIM), generator=gen, device=dev)))
            frame = (torch.arange(G, device=dev) // per).to(torch.int32)
            first = torch.clamp(torch.arange(n_frames + 1, device=dev) * per, max=G).to(torch.int32)
            h = ctypes.c_void_p()
            _lib.check(lib.vnf_gallery_create(DIM, G, ctypes.byref(h)))
            _lib.check(lib.vnf_gallery_add(h, P(rows), P(frame), G, None))
            gm = torch.empty((G, DIM), dtype=torch.float32, device=dev)
            _lib.check(lib.vnf_gallery_rows(h, P(gm), 0, G, None))
            prev, nxt, track = (torch.empty((G,), dtype=torch.int32, device=dev) for _ in range(3))
            score = torch.empty((G,), dtype=torch.float32, device=dev)
            n_dev = torch.zeros((1,), dtype=torch.int32, device=dev)
            nbytes = lib.vnf_gallery_tracks_workspace_bytes(G)
            ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            stream = _lib.current_stream_ptr()
            frame64 = frame.to(torch.int64)
            for gap in [int(v) for v in args.gaps.split(",")]:
                def ours():
                    _lib.check(lib.vnf_gallery_tracks(h, P(first), n_frames, None, T, 0.0, gap, P(prev), P(nxt), P(score), P(track), P(n_dev),
                                                      P(ws), nbytes, stream))

                us = timed(ours, args.steps, args.warmup)
                n = int(n_dev.item())
                sums = torch.empty((n, DIM), dtype=torch.float32, device=dev)
                counts = torch.empty((n,), dtype=torch.int32, device=dev)
                us_s = timed(lambda: _lib.check(lib.vnf_gallery_track_sums(h, P(prev), P(nxt), P(track), n, P(sums), P(counts), stream)),
                             args.steps, args.warmup)
                us_t = timed(lambda: torch_links(gm, frame64, per, gap), args.steps, args.warmup)
                same = int((torch_links(gm, frame64, per, gap) == nxt.to(torch.int64)).sum())
                lines.append("%9d | %9d | %3d | %9.1f | %7.1f | %8.1f | %6d | %d of %d" % (G, per, gap, us, us_s, us_t, n, same, G))
                print(lines[-1], flush=True)
            lib.vnf_destroy(h)
            del gm, rows
            torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    else:
        print(text)


if __name__ == "__main__":
    main()
