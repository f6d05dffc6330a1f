#!/usr/bin/env python3
"""Part (a) of tools/emotion_stream_time.py -- frames per second of video.run_stream + VideoEncoder on 64 synthetic 1080p
frames in batches of 16, without emotions and with emotions=6 -- for two run_stream implementations in ONE process on one
card, alternating: another commit's video.py (--parent FILE, e.g. written by `git show HEAD~1:vn_celeb_face_recognition_amd/
video.py > FILE`; loaded as a sibling module of the package) and the working tree's.  Every pass is printed, with the
parent's spread, and whether the tracker rows and the encoded files of the two are equal.

    python tools/stream_parts_ab.py --parent FILE [--frames 64] [--batch 16] [--passes 3] [--out profiles/stream_parts_ab.txt]
"""
import argparse
import importlib.util
import json
import os
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from vn_celeb_face_recognition_amd import jpeg_encode, models  # noqa: E402
from vn_celeb_face_recognition_amd import video as video_new  # noqa: E402
from vn_celeb_face_recognition_amd.pipeline import FacePipeline  # noqa: E402
from vn_celeb_face_recognition_amd.synth import make_frames  # noqa: E402

DEV = "cuda:0"
K = 6


def load_parent(path):
    name = "vn_celeb_face_recognition_amd.video_parent"
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--parent", required=True, help="the other commit's vn_celeb_face_recognition_amd/video.py")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU is visible")
    impl = {"parent": load_parent(args.parent), "new": video_new}
    n, B = args.frames, args.batch
    frames, _ = make_frames(n, 4)
    h, w = frames.shape[1:3]
    tags = json.load(open(os.path.join(ROOT, "tests", "golden", "etag2idx.json")))["idx2key"]
    tmp = tempfile.mkdtemp()
    det = models.MTCNN(keep_all=True, min_face_size=50, device=DEV, max_batch=B, max_height=h, max_width=w)
    enc = models.InceptionResnetV1(pretrained=None, max_batch=256).to(DEV).eval()
    clf = models.MLPModel(512, 1001).to(DEV).eval()
    emo = models.resnet_2branch_50(num_classes=len(tags), max_batch=64).to(DEV).eval()
    l2n = {"label": list(range(1001)), "name": ["celeb_%d" % i for i in range(1001)]}
    rows_of, video_of = {}, {}

    def stream_pass(which, with_emotions):
        v = impl[which]
        pipe = FacePipeline(det, enc, clf, l2n, 160, 0.0, embed_batch=256, emotion=emo if with_emotions else None, topk_emotions=K)
        path = os.path.join(tmp, "out_%s_%d.avi" % (which, with_emotions))
        video = jpeg_encode.VideoEncoder(path, 25.0, DEV, idx2tag=dict(enumerate(tags)))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rows, processed = v.run_stream(v.FrameSource(frames, 25.0), pipe, B, 0, 1, device=DEV, encoder=video,
                                       emotions=K if with_emotions else 0,
                                       row=lambda tm, num, names, boxes, shape, emotions=None: v.tracker_row(tm, num, names, boxes, shape))
        video.close()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert processed == n
        rows_of[which, with_emotions] = rows
        video_of[which, with_emotions] = open(path, "rb").read()
        os.remove(path)
        return dt

    order = [(wh, we) for we in (False, True) for wh in ("parent", "new")]
    for wh, we in order:                             # warm-up: code objects, tune cache, buffers
        stream_pass(wh, we)
    times = {k: [] for k in order}
    for i in range(args.passes):                     # alternating, the order reversed every other round
        for k in (order if i % 2 == 0 else order[::-1]):
            times[k].append(stream_pass(*k))
    same_rows = all(rows_of["parent", we] == rows_of["new", we] for we in (False, True))
    same_video = all(video_of["parent", we] == video_of["new", we] for we in (False, True))
    lines = ["# run_stream + VideoEncoder (q92 4:2:0), %d synthetic %dx%d frames, 4 pasted faces each, batches of %d, one GPU, one process;"
             % (n, w, h, B),
             "# parent commit's video.py and this commit's, %d alternating passes each after one warm-up pass; frames/s per pass" % args.passes,
             "# tracker rows equal: %s; encoded video files byte-identical: %s" % (same_rows, same_video)]
    for we in (False, True):
        fps = {wh: [n / t for t in times[wh, we]] for wh in ("parent", "new")}
        spread = max(fps["parent"]) - min(fps["parent"])
        short = max(fps["parent"]) - max(fps["new"])
        lines.append("emotions=%d" % (K if we else 0))
        for wh in ("parent", "new"):
            lines.append("    %-6s passes: %s   best %.1f" % (wh, "  ".join("%.1f" % f for f in fps[wh]), max(fps[wh])))
        lines.append("    parent's spread (max - min) %.1f; new best falls short of parent best by %.1f -> %s"
                     % (spread, short, "within the spread" if short <= spread else "OUTSIDE the spread"))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    os.rmdir(tmp)


if __name__ == "__main__":
    main()
