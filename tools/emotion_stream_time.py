#!/usr/bin/env python3
"""What emotions cost on the frame stream, from one process on one GPU:

  (a) frames per second of video.run_stream with the device video encoder, without emotions and with
      FacePipeline(emotion=...) + run_stream(emotions=6) + the emotion lines drawn on the device;
  (b) per batch, the SAME emotion lines drawn two ways on frames in HBM:
        glyph runs  -- jpeg_encode.text_runs builds a table, vnf_overlay_draw_text composites the glyphs;
        LABEL masks -- every line rendered by Pillow (`_label_mask`) and drawn by vnf_overlay_draw, the only way the
                       code before the text kernel could draw them;
      for each: the host's table-build time and the kernel's time from HIP events.  The two pictures are compared.

Input: 64 synthetic 1080p frames (synth.make_frames, 4 pasted faces each) in batches of 16; for (b) the pasted faces'
rectangles as boxes and six seeded tags and percentages per face.  Synthetic weights: the tags are meaningless, the
work is the real one.

    python tools/emotion_stream_time.py [--frames 64] [--batch 16] [--passes 3] [--out profiles/emotion_stream_time.txt]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from vn_celeb_face_recognition_amd import jpeg_encode, models  # noqa: E402
from vn_celeb_face_recognition_amd.pipeline import FacePipeline  # noqa: E402
from vn_celeb_face_recognition_amd.synth import make_frames  # noqa: E402
from vn_celeb_face_recognition_amd.video import FrameSource, run_stream, tracker_row  # noqa: E402

DEV = "cuda:0"
K = 6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("emotion_stream_time.py measures on the MI355X: no GPU is visible")
    n, B = args.frames, args.batch
    frames, truth = make_frames(n, 4)
    h, w = frames.shape[1:3]
    tags = json.load(open(os.path.join(ROOT, "tests", "golden", "etag2idx.json")))["idx2key"]
    tmp = tempfile.mkdtemp()

    # (a) the stream ------------------------------------------------------------------------------------------------
    det = models.MTCNN(keep_all=True, min_face_size=50, device=DEV, max_batch=B, max_height=h, max_width=w)
    enc = models.InceptionResnetV1(pretrained=None, max_batch=256).to(DEV).eval()
    clf = models.MLPModel(512, 1001).to(DEV).eval()
    emo = models.resnet_2branch_50(num_classes=len(tags), max_batch=64).to(DEV).eval()
    l2n = {"label": list(range(1001)), "name": ["celeb_%d" % i for i in range(1001)]}
    faces_seen = {}

    def stream_pass(with_emotions):
        pipe = FacePipeline(det, enc, clf, l2n, 160, 0.0, embed_batch=256, emotion=emo if with_emotions else None, topk_emotions=K)
        path = os.path.join(tmp, "out_%d.avi" % with_emotions)
        video = jpeg_encode.VideoEncoder(path, 25.0, DEV, idx2tag=dict(enumerate(tags)))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rows, processed = run_stream(FrameSource(frames, 25.0), pipe, B, 0, 1, device=DEV, encoder=video,
                                     emotions=K if with_emotions else 0,     # the default row formatter takes no emotions
                                     row=lambda tm, num, names, boxes, shape, emotions=None: tracker_row(tm, num, names, boxes, shape))
        video.close()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert processed == n
        faces_seen[with_emotions] = sum(r.count("celeb_") + r.count("Unknown") for r in rows.values())
        os.remove(path)
        return dt

    for we in (False, True):                       # warm-up: code objects, tune cache, buffers
        stream_pass(we)
    t_plain, t_emo = [], []
    for _ in range(args.passes):                   # alternating, best of
        t_plain.append(stream_pass(False))
        t_emo.append(stream_pass(True))

    # (b) the same lines two ways -----------------------------------------------------------------------------------
    rng = np.random.default_rng(0)
    boxes = [[np.asarray(t[:4], np.float32) for t in tb] for tb in truth]
    ftags = [[[tags[int(i)] for i in rng.integers(0, len(tags), K)] for _ in tb] for tb in truth]
    fprob = [[np.sort(rng.random(K).astype(np.float32))[::-1] for _ in tb] for tb in truth]
    batches = [range(b, min(n, b + B)) for b in range(0, n, B) if b + B <= n] or [range(n)]
    stream = torch.cuda.current_stream()
    jpeg_encode.text_atlas_device(DEV)
    res = {"runs": [], "labels": []}
    same = True
    for rep in range(args.passes + 1):             # the first repetition is the warm-up
        for idx in batches:
            bx, tg, pr = [boxes[i] for i in idx], [ftags[i] for i in idx], [fprob[i] for i in idx]
            pics = {}
            for way in ("runs", "labels"):
                dev = torch.from_numpy(frames[idx.start:idx.stop]).to(DEV)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                lines = jpeg_encode.emotion_lines(bx, tg, pr)
                runs, chars, ends, ops, masks = jpeg_encode.text_runs(lines, atlas=False if way == "runs" else None)
                t_host = time.perf_counter() - t0
                packed = torch.from_numpy(np.concatenate([ops.view(np.uint8), runs.view(np.uint8), masks, chars])).to(DEV)
                a, b = ops.nbytes, ops.nbytes + runs.nbytes
                e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
                e0.record(stream)
                if way == "runs":
                    jpeg_encode.overlay_draw_text(dev, packed[a:b], packed[b + masks.size:], ends)
                else:
                    jpeg_encode.overlay_draw(dev, packed[:a], packed[b:b + masks.size])
                e1.record(stream)
                torch.cuda.synchronize()
                if rep:
                    res[way].append((t_host * 1e3, e0.elapsed_time(e1), len(lines), int(runs.shape[0]), int(ops.shape[0]),
                                     len(ends), int(masks.size + chars.size)))
                pics[way] = dev
            same = same and bool(torch.equal(pics["runs"], pics["labels"]))
    med = lambda way, k: float(np.median([r[k] for r in res[way]]))   # noqa: E731
    fa, fb = n / min(t_plain), n / min(t_emo)
    lines = [
        "# %d synthetic %dx%d frames, 4 pasted faces each, batches of %d; run_stream + VideoEncoder (q92 4:2:0), one GPU, best of %d alternating passes"
        % (n, w, h, B, args.passes),
        "(a) stream without emotions                                        : %8.1f frames/s (%.2f ms per batch), %d faces"
        % (fa, B / fa * 1e3, faces_seen[False]),
        "    stream with FacePipeline(emotion=rn50_2b), emotions=%d, lines drawn : %8.1f frames/s (%.2f ms per batch), %d faces  = %.2f x"
        % (K, fb, B / fb * 1e3, faces_seen[True], fb / fa),
        "(b) the emotion lines of one batch (%d lines: %d frames x 4 faces x %d), medians over %d batches; same pixels both ways: %s"
        % (int(med("runs", 2)), B, K, len(res["runs"]), same),
        "    glyph runs : host table %7.2f ms (%d runs, %d launch(es), %d bytes besides the tables), kernel vnf_overlay_draw_text %7.3f ms"
        % (med("runs", 0), int(med("runs", 3)), int(med("runs", 5)), int(med("runs", 6)), med("runs", 1)),
        "    LABEL masks: host table %7.2f ms (%d ops, Pillow renders each line, %d mask bytes), kernel vnf_overlay_draw      %7.3f ms"
        % (med("labels", 0), int(med("labels", 4)), int(med("labels", 6)), med("labels", 1)),
        "    host %.1f x, kernel %.1f x in favour of the glyph runs" % (med("labels", 0) / med("runs", 0), med("labels", 1) / med("runs", 1)),
    ]
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    os.rmdir(tmp)


if __name__ == "__main__":
    main()
