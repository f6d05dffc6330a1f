#!/usr/bin/env python3
"""Regenerate tests/golden/extract_ref.npz by RUNNING THE REFERENCE's MTCNN.forward, extract_face and select_boxes on the
CPU (build machine only: it needs the reference checkout; the shim of tools/make_golden.py stands in for torchvision).

The input is the PNG picture under tests/golden/images alone, so the input bytes do not depend on a JPEG decoder, and it
is handed over as a uint8 tensor: the reference then crops and resamples on its tensor path
(imresample(crop.float(), (S,S)).byte(), detect_face.py:317-322), the one path this project serves.

  forward       keep_all=True at margins 0 and 32 (image_size 160); keep_all=False, margin 14, at sizes 64 and 32:
                boxes, probs, points and the faces as bytes (face * 128 + 127.5, exact)
  extract_face  hand-made float32 boxes to 32 x 32: one hanging over each frame edge, one smaller than the output
  select_boxes  the reference's own detections and a seeded table of 6 boxes: all four methods, single and batch form,
                a PIL picture as the image (center_weighted_size reads .width), a threshold below every probability (so
                that the reference's unfiltered probs / points of largest_over_threshold do not bite)

Only arrays are stored.

    python tools/make_extract_golden.py [--check]

--check compares a fresh run with the committed file instead of writing it."""
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import REPO, install_shim, ref  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "extract_ref.npz")
PICTURE = "QuangLe_PhuongMyChi_recog.png"
MIN_FACE = 30
# (keep_all, margin, image_size)
FORWARD = [(1, 0, 160), (1, 32, 160), (0, 14, 64), (0, 14, 32)]
# (x1, y1, x2, y2, margin) in the 878 x 481 picture, to 32 x 32
EF_SIZE = 32
EXTRACT_FACE = [(-20.5, 100.25, 60.75, 190.5, 0),      # over the left edge
                (300.5, -15.75, 380.25, 70.5, 8),      # over the top edge (and a margin)
                (820.25, 200.5, 900.75, 290.25, 8),    # over the right edge
                (400.75, 420.5, 470.25, 500.75, 0),    # over the bottom edge
                (500.5, 250.25, 521.75, 275.5, 4)]     # 21 x 25 pixels: up-sampling
METHODS = ("probability", "largest", "largest_over_threshold", "center_weighted_size")
SEL_THRESHOLD = 0.3


def synthetic_table(width, height):
    rng = np.random.RandomState(7)
    x1 = rng.uniform(0, width - 200, 6); y1 = rng.uniform(0, height - 200, 6)
    w = rng.uniform(30, 190, 6); h = rng.uniform(30, 190, 6)
    boxes = np.stack([x1, y1, x1 + w, y1 + h], axis=1).astype(np.float32)
    probs = rng.uniform(0.5, 1.0, 6).astype(np.float32)
    points = (boxes[:, None, :2] + rng.uniform(0, 1, (6, 5, 2)) * np.stack([w, h], axis=1)[:, None, :]).astype(np.float32)
    return boxes, probs, points


def build():
    from PIL import Image
    install_shim()
    mt = ref("mtcnn")
    df = ref("mtcnn_utils.detect_face")
    pil = Image.open(os.path.join(REPO, "tests", "golden", "images", PICTURE)).convert("RGB")
    img = torch.from_numpy(np.asarray(pil).copy())
    data = {"picture": np.array(PICTURE), "min_face_size": np.int32(MIN_FACE), "forward": np.array(FORWARD, np.int32)}
    for k, (keep_all, margin, size) in enumerate(FORWARD):
        det = mt.MTCNN(image_size=size, margin=margin, keep_all=bool(keep_all), min_face_size=MIN_FACE, device="cpu").eval()
        with torch.no_grad():
            faces, boxes, probs = det(img, return_prob=True)
        _, _, points = det.detect(img, landmarks=True)
        if not keep_all:
            _, _, points = det.select_boxes(*det.detect(img, landmarks=True), img, method=det.selection_method)
        n = len(boxes)
        u8 = (faces.reshape(n, 3, size, size) * 128.0 + 127.5).numpy()
        assert np.array_equal(u8, np.round(u8)) and u8.min() >= 0 and u8.max() <= 255
        data["fwd_%d/boxes" % k] = np.asarray(boxes, np.float32).reshape(n, 4)
        data["fwd_%d/probs" % k] = np.asarray(probs, np.float32).reshape(n)
        data["fwd_%d/points" % k] = np.asarray(points, np.float32).reshape(n, 5, 2)
        data["fwd_%d/faces" % k] = u8.astype(np.uint8)
        print("forward keep_all=%d margin=%d size=%d -> %d faces" % (keep_all, margin, size, n))
    ef = np.array(EXTRACT_FACE, np.float32)
    data["ef/boxes"], data["ef/margin"], data["ef/size"] = ef[:, :4].copy(), ef[:, 4].astype(np.int32), np.int32(EF_SIZE)
    out = []
    for row in ef:
        face = df.extract_face(img, row[:4], EF_SIZE, int(row[4])).numpy()
        assert np.array_equal(face, np.round(face))
        out.append(face.astype(np.uint8))
    data["ef/faces"] = np.stack(out)
    det = mt.MTCNN(keep_all=True, min_face_size=MIN_FACE, device="cpu").eval()
    tables = {"det": tuple(np.asarray(a, np.float32) for a in det.detect(img, landmarks=True)),
              "syn": synthetic_table(*pil.size)}
    data["sel/threshold"] = np.float64(SEL_THRESHOLD)
    for name, (b, p, q) in tables.items():
        data["sel/%s/boxes" % name], data["sel/%s/probs" % name], data["sel/%s/points" % name] = b, p, q
        for m in METHODS:
            sb, sp, sq = det.select_boxes(b, p, q, pil, method=m, threshold=SEL_THRESHOLD)
            data["sel/%s/%s/box" % (name, m)] = np.asarray(sb, np.float32)
            data["sel/%s/%s/prob" % (name, m)] = np.float32(sp)
            data["sel/%s/%s/point" % (name, m)] = np.asarray(sq, np.float32)
    for m in METHODS:        # batch form: [det, syn] on two copies of the picture
        sb, sp, sq = det.select_boxes([tables["det"][0], tables["syn"][0]], [tables["det"][1], tables["syn"][1]],
                                      [tables["det"][2], tables["syn"][2]], [pil, pil], method=m, threshold=SEL_THRESHOLD)
        data["sel/batch/%s/box" % m] = np.asarray(sb, np.float32)
        data["sel/batch/%s/prob" % m] = np.asarray(sp, np.float32)
        data["sel/batch/%s/point" % m] = np.asarray(sq, np.float32)
    return data


if __name__ == "__main__":
    new = build()
    if "--check" in sys.argv:
        old = np.load(OUT)
        bad = [k for k in new if k not in old or not np.array_equal(old[k], new[k])]
        print("differs: %s" % bad if bad else "identical (%d arrays)" % len(new))
        sys.exit(1 if bad else 0)
    np.savez_compressed(OUT, **new)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))
