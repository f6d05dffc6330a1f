#!/usr/bin/env python3
"""Regenerate tests/golden/facenet_aug_ref.npz: transforms_facenet_aug's pixel work (data_loader/__init__.py:58-61) done
by Pillow alone -- Image.rotate(angle, BICUBIC), ImageOps.expand(border, fill=0), Image.crop, Image.transpose
(FLIP_LEFT_RIGHT) -- for fixed draws, on square crops of the PNG pictures under tests/golden/images
(PNG: the input bytes do not depend on a JPEG decoder).  Only the picture's name,
the crop's origin and size, the parameters and the expected bytes are stored; tests cut the input from the picture.

    python tools/make_aug_golden.py [--check]

--check compares a fresh run with the committed file instead of writing it."""
import os
import sys

import numpy as np
from PIL import Image, ImageOps

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, "tests", "golden", "facenet_aug_ref.npz")

# (picture, crop top, crop left, S, T, angle in degrees, crop row i, crop column j, flip)
CASES = [
    ("041bc30432964f95871d4c223eba8f7c.png", 10, 10, 160, 160, 0.0, 2, 2, 0),           # the identity
    ("041bc30432964f95871d4c223eba8f7c.png", 10, 10, 160, 160, -7.3125, 0, 4, 1),
    ("318c7ec3b94b451c813a5665cfcfbda3.png", 21, 0, 160, 160, 9.84375, 4, 0, 0),
    ("33f2891da9694198a67aabd1660517c3.png", 0, 21, 160, 160, -10.0, 3, 1, 1),
    ("318c7ec3b94b451c813a5665cfcfbda3.png", 30, 35, 112, 112, 4.40625, 1, 3, 1),
    ("QuangLe_PhuongMyChi_recog.png", 100, 330, 112, 112, -2.71875, 4, 4, 0),
    ("041bc30432964f95871d4c223eba8f7c.png", 15, 16, 150, 160, 6.5, 0, 5, 0),           # pad_if_needed: border 2 + 6
    ("33f2891da9694198a67aabd1660517c3.png", 31, 0, 150, 160, -9.15625, 6, 3, 1),
]


def load_face(picture, top, left, s):
    im = np.asarray(Image.open(os.path.join(REPO, "tests", "golden", "images", picture)).convert("RGB"))
    if top + s > im.shape[0] or left + s > im.shape[1]:
        raise ValueError("%s is %dx%d: no %d-pixel crop at (%d, %d)" % (picture, im.shape[1], im.shape[0], s, top, left))
    return np.ascontiguousarray(im[top:top + s, left:left + s])


def pillow_case(face, s, t, angle, i, j, flip):
    border = 2 + max(0, t - (s + 4))
    im = Image.fromarray(face).rotate(angle, Image.BICUBIC)
    im = ImageOps.expand(im, border=border, fill=0).crop((j, i, j + t, i + t))
    if flip:
        im = im.transpose(Image.FLIP_LEFT_RIGHT)
    return np.asarray(im)


def build():
    data = {"picture": np.array([c[0] for c in CASES]),
            "origin": np.array([[c[1], c[2]] for c in CASES], np.int32),
            "s": np.array([c[3] for c in CASES], np.int32), "t": np.array([c[4] for c in CASES], np.int32),
            "angle": np.array([c[5] for c in CASES], np.float64),
            "i": np.array([c[6] for c in CASES], np.int32), "j": np.array([c[7] for c in CASES], np.int32),
            "flip": np.array([c[8] for c in CASES], np.int32)}
    for k, (pic, top, left, s, t, angle, i, j, flip) in enumerate(CASES):
        data["out_%d" % k] = pillow_case(load_face(pic, top, left, s), s, t, angle, i, j, flip)
    return data


if __name__ == "__main__":
    new = build()
    if "--check" in sys.argv:
        old = np.load(OUT)
        bad = [k for k in new if not np.array_equal(old[k], new[k])]
        print("differs: %s" % bad if bad else "identical (%d arrays)" % len(new))
        sys.exit(1 if bad else 0)
    np.savez_compressed(OUT, **new)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))
