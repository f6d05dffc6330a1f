#!/usr/bin/env python3
"""Writes tests/golden/jpeg_cases.npz: small JPEG files encoded by Pillow and the RGB bytes Pillow decodes from them,
the expected output of the native decoder (csrc/jpeg_entropy.cpp + csrc/jpeg_decode.hip), which has to match with zero
differing bytes.  The Pillow and libjpeg-turbo versions that produced the file are recorded inside it.

    python tools/make_jpeg_golden.py

The grid: sizes 1x1, 8x8, 17x13, 33x47, 64x48 (a single partial MCU, odd chroma width and height, more than one MCU
row) x 4:4:4 / 4:2:2 / 4:2:0 / grayscale at quality 75; quality 30, 92 and 100, optimize=True and restart markers (every
3 blocks, every MCU row) on 33x47 for every sampling and on 17x13 for 4:2:0; one uniform-noise image at quality 95; a
progressive and a CMYK file, which the decoder must leave to the host ("not taken")."""
import io
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(1, 1), (8, 8), (17, 13), (33, 47), (64, 48)]
SUB = {"444": 0, "422": 1, "420": 2}


def picture(w, h, seed, noise=False):
    rng = np.random.default_rng(seed)
    if noise:
        return rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    img = np.stack([128 + 100 * np.sin(xx / 5.0 + c) * np.cos(yy / 7.0 - c) for c in range(3)], axis=-1)
    img += rng.normal(0, 12, size=img.shape)
    img[h // 3:h // 3 + 3, :, 0] = 255          # saturated primaries next to each other: sharp chroma edges, clamping
    img[:, w // 2:w // 2 + 2, 1] = 0
    img[h // 2:, w // 4:w // 4 + 1, 2] = 255
    return np.clip(img, 0, 255).astype(np.uint8)


def main():
    import PIL
    from PIL import Image, features
    cases, arrays = [], {}

    def add(name, img, expect="ok", **kw):
        buf = io.BytesIO()
        img.save(buf, format="JPEG", **kw)
        data = buf.getvalue()
        i = len(cases)
        arrays["jpg_%d" % i] = np.frombuffer(data, np.uint8)
        if expect == "ok":
            arrays["rgb_%d" % i] = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
        cases.append(dict(name=name, width=img.size[0], height=img.size[1], mode=img.mode, expect=expect,
                          params={k: v for k, v in kw.items()}))

    seed = 0
    for (w, h) in SIZES:
        rgb = Image.fromarray(picture(w, h, seed))
        seed += 1
        for s, code in SUB.items():
            add("%dx%d_%s_q75" % (w, h, s), rgb, quality=75, subsampling=code)
        add("%dx%d_gray_q75" % (w, h), rgb.convert("L"), quality=75)
    for (w, h) in [(17, 13), (33, 47)]:
        rgb = Image.fromarray(picture(w, h, seed))
        seed += 1
        for q in (30, 92, 100):
            for s, code in SUB.items():
                if w == 17 and s != "420":
                    continue                     # the full sampling x quality grid on one size is enough
                add("%dx%d_%s_q%d" % (w, h, s, q), rgb, quality=q, subsampling=code)
            add("%dx%d_gray_q%d" % (w, h, q), rgb.convert("L"), quality=q)
        for s, code in SUB.items():
            if w == 17 and s != "420":
                continue
            add("%dx%d_%s_opt" % (w, h, s), rgb, quality=85, subsampling=code, optimize=True)
            add("%dx%d_%s_rstb3" % (w, h, s), rgb, quality=85, subsampling=code, restart_marker_blocks=3)
            add("%dx%d_%s_rstr1" % (w, h, s), rgb, quality=85, subsampling=code, restart_marker_rows=1)
        add("%dx%d_gray_rstb3" % (w, h), rgb.convert("L"), quality=85, restart_marker_blocks=3)
    add("64x48_420_noise_q95", Image.fromarray(picture(64, 48, 99, noise=True)), quality=95, subsampling=2)
    small = Image.fromarray(picture(33, 47, 7))
    add("33x47_progressive", small, expect="not_taken", quality=85, progressive=True)
    try:
        add("33x47_cmyk", small.convert("CMYK"), expect="not_taken", quality=85)
    except (OSError, ValueError, KeyError) as e:
        print("this Pillow does not write CMYK JPEG (%s): case dropped" % e, file=sys.stderr)
    versions = {"pillow": PIL.__version__, "libjpeg_turbo": features.version("libjpeg_turbo") or features.version("jpg")}
    arrays["meta"] = np.frombuffer(json.dumps({"versions": versions, "cases": cases}).encode(), np.uint8)
    out = os.path.join(REPO, "tests", "golden", "jpeg_cases.npz")
    np.savez_compressed(out, **arrays)
    print("%d cases, %d bytes, Pillow %s, libjpeg-turbo %s -> %s" % (len(cases), os.path.getsize(out), versions["pillow"],
                                                                      versions["libjpeg_turbo"], out))


if __name__ == "__main__":
    main()
