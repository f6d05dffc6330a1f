#!/usr/bin/env python3
"""Device time of vnf_extract_faces (MTCNN.extract's kernel) against the bytes the algorithm needs -- the crops' bytes read
once plus the fp32 NCHW output written -- and, from the same process, the cascade's crop_resize_48 stage
(MTCNN.stage_times), the kernel it is built like.  Two workloads, both to 160 x 160, standardised fp32 output:

  frames16x4   16 frames of 1920x1080, 4 boxes of about 200 px on each (64 faces, the detector's batch)
  one64x256    64 boxes of 256 px on one 1920x1080 frame

The rectangle table is already on the device; HIP events surround `--reps` back-to-back launches after a warm-up, so the
time is the kernel's (launch gaps included, which is what a caller sees).  Fractions are of the 8 TB/s HBM3E peak.

    python tools/extract_time.py [--reps 200] [--out profiles/extract_time.txt]
"""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from vn_celeb_face_recognition_amd import _lib  # noqa: E402
from vn_celeb_face_recognition_amd.models import MTCNN  # noqa: E402
from vn_celeb_face_recognition_amd.synth import make_frames  # noqa: E402

DEV = "cuda:0"
HBM_PEAK = 8.0e12
H, W, S = 1080, 1920, 160


def workloads():
    rng = np.random.RandomState(3)
    a = []
    for f in range(16):
        for _ in range(4):
            side = int(rng.randint(180, 221))
            x1, y1 = int(rng.randint(0, W - side)), int(rng.randint(0, H - side))
            a.append((f, x1, y1, x1 + side, y1 + side))
    b = []
    for _ in range(64):
        x1, y1 = int(rng.randint(0, W - 256)), int(rng.randint(0, H - 256))
        b.append((0, x1, y1, x1 + 256, y1 + 256))
    return [("frames16x4", 16, np.array(a, np.int32)), ("one64x256", 1, np.array(b, np.int32))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("extract_time.py measures on the MI355X: no GPU is visible")
    lib, stream = _lib.load(), _lib.current_stream_ptr()
    g = torch.Generator().manual_seed(9)
    noise = torch.randint(0, 256, (16, H, W, 3), generator=g, dtype=torch.uint8).to(DEV)
    lines = ["# vnf_extract_faces to %dx%d fp32 standardised, 1920x1080 frames, %d launches after 20 warm-up" % (S, S, args.reps),
             "# workload faces | us per launch | crop MB + output MB | algorithmic GB/s | of 8 TB/s HBM peak"]
    frac = {}
    for name, nb, rects in workloads():
        n = len(rects)
        rdev = torch.from_numpy(rects).to(DEV)
        x = torch.empty((n, 3, S, S), dtype=torch.float32, device=DEV)
        call = (ctypes.c_void_p(noise.data_ptr()), nb, H, W, ctypes.c_void_p(rdev.data_ptr()), n, S, 1,
                ctypes.c_void_p(x.data_ptr()), _lib.VNF_F32, None, stream)
        for _ in range(20):
            _lib.check(lib.vnf_extract_faces(*call))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(args.reps):
            lib.vnf_extract_faces(*call)
        e1.record()
        torch.cuda.synchronize()
        t = e0.elapsed_time(e1) * 1e-3 / args.reps
        crop = int(((rects[:, 3] - rects[:, 1]).astype(np.int64) * (rects[:, 4] - rects[:, 2]) * 3).sum())
        out = n * 3 * S * S * 4
        frac[name] = (crop + out) / t / HBM_PEAK
        lines.append("%-10s %5d | %13.1f | %7.2f + %6.2f | %16.1f | %6.2f %%" %
                     (name, n, t * 1e6, crop / 1e6, out / 1e6, (crop + out) / t / 1e9, 100 * frac[name]))
    # the cascade's stage on frames with faces (synthetic portraits: the stage's work depends on the candidates)
    frames = torch.from_numpy(make_frames(16, 4, H, W)[0]).to(DEV)
    det = MTCNN(keep_all=True, min_face_size=50, device=DEV, max_batch=16, max_height=H, max_width=W)
    det.detect_device(frames)
    st = det.stage_times(frames, reps=7)["crop_resize_48"]
    f48 = st["bytes"] / (st["ms"] * 1e-3) / HBM_PEAK
    lines.append("crop_resize_48 (MTCNN.stage_times, 16 synthetic 1080p frames): %.1f us, %.2f MB algorithmic, %.1f GB/s, %.2f %% of peak"
                 % (st["ms"] * 1e3, st["bytes"] / 1e6, st["bytes"] / (st["ms"] * 1e-3) / 1e9, 100 * f48))
    low = [k for k, v in frac.items() if v < f48]
    if low:
        lines.append("# %s below crop_resize_48's fraction: one launch of 64 faces moves a few MB, so the launch and the ramp of its "
                     "few hundred workgroups are a large part of the microseconds above; the crops' pieces start at the crop's "
                     "first byte, so most 16-byte loads straddle two 16-byte granules (that is what serves every x1 and row pitch "
                     "with one path); and a wave holds one output row, so a 200-px crop keeps 38 of 64 lanes loading" % ", ".join(low))
    else:
        lines.append("# both workloads reach at least crop_resize_48's fraction of the HBM peak")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
