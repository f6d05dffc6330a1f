#!/usr/bin/env python3
"""Frames per second of the two ways a Motion-JPEG stream reaches HBM, from one process on one GPU:

  (a) the host path: mjpeg_avi.MjpegFrames[i] (Pillow, serial) + upload.FrameUploader.upload, batch by batch;
  (b) the device path: jpeg.decode_batch_device (entropy decode on host threads, IDCT / upsampling / colour in HIP);
  (c) what (b) is made of: the host entropy pass (per frame on one thread, and per batch across the pool) and the two
      kernels' time per batch from HIP events;
  (d) the kernels' bytes (coefficients + tables in, planes out and in again, RGB out) over their time, as a fraction of
      the 6.29 TB/s device copy rate.

Input: 64 synthetic 1080p frames (synth.make_frames) written as a quality-92 4:2:0 Motion-JPEG AVI, batches of 16.
Both paths end in the same bytes (checked on every batch of the warm-up pass).

    python tools/jpeg_time.py [--frames 64] [--batch 16] [--passes 3] [--out profiles/jpeg_decode_time.txt]
"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from vn_celeb_face_recognition_amd import jpeg  # noqa: E402
from vn_celeb_face_recognition_amd.mjpeg_avi import read_mjpeg_avi, write_mjpeg_avi  # noqa: E402
from vn_celeb_face_recognition_amd.synth import make_frames  # noqa: E402
from vn_celeb_face_recognition_amd.upload import FrameUploader  # noqa: E402

DEV = "cuda:0"
COPY_RATE = 6.29e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("jpeg_time.py measures on the MI355X: no GPU is visible")
    n, B = args.frames, args.batch
    tmp = tempfile.mkdtemp()
    avi = os.path.join(tmp, "clip.avi")
    write_mjpeg_avi(avi, make_frames(n, 8)[0], 25.0, quality=92)
    _, frames, _ = read_mjpeg_avi(avi)
    batches = [range(b, min(n, b + B)) for b in range(0, n, B)]
    up = FrameUploader(DEV, depth=3)

    def host_pass(check=None):
        for idx in batches:
            dev, ev = up.upload([frames[i] for i in idx])
            if check is not None:
                ev.synchronize()
                check.append(dev.cpu().numpy())
            up.release(up.last_slot, ev)
        torch.cuda.synchronize()

    def device_pass(check=None, timings=None):
        for idx in batches:
            tm = {"events": True} if timings is not None else None
            r = jpeg.decode_batch_device([frames.compressed(i) for i in idx], DEV, up, timing=tm)
            if r is None:
                raise SystemExit("the device decoder refused a batch of its own benchmark")
            if check is not None:
                r[1].synchronize()
                check.append(r[0].cpu().numpy())
            if timings is not None:
                timings.append(tm)
            up.release(r[2], r[1])
        torch.cuda.synchronize()

    ha, da = [], []
    host_pass(ha)                                   # warm-up of both paths (pinned + device rings), and the equality check
    device_pass(da)
    same = all(np.array_equal(x, y) for x, y in zip(ha, da))
    del ha, da
    ta, tb, tms = [], [], []
    for _ in range(args.passes):
        t0 = time.perf_counter()
        host_pass()
        ta.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        device_pass()
        tb.append(time.perf_counter() - t0)
    device_pass(timings=tms)                        # a pass with HIP events around the kernels
    kern_ms = [t["kernel_events"][0].elapsed_time(t["kernel_events"][1]) for t in tms]
    ent_batch = [t["entropy_s"] for t in tms]
    # one frame's entropy decode on one thread
    d0 = frames.compressed(0)
    rc, info = jpeg.probe(d0)
    co = np.zeros(info.coef_count, np.int16)
    t0 = time.perf_counter()
    for i in range(min(n, 16)):
        jpeg.entropy_decode(frames.compressed(i), info, co)
    ent_one = (time.perf_counter() - t0) / min(n, 16)
    fa, fb = n / min(ta), n / min(tb)
    cc = int(info.coef_count)
    per_frame = cc * 2 + 192 + cc + cc + info.width * info.height * 3
    kb = float(np.median(kern_ms)) * 1e-3
    ent_b = float(np.median(ent_batch))
    lines = [
        "# %d synthetic %dx%d frames, Motion-JPEG quality 92 4:2:0 (%.0f KB per frame), batches of %d, best of %d passes"
        % (n, info.width, info.height, sum(len(frames.compressed(i)) for i in range(n)) / n / 1e3, B, args.passes),
        "# both paths gave the same bytes on every batch: %s" % same,
        "(a) host path   MjpegFrames[i] serial + FrameUploader.upload : %8.1f frames/s (%.2f ms per frame)" % (fa, 1e3 / fa),
        "(b) device path jpeg.decode_batch_device                     : %8.1f frames/s (%.2f ms per frame)  = %.2f x (a)"
        % (fb, 1e3 / fb, fb / fa),
        "(c) host entropy decode: %.2f ms per frame on one thread; %.2f ms per batch of %d across %d threads (%.2f ms per frame)"
        % (ent_one * 1e3, ent_b * 1e3, B, jpeg.ENTROPY_THREADS, ent_b * 1e3 / B),
        "    the entropy pass is %.0f %% of (b)'s time per batch (%.2f ms)" % (100 * ent_b / (B / fb), B / fb * 1e3),
        "    kernels (IDCT + upsample/colour, HIP events): %.3f ms per batch of %d (%.1f us per frame)" % (kb * 1e3, B, kb * 1e6 / B),
        "(d) kernel bytes per frame: %.2f MB coefficients + %.2f MB planes out + %.2f MB planes in + %.2f MB RGB = %.2f MB;"
        % (cc * 2 / 1e6, cc / 1e6, cc / 1e6, info.width * info.height * 3 / 1e6, per_frame / 1e6),
        "    %.2f TB/s = %.1f %% of the 6.29 TB/s copy rate" % (per_frame * B / kb / 1e12, 100 * per_frame * B / kb / COPY_RATE),
    ]
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    up.close()
    os.remove(avi)
    os.rmdir(tmp)


if __name__ == "__main__":
    main()
