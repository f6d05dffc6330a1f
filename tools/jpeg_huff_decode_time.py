#!/usr/bin/env python3
"""Frames per second of jpeg.decode_batch_device with the Huffman decode on host threads (entropy="host", the default)
and on the device (entropy="device", csrc/jpeg_huff_decode.hip), from one process on one GPU, the two alternating:

  (a) entropy="host":   entropy decode on the thread pool, the int16 coefficients cross the bus;
  (b) entropy="device": vnf_jpeg_huff_prepare on the thread pool, the compressed frames cross, Huffman decode in HIP;
  (c) what (b) is made of: the host prepare pass per batch, the Huffman kernels' time per batch from HIP events, and the
      IDCT / colour kernels behind them;
  (d) bytes uploaded per frame on both paths;
  (e) the Huffman kernels' time per batch over a sweep of subseq_bits.

Input: the 64 synthetic 1080p frames of tools/jpeg_time.py (synth.make_frames) as a quality-92 4:2:0 Motion-JPEG AVI,
batches of 16.  Both paths end in the same bytes (checked on every batch of the warm-up pass).  The yardstick of (b)
is (a) of this same run.

    python tools/jpeg_huff_decode_time.py [--frames 64] [--batch 16] [--passes 3] [--out profiles/jpeg_huff_decode_time.txt]
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
SWEEP = (128, 256, 512, 1024, 2048, 4096)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("jpeg_huff_decode_time.py measures on the MI355X: no GPU is visible")
    n, B = args.frames, args.batch
    tmp = tempfile.mkdtemp()
    avi = os.path.join(tmp, "clip.avi")
    write_mjpeg_avi(avi, make_frames(n, 8)[0], 25.0, quality=92)
    _, frames, _ = read_mjpeg_avi(avi)
    data = [frames.compressed(i) for i in range(n)]
    batches = [data[b:b + B] for b in range(0, n, B)]
    up = FrameUploader(DEV, depth=3)

    def run(entropy, check=None, timings=None, subseq_bits=0):
        for batch in batches:
            tm = {"events": True} if timings is not None else None
            r = jpeg.decode_batch_device(batch, DEV, up, timing=tm, entropy=entropy, subseq_bits=subseq_bits)
            if r is None:
                raise SystemExit("the decoder refused a batch of its own benchmark (entropy=%s)" % entropy)
            if check is not None:
                r[1].synchronize()
                check.append(r[0].cpu().numpy())
            if timings is not None:
                timings.append(tm)
            up.release(r[2], r[1])
        torch.cuda.synchronize()

    ha, da = [], []
    run("host", ha)                                 # warm-up of both paths (pinned + device rings), and the equality check
    run("device", da)
    same = all(np.array_equal(x, y) for x, y in zip(ha, da))
    del ha, da
    t = {"host": [], "device": []}
    for _ in range(args.passes):
        for entropy in ("host", "device"):
            t0 = time.perf_counter()
            run(entropy)
            t[entropy].append(time.perf_counter() - t0)
    tm_h, tm_d = [], []
    run("host", timings=tm_h)                       # a pass each with HIP events around the kernels
    run("device", timings=tm_d)

    def ms(tms, key):
        return float(np.median([x[key][0].elapsed_time(x[key][1]) for x in tms]))

    sweep = []
    for sb in SWEEP:
        tms = []
        run("device", timings=tms, subseq_bits=sb)
        run("device", timings=tms, subseq_bits=sb)
        sweep.append((sb, ms(tms, "huff_events")))
    fa, fb = n / min(t["host"]), n / min(t["device"])
    rc, info = jpeg.probe(data[0])
    lines = [
        "# %d synthetic %dx%d frames, Motion-JPEG quality 92 4:2:0 (%.0f KB per frame), batches of %d, one process, the two"
        % (n, info.width, info.height, sum(len(d) for d in data) / n / 1e3, B),
        "# paths alternating, best of %d passes" % args.passes,
        "# both paths gave the same bytes on every batch: %s" % same,
        "(a) entropy=host   (Huffman decode on %d host threads)   : %8.1f frames/s (%.2f ms per batch)"
        % (jpeg.ENTROPY_THREADS, fa, B / fa * 1e3),
        "(b) entropy=device (prepare on the host, Huffman in HIP) : %8.1f frames/s (%.2f ms per batch)  = %.2f x (a)"
        % (fb, B / fb * 1e3, fb / fa),
        "(c) per batch of %d: host entropy pass of (a) %.2f ms; host prepare pass of (b) %.2f ms;"
        % (B, float(np.median([x["entropy_s"] for x in tm_h])) * 1e3, float(np.median([x["entropy_s"] for x in tm_d])) * 1e3),
        "    Huffman kernels (HIP events, subseq_bits default) %.3f ms; IDCT + upsample/colour kernels behind them %.3f ms (%.3f ms in (a))"
        % (ms(tm_d, "huff_events"), ms(tm_d, "kernel_events"), ms(tm_h, "kernel_events")),
        "(d) uploaded per frame: (a) %.2f MB, (b) %.2f MB = 1 / %.1f"
        % (tm_h[0]["upload_bytes"] / B / 1e6, tm_d[0]["upload_bytes"] / B / 1e6, tm_h[0]["upload_bytes"] / tm_d[0]["upload_bytes"]),
        "(e) Huffman kernels per batch over subseq_bits: " + ", ".join("%d: %.3f ms" % s for s in sweep),
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
