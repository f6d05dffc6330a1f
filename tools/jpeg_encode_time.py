#!/usr/bin/env python3
"""Frames per second of the two ways an annotated frame leaves the GPU as a Motion-JPEG frame, from one process on one
GPU:

  (a) the host path of demo_video.py -sfr -ov: the frame decoded again on the host (jpeg.HostFrame), boxes and names
      drawn with Pillow (cli_utils.draw_boxes_on_image), a PNG written and read back, Pillow's JPEG encoder -- serial;
  (b) the device path of -ov without -sfr: jpeg_encode.draw_boxes_device + jpeg_encode.BatchEncoder on the frames in
      HBM (overlay, colour, down-sampling, DCT and quantisation in HIP, one D2H copy of the coefficients, the Huffman
      pass on host threads);
  (c) what (b) is made of: the host entropy pass (per frame on one thread, and per batch across the pool) and the
      kernels' time per batch from HIP events;
  (d) the kernels' bytes (RGB in, planes out and in again, coefficients out) over their time, as a fraction of the
      6.29 TB/s device copy rate;
  (e) the device path with the Huffman pass on the device as well (BatchEncoder(entropy="device"),
      csrc/jpeg_huff_device.hip) against (b), the two alternating inside one run: frames per second of both, the
      Huffman kernels' time per batch from HIP events, the bytes per frame each copies to the host, and whether the two
      wrote identical files.  --entropy_out writes this leg to a file of its own; --only_entropy skips (a) to (d).

Input: 64 synthetic 1080p frames (synth.make_frames) with their pasted faces' rectangles as boxes, batches of 16.  Both
paths end in the same JPEG files (checked on every frame of the warm-up pass).

    python tools/jpeg_encode_time.py [--frames 64] [--batch 16] [--passes 3] [--out profiles/jpeg_encode_time.txt]
    python tools/jpeg_encode_time.py --only_entropy --entropy_out profiles/jpeg_huff_device_time.txt
"""
import argparse
import io
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from vn_celeb_face_recognition_amd import jpeg, jpeg_encode  # noqa: E402
from vn_celeb_face_recognition_amd.cli_utils import draw_boxes_on_image, read_rgb, write_rgb  # noqa: E402
from vn_celeb_face_recognition_amd.synth import make_frames  # noqa: E402

DEV = "cuda:0"
COPY_RATE = 6.29e12
QUALITY, SAMPLING = 92, "4:2:0"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--entropy_out", default=None, help="where leg (e) is written")
    ap.add_argument("--only_entropy", action="store_true", help="leg (e) alone")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("jpeg_encode_time.py measures on the MI355X: no GPU is visible")
    from PIL import Image
    n, B = args.frames, args.batch
    frames, truth = make_frames(n, 4)
    boxes = [[[float(v) for v in t[:4]] for t in tb] for tb in truth]
    names = [["celeb_%d" % (7 * i + j) for j in range(len(tb))] for i, tb in enumerate(boxes)]
    tmp = tempfile.mkdtemp()
    # what the stream handed over: the frames as JPEG bytes on the host (jpeg.HostFrame) and as pixels in HBM
    compressed = []
    for f in frames:
        buf = io.BytesIO()
        Image.fromarray(f).save(buf, format="JPEG", quality=QUALITY)
        compressed.append(buf.getvalue())
    shown = [jpeg.decode_host(d) for d in compressed]
    batches = [range(b, min(n, b + B)) for b in range(0, n, B)]
    pristine = [torch.from_numpy(np.stack([shown[i] for i in idx])).to(DEV) for idx in batches]
    work = [p.clone() for p in pristine]
    enc = jpeg_encode.BatchEncoder(DEV, QUALITY, SAMPLING)
    stream = torch.cuda.current_stream()

    def host_pass(keep=None):
        for i in range(n):
            frame = np.asarray(jpeg.HostFrame(compressed[i], shown[i].shape))
            img = draw_boxes_on_image(frame, boxes[i], names[i]) if names[i] else frame
            png = os.path.join(tmp, "frame_%d.png" % (i + 1))
            write_rgb(png, img)
            buf = io.BytesIO()
            Image.fromarray(read_rgb(png)).save(buf, format="JPEG", quality=QUALITY)
            if keep is not None:
                keep.append(buf.getvalue())

    def device_pass(keep=None, timings=None, enc=enc):
        for k, idx in enumerate(batches):
            work[k].copy_(pristine[k])                                  # the overlay paints in place: a fresh batch every pass
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tm = {"events": True} if timings is not None else None
            ops, masks = jpeg_encode.overlay_ops([boxes[i] for i in idx], [names[i] for i in idx])   # host: Pillow renders the names
            t_ops = time.perf_counter() - t0
            packed = torch.from_numpy(np.concatenate([ops.view(np.uint8), masks])).to(DEV)
            if tm is not None:
                e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
                e0.record(stream)
            jpeg_encode.overlay_draw(work[k], packed[:ops.nbytes], packed[ops.nbytes:])
            if tm is not None:
                e1.record(stream)
            job = enc.enqueue(work[k], stream, timing=tm)
            files = enc.finish(job)
            dt = time.perf_counter() - t0
            if tm is not None:
                torch.cuda.synchronize()
                timings.append({"overlay_ms": e0.elapsed_time(e1), "ops_s": t_ops, "n_ops": int(ops.shape[0]), "encode_ms": tm["kernel_events"][0].elapsed_time(tm["kernel_events"][1]),
                                "entropy_s": enc.entropy_s, "info": job["info"], "d2h": enc.d2h_bytes / len(idx),
                                "huff_ms": tm["huff_events"][0].elapsed_time(tm["huff_events"][1]) if "huff_events" in tm else 0.0})
            if keep is not None:
                keep.extend(files)
            yield dt

    def entropy_leg():
        dev_enc = jpeg_encode.BatchEncoder(DEV, QUALITY, SAMPLING, entropy="device")
        fh, fd = [], []
        list(device_pass(fh))                       # warm-up of both back ends, and the equality check
        list(device_pass(fd, enc=dev_enc))
        th, td, mh, md = [], [], [], []
        for _ in range(args.passes):                # alternating: both see the same machine
            th.append(sum(device_pass()))
            td.append(sum(device_pass(enc=dev_enc)))
        list(device_pass(timings=mh))
        list(device_pass(timings=md, enc=dev_enc))
        full = slice(0, max(1, len(md) - (1 if n % B else 0)))
        info = md[0]["info"]
        med = lambda rows, key: float(np.median([t[key] for t in rows[full]]))
        rh, rd = n / min(th), n / min(td)
        return [
            "# (e) %d synthetic %dx%d annotated frames, quality %d %s (%.0f KB per frame), batches of %d, best of %d passes, the two back ends alternating"
            % (n, info.width, info.height, QUALITY, SAMPLING, sum(len(d) for d in fd) / n / 1e3, B, args.passes),
            "# both back ends wrote the same JPEG files for every frame: %s" % (fh == fd),
            "(e) entropy=host    kernels, D2H of coefficients, Huffman pass on %d host threads            : %8.1f frames/s (%.2f ms per batch)"
            % (jpeg_encode.ENTROPY_THREADS, rh, B / rh * 1e3),
            "    entropy=device  kernels, Huffman kernels, D2H of the files                              : %8.1f frames/s (%.2f ms per batch)  = %.2f x host"
            % (rd, B / rd * 1e3, rd / rh),
            "    Huffman kernels (HIP events, memset + 6 launches): %.3f ms per batch of %d (%.1f us per frame); encode kernels %.3f ms"
            % (med(md, "huff_ms"), B, med(md, "huff_ms") * 1e3 / B, med(md, "encode_ms")),
            "    host time behind the kernels: entropy=host %.2f ms per batch (threaded Huffman pass), entropy=device %.2f ms (wait, copy of the files)"
            % (med(mh, "entropy_s") * 1e3, med(md, "entropy_s") * 1e3),
            "    D2H bytes per frame: entropy=host %.2f MB (coefficients), entropy=device %.2f MB (the file and its table entry)"
            % (med(mh, "d2h") / 1e6, med(md, "d2h") / 1e6),
        ]

    def write(path, text):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as f:
                f.write(text + "\n")

    if args.only_entropy:
        text = "\n".join(entropy_leg())
        print(text)
        write(args.entropy_out, text)
        os.rmdir(tmp)
        return
    ha, da = [], []
    host_pass(ha)                                   # warm-up of both paths, and the equality check
    list(device_pass(da))
    same = ha == da
    ta, tb, tms = [], [], []
    for _ in range(args.passes):
        t0 = time.perf_counter()
        host_pass()
        ta.append(time.perf_counter() - t0)
        tb.append(sum(device_pass()))               # without the restore copy of this benchmark's own batches
    list(device_pass(timings=tms))                  # a pass with HIP events around the kernels
    info = tms[0]["info"]
    cc = int(info.coef_count)
    coefs = [np.zeros(cc, np.int16) for _ in range(min(n, 16))]
    for i, c in enumerate(coefs):
        assert jpeg.entropy_decode(da[i], jpeg.probe(da[i])[1], c) == 0
    t0 = time.perf_counter()
    for c in coefs:
        jpeg_encode.entropy_encode(c, info)
    ent_one = (time.perf_counter() - t0) / len(coefs)
    fa, fb = n / min(ta), n / min(tb)
    full = tms[:max(1, len(tms) - (1 if n % B else 0))]      # a short last batch does not speak for a batch of B
    ent_b = float(np.median([t["entropy_s"] for t in full]))
    ov_ms = float(np.median([t["overlay_ms"] for t in full]))
    ops_ms = float(np.median([t["ops_s"] for t in full])) * 1e3
    en_ms = float(np.median([t["encode_ms"] for t in full]))
    rgb = info.width * info.height * 3
    per_frame = rgb + cc + cc + cc * 2
    lines = [
        "# %d synthetic %dx%d annotated frames (%d boxes with names), Motion-JPEG quality %d %s (%.0f KB per frame), batches of %d, best of %d passes"
        % (n, info.width, info.height, sum(len(b) for b in boxes), QUALITY, SAMPLING, sum(len(d) for d in da) / n / 1e3, B, args.passes),
        "# both paths wrote the same JPEG files for every frame: %s" % same,
        "(a) host path   HostFrame decode + Pillow draw + PNG write + PNG read + Pillow JPEG, serial : %8.1f frames/s (%.2f ms per frame)"
        % (fa, 1e3 / fa),
        "(b) device path draw_boxes_device + BatchEncoder (kernels, D2H of coefficients, entropy)    : %8.1f frames/s (%.2f ms per frame)  = %.2f x (a)"
        % (fb, 1e3 / fb, fb / fa),
        "(c) host entropy encode: %.2f ms per frame on one thread; %.2f ms per batch of %d across %d threads (%.2f ms per frame)"
        % (ent_one * 1e3, ent_b * 1e3, B, jpeg_encode.ENTROPY_THREADS, ent_b * 1e3 / B),
        "    the entropy pass is %.0f %% of (b)'s time per batch (%.2f ms)" % (100 * ent_b / (B / fb), B / fb * 1e3),
        "    overlay table on the host (Pillow renders the label masks): %.2f ms per batch (%d entries)" % (ops_ms, full[0]["n_ops"]),
        "    kernels (HIP events): overlay %.3f ms, colour/down-sample + FDCT/quantise %.3f ms per batch of %d (%.1f us per frame)"
        % (ov_ms, en_ms, B, en_ms * 1e3 / B),
        "(d) encode kernel bytes per frame: %.2f MB RGB + %.2f MB planes out + %.2f MB planes in + %.2f MB coefficients = %.2f MB;"
        % (rgb / 1e6, cc / 1e6, cc / 1e6, cc * 2 / 1e6, per_frame / 1e6),
        "    %.2f TB/s = %.1f %% of the 6.29 TB/s copy rate" % (per_frame * B / (en_ms * 1e-3) / 1e12, 100 * per_frame * B / (en_ms * 1e-3) / COPY_RATE),
    ]
    text = "\n".join(lines)
    print(text)
    write(args.out, text)
    leg_e = "\n".join(entropy_leg())
    print(leg_e)
    write(args.entropy_out, leg_e)
    for i in range(n):
        os.remove(os.path.join(tmp, "frame_%d.png" % (i + 1)))
    os.rmdir(tmp)


if __name__ == "__main__":
    main()
