"""Annotated video frames encoded on the device (include/vnface.h, "JPEG video frames, written" and "frame overlay").

The reference draws boxes and names on every frame with OpenCV and hands the frame to cv2.VideoWriter
(/root/reference/demo_video.py:25-43,149-152); this package decoded the frame again on the host, drew with Pillow, wrote a
PNG and, after the run, read every PNG back to JPEG-encode it on one thread.  Here the frame stays where the detector
read it:

  * boxes and names are painted in place by one launch (csrc/overlay.hip; `overlay_ops` builds its table -- the label
    masks are rendered by Pillow's own font code, so the glyphs are Pillow's);
  * colour conversion, chroma down-sampling, forward DCT and quantisation run on the MI355X (csrc/jpeg_encode.hip);
  * one D2H copy brings the coefficients (not the pixels) into pinned memory, and the serial Huffman pass
    (csrc/jpeg_huff_encode.cpp) runs on a few host threads, one frame each (ctypes releases the GIL);
  * or, with entropy="device", the Huffman pass runs on the MI355X as well (csrc/jpeg_huff_device.hip) and only the
    finished files cross to the host.  It writes the same bytes; "host" is the default.

The files are libjpeg's (and so Pillow's `save(format="JPEG", quality=q, subsampling=s)`) byte for byte.
"""
import ctypes
import math
import os
import struct
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from . import _lib
from .jpeg import S420, S422, S444

SAMPLINGS = {"4:4:4": S444, "4:2:2": S422, "4:2:0": S420}
ENTROPY = ("host", "device")                    # where the Huffman pass runs; both write the same files
ENTROPY_THREADS = 8                             # fixed: the frames of a batch, never sized from the machine's CPU count
RECT, LABEL = 0, 1                              # VNF_OVERLAY_*
GREEN = (0, 255, 0)                             # cli_utils.draw_boxes_on_image
OP_DTYPE = np.dtype([("kind", "<i4"), ("frame", "<i4"), ("x0", "<i4"), ("y0", "<i4"), ("x1", "<i4"), ("y1", "<i4"),
                     ("mask_offset", "<i4"), ("rgb", "<u4")])          # vnf_overlay_op
_COORD = 1 << 30                                # table coordinates are clamped here: far outside any frame either way
ENCODE_STREAM_ROLE = 8                          # streams.side_stream roles: 0..5 the pipeline's, 6 upload, 7 collective

_pool = None


def _entropy_pool():
    global _pool
    if _pool is None:
        _pool = ThreadPoolExecutor(max_workers=ENTROPY_THREADS, thread_name_prefix="vnf-jpeg-enc")
    return _pool


def sampling_code(sampling):
    if sampling in SAMPLINGS:
        return SAMPLINGS[sampling]
    if sampling in SAMPLINGS.values():
        return int(sampling)
    raise ValueError("sampling must be one of %s, got %r" % (", ".join(SAMPLINGS), sampling))


def entropy_mode(entropy):
    if entropy not in ENTROPY:
        raise ValueError("entropy must be one of %s, got %r" % (", ".join(ENTROPY), entropy))
    return entropy


def quant_tables(quality):
    """(2,64) u8: libjpeg's luma and chroma tables for `quality` (1..100), natural order"""
    out = np.zeros((2, 64), np.uint8)
    _lib.check(_lib.load().vnf_jpeg_quant_tables(int(quality), out[0].ctypes.data, out[1].ctypes.data))
    return out


def encode_info(width, height, sampling, quality):
    """the JpegInfo of a (height,width,3) RGB frame written with this sampling and quality"""
    info = _lib.JpegInfo()
    _lib.check(_lib.load().vnf_jpeg_encode_info(int(width), int(height), sampling_code(sampling), int(quality),
                                                ctypes.byref(info)))
    return info


def entropy_encode(coefs, info):
    """Huffman-encode one frame's coefficients (C-contiguous int16, info.coef_count of them) -> the JPEG file's bytes"""
    if coefs.dtype != np.int16 or not coefs.flags.c_contiguous or coefs.size < info.coef_count:
        raise ValueError("entropy_encode: coefs must be a contiguous int16 array of at least info.coef_count elements")
    lib = _lib.load()
    cap = 1024 + int(info.coef_count)           # a byte per coefficient covers all but noise at quality 100
    n = ctypes.c_int64()
    for _ in range(2):
        out = np.empty((cap,), np.uint8)
        rc = lib.vnf_jpeg_entropy_encode(coefs.ctypes.data, ctypes.byref(info), out.ctypes.data, cap, ctypes.byref(n))
        if rc == 0:
            return out[:n.value].tobytes()
        if rc != -4:                            # VNF_E_CAPACITY reports the size that fits
            break
        cap = int(n.value)
    raise _lib.VnfError("vnf_jpeg_entropy_encode failed (%d): a coefficient outside the baseline range or a bad info" % rc)


def huff_header(info):
    """the bytes SOI .. end of the SOS header of the file entropy_encode writes for `info` -> (623,) u8"""
    out = np.zeros((1024,), np.uint8)
    n = ctypes.c_int64()
    _lib.check(_lib.load().vnf_jpeg_huff_header(ctypes.byref(info), out.ctypes.data, out.size, ctypes.byref(n)))
    return out[:n.value].copy()


def huff_workspace_bytes(n, info, capacity):
    ws = int(_lib.load().vnf_jpeg_huff_workspace_bytes(int(n), ctypes.byref(info), int(capacity)))
    if ws < 0:
        _lib.check(ws)
    return ws


def huff_encode_frames(coefs_dev, n, info, header_dev, out_dev, capacity, lengths_dev, status_dev, workspace, stream_ptr=None):
    """vnf_jpeg_huff_encode_frames on torch tensors: coefs_dev (n * info.coef_count) int16 cuda as encode_frames leaves
    them; header_dev: huff_header(info) on the device; out_dev: (n * capacity) u8; lengths_dev (n) int64; status_dev
    (n) int32; enqueues on `stream_ptr` (default: the current stream)."""
    ts = (coefs_dev, header_dev, out_dev, lengths_dev, status_dev, workspace)
    if not all(t.is_cuda for t in ts):
        raise RuntimeError("jpeg_encode.huff_encode_frames needs cuda tensors (there is no CPU path)")
    _lib.check(_lib.load().vnf_jpeg_huff_encode_frames(
        coefs_dev.data_ptr(), int(n), ctypes.byref(info), header_dev.data_ptr(), int(header_dev.numel()), out_dev.data_ptr(),
        int(capacity), lengths_dev.data_ptr(), status_dev.data_ptr(), workspace.data_ptr(),
        workspace.numel() * workspace.element_size(), stream_ptr if stream_ptr is not None else _lib.current_stream_ptr()))


def encode_frames(frames_dev, quant_dev, coefs_out, workspace, sampling, stream_ptr=None):
    """vnf_jpeg_encode_frames on torch tensors: frames_dev (n,H,W,3) u8 cuda, contiguous; enqueues on `stream_ptr`
    (default: the current stream)."""
    if not (frames_dev.is_cuda and quant_dev.is_cuda and coefs_out.is_cuda and workspace.is_cuda):
        raise RuntimeError("jpeg_encode.encode_frames needs cuda tensors (there is no CPU path)")
    if frames_dev.dim() != 4 or frames_dev.shape[3] != 3 or not frames_dev.is_contiguous():
        raise ValueError("encode_frames: frames_dev must be a contiguous (n,H,W,3) u8 tensor")
    n, h, w = (int(s) for s in frames_dev.shape[:3])
    _lib.check(_lib.load().vnf_jpeg_encode_frames(
        frames_dev.data_ptr(), n, w, h, sampling_code(sampling), quant_dev.data_ptr(), coefs_out.data_ptr(),
        workspace.data_ptr(), workspace.numel() * workspace.element_size(),
        stream_ptr if stream_ptr is not None else _lib.current_stream_ptr()))
    return coefs_out


class BatchEncoder:
    """Buffers of one (device, quality, sampling, entropy): the tables on the device, and -- grown to the largest batch
    seen -- the coefficient and plane buffers and, with entropy="host", the pinned landing area of the one D2H copy of
    the coefficients; with entropy="device", the Huffman workspace, the files on the device and their pinned landing
    area (no pinned coefficient buffer, and the thread pool is not touched)."""

    def __init__(self, device, quality=92, sampling="4:2:0", entropy="host"):
        import torch
        self.entropy = entropy_mode(entropy)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("BatchEncoder needs a cuda device (there is no CPU path)")
        self.quality, self.sampling = int(quality), sampling_code(sampling)
        self.quant = torch.from_numpy(quant_tables(self.quality)).to(self.device)
        self._coefs = self._ws = self._host = None
        self._hws = self._files = self._table = self._table_host = self._files_host = None
        self._headers = {}                      # (width, height) -> the file header on the device
        self.entropy_s = 0.0                    # host wall time of the last batch's entropy pass: the threaded Huffman
        #                                         pass ("host"), or all of `finish` ("device") (tools)
        self.d2h_bytes = 0                      # what the last batch copied to the host (tools)

    def _grown(self, t, count, dtype, pinned=False):
        import torch
        if t is not None and t.numel() >= count:
            return t
        if pinned:
            return torch.empty((count,), dtype=dtype).pin_memory()
        return torch.empty((count,), dtype=dtype, device=self.device)

    def _huff_enqueue(self, job, capacity, stream):
        """the Huffman kernels for `job` at `capacity` bytes per frame and the copy of the (length, status) table, on
        `stream`, which is the current one"""
        import torch
        n, info = job["n"], job["info"]
        key = (int(info.width), int(info.height))
        if key not in self._headers:
            self._headers[key] = torch.from_numpy(huff_header(info)).to(self.device)
        self._hws = self._grown(self._hws, huff_workspace_bytes(n, info, capacity), torch.uint8)
        self._files = self._grown(self._files, n * capacity, torch.uint8)
        self._table = self._grown(self._table, 2 * n, torch.int64)          # n lengths, then n int32 statuses
        self._table_host = self._grown(self._table_host, 2 * n, torch.int64, pinned=True)
        timed = job.get("timing") is not None and job["timing"].get("events")
        if timed:
            e0 = torch.cuda.Event(enable_timing=True)
            e0.record(stream)
        huff_encode_frames(self._coefs, n, info, self._headers[key], self._files, capacity, self._table[:n],
                           self._table[n:2 * n].view(torch.int32), self._hws, ctypes.c_void_p(stream.cuda_stream))
        if timed:
            e1 = torch.cuda.Event(enable_timing=True)
            e1.record(stream)
            job["timing"]["huff_events"] = (e0, e1)
        self._table_host[:2 * n].copy_(self._table[:2 * n], non_blocking=True)
        job["capacity"] = capacity
        job["copied"] = stream.record_event()

    def enqueue(self, frames_dev, stream=None, timing=None):
        """kernels + the D2H copy of the coefficients (entropy="host") or the Huffman kernels + the D2H copy of the
        files' lengths (entropy="device") on `stream` (default: the current one) -> a handle for `finish`.
        timing: optional dict; with timing["events"] set it receives 'kernel_events' (and 'huff_events'), two timed
        events around the kernels."""
        import torch
        n, h, w = (int(s) for s in frames_dev.shape[:3])
        info = encode_info(w, h, self.sampling, self.quality)
        cc = int(info.coef_count)
        ws = int(_lib.load().vnf_jpeg_encode_workspace_bytes(n, w, h, self.sampling))
        if ws < 0:
            _lib.check(ws)
        stream = stream if stream is not None else torch.cuda.current_stream(self.device)
        job = {"n": n, "cc": cc, "info": info, "stream": stream, "timing": timing}
        with torch.cuda.stream(stream):
            if self._coefs is None or self._coefs.numel() < n * cc:
                self._coefs = torch.empty((n * cc,), dtype=torch.int16, device=self.device)
            if self._ws is None or self._ws.numel() < ws:
                self._ws = torch.empty((ws,), dtype=torch.uint8, device=self.device)
            if self.entropy == "host" and (self._host is None or self._host.numel() < n * cc):
                self._host = torch.empty((n * cc,), dtype=torch.int16).pin_memory()
            if timing is not None and timing.get("events"):
                e0 = torch.cuda.Event(enable_timing=True)
                e0.record(stream)
            encode_frames(frames_dev, self.quant, self._coefs, self._ws, self.sampling, ctypes.c_void_p(stream.cuda_stream))
            if timing is not None and timing.get("events"):
                e1 = torch.cuda.Event(enable_timing=True)
                e1.record(stream)
                timing["kernel_events"] = (e0, e1)
            job["kernels"] = stream.record_event()
            if self.entropy == "host":
                self._host[:n * cc].copy_(self._coefs[:n * cc], non_blocking=True)
                job["copied"] = stream.record_event()
            elif n:
                self._huff_enqueue(job, 1024 + cc, stream)     # a byte per coefficient: entropy_encode's own first guess
        return job

    def finish(self, job):
        """wait for the copy, entropy-encode the frames on the pool -> list of JPEG files (bytes); entropy="device":
        wait for the lengths, copy exactly that many bytes of every file to pinned memory, one synchronise"""
        import time
        if self.entropy == "device":
            t0 = time.perf_counter()
            out = self._finish_device(job)
            self.entropy_s = time.perf_counter() - t0
            return out
        job["copied"].synchronize()
        n, cc, info = job["n"], job["cc"], job["info"]
        host = self._host.numpy()[:n * cc].reshape(n, cc)
        self.d2h_bytes = 2 * n * cc
        t0 = time.perf_counter()
        one = lambda i: entropy_encode(host[i], info)
        out = list(_entropy_pool().map(one, range(n))) if n > 1 else [one(0)]
        self.entropy_s = time.perf_counter() - t0
        return out

    def _finish_device(self, job):
        import torch
        n, stream = job["n"], job["stream"]
        if n == 0:
            return []
        self.d2h_bytes = 0
        for attempt in range(2):
            job["copied"].synchronize()
            self.d2h_bytes += 16 * n
            table = self._table_host.numpy()
            lengths = [int(v) for v in table[:n]]
            status = [int(v) for v in table[n:2 * n].view(np.int32)[:n]]
            bad = [st for st in status if st not in (0, -4)]
            if bad or (attempt and any(status)):
                raise _lib.VnfError("vnf_jpeg_huff_encode_frames failed (%d): a coefficient outside the baseline range or "
                                    "a bad info" % (bad[0] if bad else -4))
            if not any(status):
                break
            with torch.cuda.stream(stream):                  # VNF_E_CAPACITY reports the size that fits: once more, for
                self._huff_enqueue(job, max(lengths), stream)  # the batch, from the coefficients still in _coefs
        cap, total = job["capacity"], sum(lengths)
        with torch.cuda.stream(stream):
            self._files_host = self._grown(self._files_host, total, torch.uint8, pinned=True)
            at = 0
            for i, ln in enumerate(lengths):
                self._files_host[at:at + ln].copy_(self._files[i * cap:i * cap + ln], non_blocking=True)
                at += ln
        stream.synchronize()
        self.d2h_bytes += total
        host, out, at = self._files_host.numpy(), [], 0
        for ln in lengths:
            out.append(host[at:at + ln].tobytes())
            at += ln
        return out

    def encode(self, frames_dev, stream=None):
        return self.finish(self.enqueue(frames_dev, stream))


# one BatchEncoder per (device, quality, sampling, entropy) a caller of encode_batch_device has used, kept for the life of the
# process: each holds the device coefficient / plane buffers and the pinned landing area of its largest batch (about
# 9.4 MB + 6.3 MB pinned per 1080p 4:2:0 frame).  A caller that cycles through settings or wants the memory back owns
# a BatchEncoder itself and drops it.
_encoders = {}


def encode_batch_device(frames_dev, quality=92, sampling="4:2:0", stream=None, entropy="host"):
    """frames_dev: (n,H,W,3) u8 cuda tensor -> a list of n JPEG files (bytes), the ones Pillow writes for these pixels
    with save(format="JPEG", quality=quality, subsampling=sampling).  stream: a torch stream, or an object with a
    `.stream` (upload.FrameUploader); default: the current stream.  entropy: "host" (the Huffman pass on host threads)
    or "device" (in HIP; the same files).  Synchronises with the host (one D2H copy, or one per file)."""
    stream = getattr(stream, "stream", stream)
    key = (str(frames_dev.device), int(quality), sampling_code(sampling), entropy_mode(entropy))
    if key not in _encoders:
        _encoders[key] = BatchEncoder(frames_dev.device, quality, sampling, entropy)
    return _encoders[key].encode(frames_dev, stream)


# overlay -------------------------------------------------------------------------------------------------------------

_font = None


def _label_mask(name, fx, fy):
    """The coverage of `name` as ImageDraw.text paints it with the pen at the sub-pixel offset (fx, fy) of a tile's
    origin -> ((th,tw) u8 cut to the ink, its column and row inside the tile), or (None, 0, 0) for no ink.  Pillow
    puts a text at int(anchor) with the signed fraction math.modf leaves as FreeType's start; drawing at (fx, fy)
    makes exactly that call.  Ink left of or above the tile's origin is cut off: with a negative fraction the anchor is
    negative, the origin lies at or outside the frame's edge, and those pixels are outside the frame too."""
    from PIL import Image, ImageDraw
    global _font
    if _font is None:
        _font = ImageDraw.Draw(Image.new("L", (1, 1))).getfont()
    probe = ImageDraw.Draw(Image.new("L", (1, 1)))
    _, _, r, b = probe.textbbox((fx, fy), name, font=_font)
    im = Image.new("L", (max(1, int(math.ceil(r)) + 2), max(1, int(math.ceil(b)) + 2)), 0)
    ImageDraw.Draw(im).text((fx, fy), name, fill=255, font=_font)
    a = np.asarray(im)
    ys, xs = np.nonzero(a)
    if ys.size == 0:
        return None, 0, 0
    y0, x0 = int(ys.min()), int(xs.min())
    return np.ascontiguousarray(a[y0:int(ys.max()) + 1, x0:int(xs.max()) + 1]), x0, y0


def _trunc(v):
    v = float(v)
    if v != v:
        raise ValueError("overlay_ops: a box coordinate is NaN")
    return int(max(-_COORD, min(_COORD, v)))


def overlay_ops(boxes, names, colour=GREEN):
    """The host side of vnf_overlay_draw: what cli_utils.draw_boxes_on_image(frame, boxes[f], names[f]) paints on
    every frame f of a batch, as a table.  boxes: per frame a list of (x1,y1,x2,y2); names: per frame as many strings.
    -> (ops: OP_DTYPE array in draw order, masks: u8 array).  A frame's rectangle comes before its label, a face after
    the faces before it.  Inverted boxes (Pillow raises on them) get no rectangle."""
    if len(boxes) != len(names):
        raise ValueError("overlay_ops: boxes and names must list the same frames")
    rgb = (int(colour[0]) & 255) | (int(colour[1]) & 255) << 8 | (int(colour[2]) & 255) << 16
    ops, masks, at = [], [], 0
    for f, (bx, nm) in enumerate(zip(boxes, names)):
        if len(bx) != len(nm):
            raise ValueError("overlay_ops: frame %d has %d boxes and %d names" % (f, len(bx), len(nm)))
        for box, name in zip(bx, nm):
            x0, y0, x1, y1 = (_trunc(v) for v in box[:4])
            if x1 >= x0 and y1 >= y0:
                ops.append((RECT, f, x0, y0, x1, y1, 0, rgb))
            ax, ay = float(box[2]), float(box[1])
            if not (abs(ax) < _COORD and abs(ay) < _COORD):
                continue                          # nowhere near a frame
            (fx, ix), (fy, iy) = math.modf(ax), math.modf(ay)
            m, ox, oy = _label_mask(str(name), fx, fy)
            if m is None:
                continue
            ops.append((LABEL, f, int(ix) + ox, int(iy) + oy, m.shape[1], m.shape[0], at, rgb))
            masks.append(m.reshape(-1))
            at += m.size
    return (np.array(ops, dtype=OP_DTYPE) if ops else np.zeros((0,), OP_DTYPE),
            np.concatenate(masks) if masks else np.zeros((0,), np.uint8))


def overlay_draw(frames_dev, ops_dev, masks_dev, stream_ptr=None):
    """vnf_overlay_draw on torch tensors: frames_dev (b,H,W,3) u8 cuda, contiguous, painted in place; ops_dev: the
    bytes of an OP_DTYPE table on the device; masks_dev: u8 cuda (may be empty)."""
    if not (frames_dev.is_cuda and ops_dev.is_cuda and masks_dev.is_cuda):
        raise RuntimeError("jpeg_encode.overlay_draw needs cuda tensors (there is no CPU path)")
    if frames_dev.dim() != 4 or frames_dev.shape[3] != 3 or not frames_dev.is_contiguous():
        raise ValueError("overlay_draw: frames_dev must be a contiguous (b,H,W,3) u8 tensor")
    b, h, w = (int(s) for s in frames_dev.shape[:3])
    n_ops = ops_dev.numel() * ops_dev.element_size() // OP_DTYPE.itemsize
    _lib.check(_lib.load().vnf_overlay_draw(
        frames_dev.data_ptr(), b, h, w, ops_dev.data_ptr(), int(n_ops), masks_dev.data_ptr() if masks_dev.numel() else None,
        int(masks_dev.numel()), stream_ptr if stream_ptr is not None else _lib.current_stream_ptr()))
    return frames_dev


def draw_boxes_device(frames_dev, boxes, names, stream=None):
    """draw_boxes_on_image for every frame of a device batch, in place, on `stream` (default: the current one)"""
    import torch
    ops, masks = overlay_ops(boxes, names)
    if ops.shape[0] == 0:
        return frames_dev
    stream = stream if stream is not None else torch.cuda.current_stream(frames_dev.device)
    with torch.cuda.stream(stream):
        packed = np.concatenate([ops.view(np.uint8), masks])            # one upload; the table first keeps it aligned
        dev = torch.from_numpy(packed).to(frames_dev.device, non_blocking=False)
        nb = ops.nbytes
        overlay_draw(frames_dev, dev[:nb], dev[nb:], ctypes.c_void_p(stream.cuda_stream))
        dev.record_stream(stream)
    return frames_dev


# text runs -------------------------------------------------------------------------------------------------------------
# The emotion lines ('<tag> - <percent>%', cli_utils.draw_emotions) differ per face and per frame: rendering each with
# Pillow would put the font renderer on the batch's critical path.  They are composited on the device from an atlas of
# the default font's glyphs instead (vnf_overlay_draw_text); a line the atlas cannot express is rendered by
# `_label_mask` and goes through the LABEL path, so the picture is Pillow's either way.

RUN_DTYPE = np.dtype([("frame", "<i4"), ("x", "<i4"), ("y", "<i4"), ("rgb", "<u4"), ("first", "<i4"), ("length", "<i4")])  # vnf_text_run
GLYPH_DTYPE = np.dtype([("offset", "<i4"), ("w", "<i4"), ("h", "<i4"), ("ox", "<i4"), ("oy", "<i4"), ("advance", "<i4")])  # vnf_text_glyph
TEXT_RUN_MAX = 64                               # VNF_TEXT_RUN_MAX
TEXT_GLYPH_MAX = 64                             # VNF_TEXT_GLYPH_MAX
ATLAS_FIRST, ATLAS_LAST = 32, 126               # printable ASCII
LABEL_PEN = 16                                  # where a fallback line's pen sits inside its rendered tile (pixels)

_atlas = False                                  # False: not built yet; None: this Pillow's default font has no atlas
_atlas_dev = {}


def text_atlas():
    """The default font's glyphs for printable ASCII, built once per process: {'glyphs': GLYPH_DTYPE array,
    'coverage': u8 array, 'bytes': the vnf_text_atlas image of both}, or None when a string's picture is not the sum of
    its glyphs' -- the font is no FreeType face laid out by Layout.BASIC, an advance is not an integer, or a glyph is
    larger than the kernel takes.  Each glyph is what ImageDraw.text paints for the character alone, cut to its ink."""
    global _atlas
    if _atlas is not False:
        return _atlas
    from PIL import Image, ImageDraw, ImageFont
    font = ImageDraw.Draw(Image.new("L", (1, 1))).getfont()
    _atlas = None
    if getattr(font, "layout_engine", None) != ImageFont.Layout.BASIC or not hasattr(font, "getlength"):
        return None
    pad = TEXT_GLYPH_MAX
    glyphs, cov, at = np.zeros((ATLAS_LAST - ATLAS_FIRST + 1,), GLYPH_DTYPE), [], 0
    for c in range(ATLAS_FIRST, ATLAS_LAST + 1):
        adv = float(font.getlength(chr(c)))
        if adv != int(adv) or not 0 <= adv <= TEXT_GLYPH_MAX:
            return None
        im = Image.new("L", (3 * pad, 3 * pad), 0)
        ImageDraw.Draw(im).text((pad, pad), chr(c), fill=255, font=font)
        a = np.asarray(im)
        ys, xs = np.nonzero(a)
        g = glyphs[c - ATLAS_FIRST]
        g["advance"] = int(adv)
        if ys.size == 0:
            continue
        y0, y1, x0, x1 = int(ys.min()), int(ys.max()) + 1, int(xs.min()), int(xs.max()) + 1
        if x0 == 0 or y0 == 0 or x1 == 3 * pad or y1 == 3 * pad or x1 - x0 > TEXT_GLYPH_MAX or y1 - y0 > TEXT_GLYPH_MAX:
            return None                          # ink up to the canvas's edge: the glyph may be larger than it
        g["offset"], g["w"], g["h"], g["ox"], g["oy"] = at, x1 - x0, y1 - y0, x0 - pad, y0 - pad
        cov.append(np.ascontiguousarray(a[y0:y1, x0:x1]).reshape(-1))
        at += cov[-1].size
    coverage = np.concatenate(cov) if cov else np.zeros((0,), np.uint8)
    head = np.array([ATLAS_FIRST, glyphs.shape[0]], "<i4")
    _atlas = {"glyphs": glyphs, "coverage": coverage,
              "bytes": np.concatenate([head.view(np.uint8), glyphs.view(np.uint8), coverage]),
              # what text_runs needs per line, in forms the bytes methods and sum() take
              "charset": bytes(range(ATLAS_FIRST, ATLAS_LAST + 1)),
              "blank": bytes(ATLAS_FIRST + i for i, g in enumerate(glyphs) if not g["w"]),
              "advance": [0] * ATLAS_FIRST + [int(a) for a in glyphs["advance"]] + [0] * (255 - ATLAS_LAST)}
    ink = glyphs[glyphs["w"] > 0]
    # a box every glyph's ink fits when the pen is at 0: columns [left, advance + right), rows [top, bottom)
    _atlas["extent"] = (int(ink["ox"].min()), int((ink["ox"] + ink["w"] - ink["advance"]).max()), int(ink["oy"].min()),
                        int((ink["oy"] + ink["h"]).max())) if ink.size else (0, 0, 0, 0)
    return _atlas


def text_atlas_device(device):
    """the atlas's bytes on `device`, uploaded once per process and device"""
    import torch
    key = str(torch.device(device))
    if key not in _atlas_dev:
        _atlas_dev[key] = torch.from_numpy(text_atlas()["bytes"]).to(device)
    return _atlas_dev[key]


def _run_box(atlas, text, x, y):
    """a rectangle (x0, y0, x1, y1), half open, that holds the ink of the run `text` (bytes inside the atlas) anchored
    at (x, y) -- the pen's travel widened by the font's largest overhangs, the font's rows --, or None for no ink"""
    if not text.strip(atlas["blank"]):
        return None
    left, right, top, bottom = atlas["extent"]
    return x + min(left, 0), y + top, x + sum(map(atlas["advance"].__getitem__, text)) + max(right, 0), y + bottom


def emotion_lines(boxes, tags, probs):
    """cli_utils.draw_emotions's text calls for a batch: boxes per frame; tags / probs per frame and face -> a list of
    (frame, x, y, string) in draw order"""
    out = []
    for f, bx in enumerate(boxes):
        for idx, box in enumerate(bx):
            for i, (tag, p) in enumerate(zip(tags[f][idx], probs[f][idx])):
                # the anchor in draw_emotions's own arithmetic (box[0] + 5 in the box's dtype, then truncated)
                out.append((f, int(box[0] + 5), int(box[1]) + i * 16 + 4, '{} - {:.2f}%'.format(tag, p * 100)))
    return out


def text_runs(lines, colour=GREEN, atlas=False):
    """The host side of vnf_overlay_draw_text: consecutive ImageDraw.text((x, y), s, fill=colour) calls with integer
    anchors, as tables.  lines: (frame, x, y, string) in draw order.
    -> (runs: RUN_DTYPE array, chars: u8 array, launch_ends: int32 array, label_ops: OP_DTYPE array, masks: u8 array).
    The runs are ordered by launch, draw order inside one: a run whose rectangle (`_run_box`, which holds its ink)
    intersects an earlier run's on the same frame sits in a later launch than it (in practice there is one launch).
    A frame with a line the atlas cannot express -- a character outside it, more than TEXT_RUN_MAX characters, or no
    atlas at all -- has ALL its lines as LABEL ops (rendered by `_label_mask`, for vnf_overlay_draw, behind the boxes
    and names), so that the draw order inside a frame never crosses the two paths."""
    atlas = text_atlas() if atlas is False else atlas
    rgb = (int(colour[0]) & 255) | (int(colour[1]) & 255) << 8 | (int(colour[2]) & 255) << 16
    coded, by_label = [], set()
    for f, x, y, s in lines:
        b = s.encode("ascii", "replace") if s.isascii() else None
        ok = atlas is not None and b is not None and len(b) <= TEXT_RUN_MAX and not b.translate(None, atlas["charset"])
        if not ok:
            by_label.add(int(f))
        coded.append(b if ok else None)
    runs, chars, levels, placed = [], bytearray(), [], {}
    ops, masks, mat = [], [], 0
    for (f, x, y, s), text in zip(lines, coded):
        f, x, y = int(f), int(max(-_COORD, min(_COORD, x))), int(max(-_COORD, min(_COORD, y)))
        if f in by_label:
            # the pen sits LABEL_PEN pixels inside the tile: `_label_mask` cuts ink left of or above the tile's origin,
            # and glyphs such as 's' or ')' start a pixel left of the pen
            m, ox, oy = _label_mask(s, float(LABEL_PEN), float(LABEL_PEN))
            if m is not None:
                ops.append((LABEL, f, x + ox - LABEL_PEN, y + oy - LABEL_PEN, m.shape[1], m.shape[0], mat, rgb))
                masks.append(m.reshape(-1))
                mat += m.size
            continue
        box = _run_box(atlas, text, x, y)
        if box is None:
            continue
        level = 0
        for (x0, y0, x1, y1), lv in placed.get(f, ()):
            if lv >= level and box[0] < x1 and x0 < box[2] and box[1] < y1 and y0 < box[3]:
                level = lv + 1
        placed.setdefault(f, []).append((box, level))
        runs.append((f, x, y, rgb, len(chars), len(text)))
        levels.append(level)
        chars += text
    runs = np.array(runs, dtype=RUN_DTYPE) if runs else np.zeros((0,), RUN_DTYPE)
    levels = np.asarray(levels, np.int64)
    order = np.argsort(levels, kind="stable")
    ends = np.cumsum(np.bincount(levels)).astype(np.int32) if levels.size else np.zeros((0,), np.int32)
    return (runs[order], np.frombuffer(bytes(chars), np.uint8), ends,
            np.array(ops, dtype=OP_DTYPE) if ops else np.zeros((0,), OP_DTYPE),
            np.concatenate(masks) if masks else np.zeros((0,), np.uint8))


def overlay_draw_text(frames_dev, runs_dev, chars_dev, launch_ends=None, atlas_dev=None, stream_ptr=None):
    """vnf_overlay_draw_text on torch tensors: frames_dev (b,H,W,3) u8 cuda, contiguous, painted in place; runs_dev:
    the bytes of a RUN_DTYPE table on the device; chars_dev: u8 cuda; launch_ends: host int32 array (None: one launch);
    atlas_dev: default text_atlas_device(frames_dev.device)."""
    if not (frames_dev.is_cuda and runs_dev.is_cuda and chars_dev.is_cuda):
        raise RuntimeError("jpeg_encode.overlay_draw_text needs cuda tensors (there is no CPU path)")
    if frames_dev.dim() != 4 or frames_dev.shape[3] != 3 or not frames_dev.is_contiguous():
        raise ValueError("overlay_draw_text: frames_dev must be a contiguous (b,H,W,3) u8 tensor")
    if atlas_dev is None:
        if text_atlas() is None:
            raise RuntimeError("overlay_draw_text: this Pillow's default font has no glyph atlas (text_runs sends every "
                               "line through the LABEL path then)")
        atlas_dev = text_atlas_device(frames_dev.device)
    b, h, w = (int(s) for s in frames_dev.shape[:3])
    n_runs = runs_dev.numel() * runs_dev.element_size() // RUN_DTYPE.itemsize
    ends = None if launch_ends is None else np.ascontiguousarray(launch_ends, dtype=np.int32)
    _lib.check(_lib.load().vnf_overlay_draw_text(
        frames_dev.data_ptr(), b, h, w, runs_dev.data_ptr(), int(n_runs), ends.ctypes.data if ends is not None else None,
        int(ends.size) if ends is not None else 0, chars_dev.data_ptr() if chars_dev.numel() else None, int(chars_dev.numel()),
        atlas_dev.data_ptr(), int(atlas_dev.numel()), stream_ptr if stream_ptr is not None else _lib.current_stream_ptr()))
    return frames_dev


def _upload_and_draw(frames_dev, ops, masks, runs, chars, ends, stream):
    """one upload of every table, then vnf_overlay_draw (boxes, names, LABEL lines) and vnf_overlay_draw_text"""
    import torch
    if ops.shape[0] == 0 and runs.shape[0] == 0:
        return frames_dev
    stream = stream if stream is not None else torch.cuda.current_stream(frames_dev.device)
    with torch.cuda.stream(stream):
        # the tables first keeps them 4-byte aligned (both records are multiples of 4 bytes)
        packed = np.concatenate([ops.view(np.uint8), runs.view(np.uint8), masks, chars])
        dev = torch.from_numpy(packed).to(frames_dev.device, non_blocking=False)
        a, b = ops.nbytes, ops.nbytes + runs.nbytes
        sp = ctypes.c_void_p(stream.cuda_stream)
        if ops.shape[0]:
            overlay_draw(frames_dev, dev[:a], dev[b:b + masks.size], sp)
        if runs.shape[0]:
            overlay_draw_text(frames_dev, dev[a:b], dev[b + masks.size:], ends, None, sp)
        dev.record_stream(stream)
    return frames_dev


def draw_emotions_device(frames_dev, boxes, tags, probs, stream=None):
    """cli_utils.draw_emotions for every frame of a device batch, in place, on `stream` (default: the current one)"""
    runs, chars, ends, ops, masks = text_runs(emotion_lines(boxes, tags, probs))
    return _upload_and_draw(frames_dev, ops, masks, runs, chars, ends, stream)


def draw_annotations_device(frames_dev, boxes, names, tags=None, probs=None, stream=None):
    """draw_boxes_on_image, then (with tags) draw_emotions, for every frame of a device batch, in place: the
    rectangles, the names and the lines that need the LABEL path in one vnf_overlay_draw launch, the text runs behind
    it."""
    ops, masks = overlay_ops(boxes, names)
    runs, chars, ends = np.zeros((0,), RUN_DTYPE), np.zeros((0,), np.uint8), None
    if tags is not None:
        runs, chars, ends, ops2, masks2 = text_runs(emotion_lines(boxes, tags, probs))
        if ops2.shape[0]:
            ops2 = ops2.copy()
            ops2["mask_offset"] += masks.size
            ops, masks = np.concatenate([ops, ops2]), np.concatenate([masks, masks2])
    return _upload_and_draw(frames_dev, ops, masks, runs, chars, ends, stream)


# the video writer video.run_stream drives --------------------------------------------------------------------------

PART_MAGIC = b"VNFMJPG1"


class VideoEncoder:
    """`encoder` of video.run_stream: draws on a round's own device frames, encodes them and appends them, in frame
    order, to a Motion-JPEG AVI (one process) or to this rank's spool file `<path>.rank<r>.part` (several; rank 0
    merges them with `merge` once every rank has closed its own)."""

    def __init__(self, path, fps, device, quality=92, sampling="4:2:0", rank=0, world=1, idx2tag=None, entropy="host"):
        """entropy: where the Huffman pass runs, "host" or "device" (BatchEncoder).  idx2tag: the emotion tag table (index -> tag) for write_batch(emotions=...) called with class indices, as
        video.run_stream(emotions=k) calls it; None: the tags are drawn as they are handed over."""
        import torch
        from .mjpeg_avi import MjpegAviWriter
        from .streams import side_stream
        entropy_mode(entropy)
        if not str(path).lower().endswith(".avi"):
            raise ValueError("the device encoder writes a Motion-JPEG AVI: give the video a name ending in .avi, got %r" % (path,))
        self.path, self.fps, self.rank, self.world = str(path), float(fps), int(rank), int(world)
        self.device = torch.device(device)
        self.enc = BatchEncoder(self.device, quality, sampling, entropy)
        self.stream = side_stream(self.device, ENCODE_STREAM_ROLE)
        self.frames = 0
        self.idx2tag = idx2tag
        if self.world == 1:
            self._avi, self._part = MjpegAviWriter(self.path, self.fps), None
        else:
            self._avi, self._part = None, open(self.part_path(self.path, self.rank), "wb")
            self._part.write(PART_MAGIC)

    @staticmethod
    def part_path(path, rank):
        return "%s.rank%d.part" % (path, rank)

    def write_batch(self, frames_dev, numbers, boxes, names, after=None, emotions=None):
        """frames_dev: the batch in HBM, drawn on IN PLACE: the caller hands it over for good -- a buffer nobody reads
        again, never a caller's own source frames (run_stream passes its upload-ring slot, or a copy) -- and its other
        readers are done once `after`, an event, has passed.  numbers: the frames' numbers (ascending); boxes / names: per frame.
        emotions: None, or per frame (tags, probs), each with one row of top-k entries per face: drawn behind the
        boxes and names as cli_utils.draw_emotions draws them (a tag that is an integer goes through `idx2tag`).
        -> the event behind the last kernel that reads frames_dev."""
        if after is not None:
            self.stream.wait_event(after)
        if any(len(n) for n in names):
            tags = probs = None
            if emotions is not None:
                probs = [e[1] for e in emotions]
                tags = [[[self._tag(t) for t in face] for face in e[0]] for e in emotions]
            draw_annotations_device(frames_dev, boxes, names, tags, probs, self.stream)
        job = self.enc.enqueue(frames_dev, self.stream)
        h, w = int(frames_dev.shape[1]), int(frames_dev.shape[2])
        for num, data in zip(numbers, self.enc.finish(job)):
            if self._avi is not None:
                self._avi.append(data, (w, h))
            else:
                self._part.write(struct.pack("<IIII", int(num), len(data), w, h))
                self._part.write(data)
            self.frames += 1
        return job["kernels"]

    def _tag(self, t):
        if self.idx2tag is not None and isinstance(t, (int, np.integer)):
            return self.idx2tag[int(t)]
        return t

    def close(self):
        """finish this process's file.  One process: the AVI (a stream without frames is an error: there is no video to
        write); several: this rank's spool file, which may be empty."""
        if self._avi is not None:
            avi, self._avi = self._avi, None
            if not len(avi):
                raise ValueError("no frame reached the video encoder: %r is not written" % (self.path,))
            avi.close()
        if self._part is not None:
            self._part.close()
            self._part = None

    def abort(self):
        """give up after an error: close and remove what this process wrote (a half-written AVI, its spool file)"""
        if self._avi is not None:
            self._avi.abort()
            self._avi = None
        if self._part is not None:
            self._part.close()
            self._part = None
        part = self.part_path(self.path, self.rank)
        if self.world > 1 and os.path.exists(part):
            os.remove(part)

    def merge(self, remove=True):
        """rank 0, after every rank's close(): the spool files -> the AVI, frames in number order"""
        from .mjpeg_avi import merge_mjpeg_parts
        parts = [self.part_path(self.path, r) for r in range(self.world)]
        n = merge_mjpeg_parts(parts, self.path, self.fps)
        if remove:
            for p in parts:
                os.remove(p)
        return n
