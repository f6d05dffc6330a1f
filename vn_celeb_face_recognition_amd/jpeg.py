"""JPEG video frames decoded on the device (include/vnface.h, "JPEG video frames").

The reference pulls decoded frames out of cv2.VideoCapture.read (/root/reference/demo_video.py:78-110); this package
read Motion-JPEG AVIs and directories of .jpg frames with Pillow, one frame at a time on one host thread.  Here a batch
of compressed frames is split in two:

  * the bitstream walk (markers, Huffman decode) stays on the host, in C++ (csrc/jpeg_entropy.cpp), one frame per call,
    threaded across the frames of the batch (ctypes releases the GIL) straight into a pinned int16 staging slot of the
    batch's `upload.FrameUploader`;
  * dequantisation, IDCT, chroma upsampling and YCbCr -> RGB run on the MI355X (csrc/jpeg_decode.hip) on the upload
    stream, behind the one host -> HBM copy of the coefficients.  The RGB batch is born in the uploader's device ring.

The bytes are libjpeg's (and so Pillow's) exactly.  Anything the native decoder does not take -- progressive, CMYK,
12-bit, frames without Huffman tables, a batch of mixed geometry, a corrupt stream -- is reported as `None` and the
caller decodes that batch with Pillow as before (`decode_host`), which then raises whatever it raised before.
"""
import ctypes
import io
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from . import _lib

NOT_TAKEN = 1                                   # VNF_JPEG_NOT_TAKEN
GRAY, S444, S422, S420 = 0, 1, 2, 3             # VNF_JPEG_* sampling codes
ENTROPY_THREADS = 8                             # fixed: the frames of a batch, never sized from the machine's CPU count

_pool = None


def _entropy_pool():
    global _pool
    if _pool is None:
        _pool = ThreadPoolExecutor(max_workers=ENTROPY_THREADS, thread_name_prefix="vnf-jpeg")
    return _pool


def probe(data):
    """-> (status, JpegInfo): 0 taken, NOT_TAKEN a JPEG left to the host decoder, negative: not a decodable JPEG."""
    info = _lib.JpegInfo()
    rc = _lib.load().vnf_jpeg_probe(data, len(data), ctypes.byref(info))
    return rc, info


def entropy_decode(data, info, coefs):
    """Huffman-decode `data` (bytes) into `coefs`, a writable C-contiguous int16 array of at least info.coef_count
    elements.  -> status (0: done)."""
    if coefs.dtype != np.int16 or not coefs.flags.c_contiguous or not coefs.flags.writeable:
        raise ValueError("entropy_decode: coefs must be a writable contiguous int16 array")
    return _lib.load().vnf_jpeg_entropy_decode(data, len(data), ctypes.byref(info), coefs.ctypes.data, coefs.size)


def quant_table(info):
    """(3,64) u8: the component tables of a probed frame, natural order"""
    return np.ctypeslib.as_array(info.quant).reshape(3, 64).copy()


def decode_host(data):
    """The host decoder (Pillow), as mjpeg_avi.MjpegFrames and cli_utils.read_rgb use it: (H,W,3) u8 RGB."""
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


class CompressedBatch(list):
    """The frames of one batch as compressed JPEG bytes (video.FrameSource.rank_batches(compressed=True))."""


class HostFrame:
    """A frame of a device-decoded batch on the host side: its shape is known, its pixels are decoded (by the host
    decoder: the same bytes) only when somebody asks for them (run_stream's on_frame)."""

    def __init__(self, data, shape):
        self.data, self.shape = data, tuple(shape)

    def __array__(self, dtype=None, copy=None):
        a = decode_host(self.data)
        return a if dtype is None else a.astype(dtype)


def decode_frames(coefs_dev, quant_dev, n, width, height, sampling, out, workspace, stream_ptr=None):
    """vnf_jpeg_decode_frames on torch tensors; enqueues on `stream_ptr` (default: the current stream)."""
    if not (coefs_dev.is_cuda and quant_dev.is_cuda and out.is_cuda and workspace.is_cuda):
        raise RuntimeError("jpeg.decode_frames needs cuda tensors (there is no CPU path)")
    _lib.check(_lib.load().vnf_jpeg_decode_frames(
        coefs_dev.data_ptr(), quant_dev.data_ptr(), int(n), int(width), int(height), int(sampling), out.data_ptr(),
        workspace.data_ptr(), workspace.numel() * workspace.element_size(),
        stream_ptr if stream_ptr is not None else _lib.current_stream_ptr()))
    return out


def decode_batch_device(frames, device, uploader, timing=None):
    """frames: list of JPEG byte strings.  -> ((B,H,W,3) u8 cuda tensor, ready event, device slot for
    uploader.release()), or None when the batch is not taken (a frame that does not probe or entropy-decode, mixed
    geometry): the caller then decodes it on the host.  Nothing of a refused batch reaches the device.
    timing: optional dict that receives 'entropy_s' (host wall time of the threaded entropy pass)."""
    import torch
    if not frames:
        return None
    infos = []
    for d in frames:
        rc, info = probe(d)
        if rc != 0:
            return None
        infos.append(info)
    i0 = infos[0]
    geom = (i0.width, i0.height, i0.sampling)
    if any((i.width, i.height, i.sampling) != geom or i.coef_count != i0.coef_count for i in infos):
        return None
    B, cc = len(frames), int(i0.coef_count)
    lib = _lib.load()
    ws = int(lib.vnf_jpeg_workspace_bytes(B, i0.width, i0.height, i0.sampling))
    if ws < 0:
        return None
    coef_bytes, quant_bytes = B * cc * 2, B * 192
    staged, k = uploader.slot((coef_bytes + quant_bytes,))
    host = staged.numpy()
    coefs = host[:coef_bytes].view(np.int16).reshape(B, cc)
    quant = host[coef_bytes:].reshape(B, 3, 64)

    def one(i):
        quant[i] = quant_table(infos[i])
        return entropy_decode(frames[i], infos[i], coefs[i])

    if timing is not None:
        import time
        t0 = time.perf_counter()
    rcs = list(_entropy_pool().map(one, range(B))) if B > 1 else [one(0)]
    if timing is not None:
        timing["entropy_s"] = time.perf_counter() - t0
    if any(rc != 0 for rc in rcs):
        return None
    shape = (B, int(i0.height), int(i0.width), 3)
    out, slot = uploader.take_device_slot(shape)
    scratch = uploader.scratch(coef_bytes + quant_bytes + ws)
    with torch.cuda.stream(uploader.stream):
        scratch[:coef_bytes + quant_bytes].copy_(staged, non_blocking=True)
        copied = uploader.stream.record_event()
        if timing is not None and timing.get("events"):
            e0 = torch.cuda.Event(enable_timing=True)
            e0.record(uploader.stream)
        decode_frames(scratch[:coef_bytes], scratch[coef_bytes:coef_bytes + quant_bytes], B, i0.width, i0.height,
                      i0.sampling, out, scratch[coef_bytes + quant_bytes:],
                      ctypes.c_void_p(uploader.stream.cuda_stream))
        if timing is not None and timing.get("events"):
            e1 = torch.cuda.Event(enable_timing=True)
            e1.record(uploader.stream)
            timing["kernel_events"] = (e0, e1)
        ev = uploader.stream.record_event()
    uploader.staged(k, copied, coef_bytes + quant_bytes)
    return out, ev, slot


def decode_batch(frames, device, uploader):
    """Device decode with the host fallback: -> (frames_dev, ready event, device slot, host_frames) where host_frames
    are `HostFrame`s (device path) or the decoded arrays (host path, uploaded as before)."""
    r = decode_batch_device(frames, device, uploader)
    if r is not None:
        shape = tuple(r[0].shape[1:])
        return r + ([HostFrame(d, shape) for d in frames],)
    host = [decode_host(d) for d in frames]
    dev, ev = uploader.upload(host)
    return dev, ev, uploader.last_slot, host
