"""JPEG video frames decoded on the device (include/vnface.h, "JPEG video frames").

The reference pulls decoded frames out of cv2.VideoCapture.read (/root/reference/demo_video.py:78-110); this package
read Motion-JPEG AVIs and directories of .jpg frames with Pillow, one frame at a time on one host thread.  Here a batch
of compressed frames is split in two:

  * the bitstream walk (markers, Huffman decode) stays on the host, in C++ (csrc/jpeg_entropy.cpp), one frame per call,
    threaded across the frames of the batch (ctypes releases the GIL) straight into a pinned int16 staging slot of the
    batch's `upload.FrameUploader`;
  * dequantisation, IDCT, chroma upsampling and YCbCr -> RGB run on the MI355X (csrc/jpeg_decode.hip) on the upload
    stream, behind the one host -> HBM copy of the coefficients.  The RGB batch is born in the uploader's device ring.

With entropy="device" (default "host") the Huffman decode moves to the device as well (csrc/jpeg_huff_decode.hip): the
host only PREPARES a frame (vnf_jpeg_huff_prepare: the scan unstuffed and cut at its restart markers, the decode tables
laid out, no symbol decoded) into the pinned slot, the compressed frames cross the bus as they are, and the
coefficients live only in the uploader's device scratch.  A batch the device decoder refuses is decoded again by the
host path.

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
ENTROPY = ("host", "device")                    # where the Huffman decode of decode_batch_device runs
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


def huff_prepare(data, info, out):
    """vnf_jpeg_huff_prepare: `data` (bytes) of a probed frame -> the blob the device Huffman decoder reads, into `out`
    (a writable C-contiguous uint8 array; huff_prepared_bound(len(data), info) bytes always suffice).
    -> (status, blob length)"""
    if out.dtype != np.uint8 or not out.flags.c_contiguous or not out.flags.writeable:
        raise ValueError("huff_prepare: out must be a writable contiguous uint8 array")
    n = ctypes.c_int64(0)
    rc = _lib.load().vnf_jpeg_huff_prepare(data, len(data), ctypes.byref(info), out.ctypes.data, out.size, ctypes.byref(n))
    return rc, int(n.value)


def huff_prepared_bound(nbytes, info):
    n = int(_lib.load().vnf_jpeg_huff_prepared_bound(int(nbytes), ctypes.byref(info)))
    return n if n >= 0 else _lib.check(n)


def huff_decode_workspace_bytes(n, info, max_blob_bytes, subseq_bits=0):
    n = int(_lib.load().vnf_jpeg_huff_decode_workspace_bytes(int(n), ctypes.byref(info), int(max_blob_bytes), int(subseq_bits)))
    return n if n >= 0 else _lib.check(n)


def huff_decode_frames(blobs_dev, offsets, sizes, info, coefs_dev, status_dev, workspace, subseq_bits=0, stream_ptr=None):
    """vnf_jpeg_huff_decode_frames on torch tensors: len(offsets) prepared frames inside the u8 tensor blobs_dev ->
    coefs_dev (int16) and status_dev (int32); enqueues on `stream_ptr` (default: the current stream)."""
    if not (blobs_dev.is_cuda and coefs_dev.is_cuda and status_dev.is_cuda and workspace.is_cuda):
        raise RuntimeError("jpeg.huff_decode_frames needs cuda tensors (there is no CPU path)")
    n = len(offsets)
    arr = ctypes.c_int64 * max(n, 1)
    _lib.check(_lib.load().vnf_jpeg_huff_decode_frames(
        blobs_dev.data_ptr(), arr(*[int(o) for o in offsets]), arr(*[int(b) for b in sizes]), n, ctypes.byref(info),
        int(subseq_bits), coefs_dev.data_ptr(), status_dev.data_ptr(), workspace.data_ptr(),
        workspace.numel() * workspace.element_size(), stream_ptr if stream_ptr is not None else _lib.current_stream_ptr()))


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


def decode_batch_device(frames, device, uploader, timing=None, *, entropy="host", subseq_bits=0):
    """frames: list of JPEG byte strings.  -> ((B,H,W,3) u8 cuda tensor, ready event, device slot for
    uploader.release()), or None when the batch is not taken (a frame that does not probe or entropy-decode, mixed
    geometry): the caller then decodes it on the host.  Nothing of a refused batch reaches the device.
    entropy: "host" -- the Huffman decode on host threads, the coefficients cross the bus; "device" -- the frames are
    prepared on those threads, cross as they are and are Huffman-decoded in HIP (subseq_bits: its tuning parameter, 0 for
    the default).  A batch the device decoder refuses (any frame's status) releases its device slot and goes through the
    "host" path, so the result is the same either way.
    timing: optional dict that receives 'entropy_s' (host wall time of the threaded entropy or prepare pass),
    'upload_bytes', and with timing['events'] the HIP events 'kernel_events' (around the IDCT / colour kernels) and, for
    "device", 'huff_events' (around the Huffman kernels)."""
    if entropy not in ENTROPY:
        raise ValueError("decode_batch_device: entropy must be one of %s, got %r" % (ENTROPY, entropy))
    if entropy == "device":
        import torch
        if torch.device(device).type != "cuda" or uploader is None:
            raise RuntimeError("jpeg.decode_batch_device(entropy='device') needs cuda tensors (there is no CPU path)")
        r = _decode_batch_huff_device(frames, uploader, timing, subseq_bits)
        if r is not None:
            return r
    import torch
    if not frames:
        return None
    infos = _probe_batch(frames)
    if infos is None:
        return None
    i0 = infos[0]
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
    if timing is not None:
        timing["upload_bytes"] = coef_bytes + quant_bytes
    return out, ev, slot


def _probe_batch(frames):
    """-> the frames' infos when every one probes and they share one geometry, else None"""
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
    return infos


def _round16(v):
    return (int(v) + 15) & ~15


def _decode_batch_huff_device(frames, uploader, timing, subseq_bits):
    """decode_batch_device's entropy="device": probe, prepare into the pinned slot (blobs, then the quantisation
    tables), one copy, vnf_jpeg_huff_decode_frames, vnf_jpeg_decode_frames, all on the upload stream.  The statuses come
    back through a small pinned copy behind the Huffman kernels; only that event is waited for.  -> (frames, event,
    slot), or None: not taken, or a frame the device decoder refused (its device slot is released)."""
    import torch
    if not frames:
        return None
    infos = _probe_batch(frames)
    if infos is None:
        return None
    i0, B = infos[0], len(frames)
    cc = int(i0.coef_count)
    lib = _lib.load()
    ws_pix = int(lib.vnf_jpeg_workspace_bytes(B, i0.width, i0.height, i0.sampling))
    if ws_pix < 0:
        return None
    bounds = [huff_prepared_bound(len(d), inf) for d, inf in zip(frames, infos)]
    offs = [0] * B
    for i in range(1, B):
        offs[i] = offs[i - 1] + _round16(bounds[i - 1])
    quant_at = offs[-1] + _round16(bounds[-1])
    up_bytes = quant_at + B * 192
    ws_huff = int(lib.vnf_jpeg_huff_decode_workspace_bytes(B, ctypes.byref(i0), max(bounds), int(subseq_bits)))
    if ws_huff < 0:
        if int(subseq_bits) and (int(subseq_bits) % 32 or not 32 <= int(subseq_bits) <= 8192):
            raise ValueError("decode_batch_device: subseq_bits must be 0 or a multiple of 32 in 32..8192, got %r" % (subseq_bits,))
        return None
    staged, k = uploader.slot((up_bytes,))
    host = staged.numpy()
    quant = host[quant_at:].reshape(B, 3, 64)

    def one(i):
        quant[i] = quant_table(infos[i])
        return huff_prepare(frames[i], infos[i], host[offs[i]:offs[i] + bounds[i]])

    if timing is not None:
        import time
        t0 = time.perf_counter()
    res = list(_entropy_pool().map(one, range(B))) if B > 1 else [one(0)]
    if timing is not None:
        timing["entropy_s"] = time.perf_counter() - t0
    if any(rc != 0 for rc, _ in res):
        return None
    sizes = [n for _, n in res]
    shape = (B, int(i0.height), int(i0.width), 3)
    out, slot = uploader.take_device_slot(shape)
    coef_at = _round16(up_bytes)
    status_at = coef_at + _round16(B * cc * 2)
    huff_at = status_at + _round16(4 * B)
    pix_at = huff_at + _round16(ws_huff)
    scratch = uploader.scratch(pix_at + ws_pix)
    status_dev = scratch[status_at:status_at + 4 * B].view(torch.int32)
    status_host = uploader.status_buffer(B)
    events = timing is not None and timing.get("events")
    stream_ptr = ctypes.c_void_p(uploader.stream.cuda_stream)
    with torch.cuda.stream(uploader.stream):
        scratch[:up_bytes].copy_(staged, non_blocking=True)
        copied = uploader.stream.record_event()
        if events:
            h0 = torch.cuda.Event(enable_timing=True)
            h0.record(uploader.stream)
        coefs_dev = scratch[coef_at:coef_at + B * cc * 2].view(torch.int16)
        huff_decode_frames(scratch[:quant_at], offs, sizes, i0, coefs_dev, status_dev, scratch[huff_at:huff_at + ws_huff],
                           subseq_bits, stream_ptr)
        if events:
            h1 = torch.cuda.Event(enable_timing=True)
            h1.record(uploader.stream)
            timing["huff_events"] = (h0, h1)
        status_host.copy_(status_dev, non_blocking=True)
        decided = uploader.stream.record_event()
        decode_frames(coefs_dev, scratch[quant_at:up_bytes], B, i0.width, i0.height, i0.sampling, out,
                      scratch[pix_at:pix_at + ws_pix], stream_ptr)
        if events:
            e1 = torch.cuda.Event(enable_timing=True)
            e1.record(uploader.stream)
            timing["kernel_events"] = (h1, e1)
        ev = uploader.stream.record_event()
    uploader.staged(k, copied, up_bytes)
    if timing is not None:
        timing["upload_bytes"] = up_bytes
    decided.synchronize()
    if bool((status_host != 0).any()):
        uploader.release(slot, ev)
        return None
    return out, ev, slot


def decode_batch(frames, device, uploader, *, entropy="host"):
    """Device decode with the host fallback: -> (frames_dev, ready event, device slot, host_frames) where host_frames
    are `HostFrame`s (device path) or the decoded arrays (host path, uploaded as before).  entropy: where the Huffman
    decode runs, as in decode_batch_device."""
    if entropy not in ENTROPY:
        raise ValueError("decode_batch: entropy must be one of %s, got %r" % (ENTROPY, entropy))
    r = decode_batch_device(frames, device, uploader) if entropy == "host" else \
        decode_batch_device(frames, device, uploader, entropy=entropy)
    if r is not None:
        shape = tuple(r[0].shape[1:])
        return r + ([HostFrame(d, shape) for d in frames],)
    host = [decode_host(d) for d in frames]
    dev, ev = uploader.upload(host)
    return dev, ev, uploader.last_slot, host
