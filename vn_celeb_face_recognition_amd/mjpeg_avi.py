"""Motion-JPEG AVI reader / writer in pure Python (PIL for the JPEG frames): the video container the CLIs can read and
write when OpenCV is not installed.

The reference decodes its input with cv2.VideoCapture (/root/reference/demo_video.py:78-110) and exports the annotated
frames with cv2.VideoWriter as MP4V (demo_video.py:25-43).  Neither codec can be produced without OpenCV / FFmpeg; an
AVI whose video stream is MJPG (every frame an independent baseline JPEG) needs nothing but a RIFF walker, and plays in
any player.  Layout written: RIFF 'AVI ' { LIST hdrl { avih, LIST strl { strh(vids/MJPG), strf(BITMAPINFOHEADER) } },
LIST movi { 00dc ... }, idx1 }.
"""
import io
import os
import struct

import numpy as np


def _chunk(fourcc, payload):
    pad = b"\x00" if len(payload) & 1 else b""
    return fourcc + struct.pack("<I", len(payload)) + payload + pad


def _list(kind, payload):
    return b"LIST" + struct.pack("<I", len(payload) + 4) + kind + payload


def _hdrl(w, h, n, biggest, fps):
    scale = 1000
    rate = int(round(float(fps) * scale))
    avih = struct.pack("<14I", int(round(1e6 / float(fps))), int(biggest * float(fps)), 0, 0x10, n, 0, 1, biggest, w, h, 0, 0, 0, 0)
    strh = b"vids" + b"MJPG" + struct.pack("<IHHIIIIIIII4h", 0, 0, 0, 0, scale, rate, 0, n, biggest, 0xFFFFFFFF, 0, 0, 0, w, h)
    strf = struct.pack("<IiiHH4sIiiII", 40, w, h, 1, 24, b"MJPG", w * h * 3, 0, 0, 0, 0)
    return _list(b"hdrl", _chunk(b"avih", avih) + _list(b"strl", _chunk(b"strh", strh) + _chunk(b"strf", strf)))


class MjpegAviWriter:
    """Streaming writer of the layout above: `append` puts a frame's JPEG file into the movi list as it arrives, `close`
    writes the index and patches the sizes, frame count and largest chunk into the header (whose length does not depend
    on them).  Nothing but the index entries (16 bytes a frame) is kept in memory.  The file appears with the first
    frame; closing a writer that never got one raises, as an AVI without frames is none."""

    def __init__(self, path, fps):
        self.path, self.fps = path, float(fps)
        self._f = self._size = None
        self._index, self._off, self._biggest = [], 4, 0          # offsets count from the 'movi' fourcc

    def __len__(self):
        return len(self._index)

    @property
    def size(self):
        """(width, height) of the frames, None before the first one"""
        return self._size

    def _head(self, movi_bytes, idx_bytes):
        w, h = self._size
        hdrl = _hdrl(w, h, len(self._index), self._biggest, self.fps)
        riff = 4 + len(hdrl) + 12 + movi_bytes + idx_bytes
        return b"RIFF" + struct.pack("<I", riff) + b"AVI " + hdrl + b"LIST" + struct.pack("<I", movi_bytes + 4) + b"movi"

    def append(self, jpeg_bytes, size):
        """jpeg_bytes: one frame as a baseline JPEG file; size: its (width, height)"""
        size = (int(size[0]), int(size[1]))
        if self._size is None:
            self._size = size
            self._f = open(self.path, "wb")
            self._f.write(self._head(0, 0))                     # placeholder of the final length
        elif size != self._size:
            raise ValueError("MjpegAviWriter: frames must have equal size")
        c = _chunk(b"00dc", jpeg_bytes)
        self._index.append(b"00dc" + struct.pack("<III", 0x10, self._off, len(jpeg_bytes)))
        self._off += len(c)
        self._biggest = max(self._biggest, len(jpeg_bytes))
        self._f.write(c)

    def close(self):
        """-> the number of frames written"""
        if self._f is None:
            raise ValueError("MjpegAviWriter: no frames")
        idx = _chunk(b"idx1", b"".join(self._index))
        self._f.write(idx)
        self._f.seek(0)
        self._f.write(self._head(self._off - 4, len(idx)))
        self._f.close()
        self._f = None
        return len(self._index)

    def abort(self):
        """give up: close and remove whatever was written (an AVI without its index and sizes is no video)"""
        if self._f is not None:
            self._f.close()
            self._f = None
            os.remove(self.path)


def write_mjpeg_avi(path, frames, fps, quality=92):
    """frames: iterable of (H,W,3) uint8 RGB arrays of equal size.  Returns the number of frames written."""
    from PIL import Image
    wr = MjpegAviWriter(path, fps)
    try:
        for fr in frames:
            a = np.asarray(fr, dtype=np.uint8)
            if len(wr) and (a.shape[1], a.shape[0]) != wr.size:
                raise ValueError("write_mjpeg_avi: frames must have equal size")
            buf = io.BytesIO()
            Image.fromarray(a).save(buf, format="JPEG", quality=quality)
            wr.append(buf.getvalue(), (a.shape[1], a.shape[0]))
        if not len(wr):
            raise ValueError("write_mjpeg_avi: no frames")
    except BaseException:
        wr.abort()                                  # no half-written file is left behind
        raise
    return wr.close()


def read_mjpeg_part(path):
    """A rank's spool file (jpeg_encode.VideoEncoder): yields (frame number, (width, height), JPEG bytes) record by
    record, one frame in memory at a time"""
    with open(path, "rb") as f:
        if f.read(8) != b"VNFMJPG1":
            raise ValueError("%s: not a Motion-JPEG spool file" % path)
        while True:
            head = f.read(16)
            if not head:
                return
            if len(head) != 16:
                raise ValueError("%s: truncated spool file" % path)
            num, n, w, h = struct.unpack("<IIII", head)
            data = f.read(n)
            if len(data) != n:
                raise ValueError("%s: truncated spool file" % path)
            yield num, (w, h), data


def merge_mjpeg_parts(parts, out, fps):
    """The ranks' spool files -> one AVI at `out` with the frames in frame-number order (every part ascending, a frame
    number only once).  The parts are read lazily: one frame of every rank is in memory at a time.  On an error nothing is left at
    `out`.  Returns the number of frames."""
    import heapq
    wr = MjpegAviWriter(out, fps)
    last = None
    try:
        for num, size, data in heapq.merge(*[read_mjpeg_part(p) for p in parts], key=lambda r: r[0]):
            if last is not None and num <= last:      # a part out of order shows here too: the merge is then not sorted
                raise ValueError("merge_mjpeg_parts: frame %d appears twice or out of order" % num)
            last = num
            wr.append(data, size)
        if not len(wr):
            raise ValueError("merge_mjpeg_parts: no frames")
    except BaseException:
        wr.abort()
        raise
    return wr.close()


def _walk(buf, start, end):
    """Yield (fourcc, payload_start, payload_size) of the chunks in buf[start:end]."""
    p = start
    while p + 8 <= end:
        cc = bytes(buf[p:p + 4])
        (sz,) = struct.unpack_from("<I", buf, p + 4)
        yield cc, p + 8, sz
        p += 8 + sz + (sz & 1)


def read_mjpeg_avi(path):
    """-> (fps, random-access sequence of (H,W,3) uint8 RGB frames, frame count).  Raises ValueError for anything that
    is not an AVI with an MJPG video stream."""
    data = np.memmap(path, dtype=np.uint8, mode="r")
    if len(data) < 12 or bytes(data[0:4]) != b"RIFF" or bytes(data[8:12]) != b"AVI ":
        raise ValueError("%s: not a RIFF AVI file" % path)
    fps = None
    handler = None
    spans = []
    for cc, ps, sz in _walk(data, 12, len(data)):
        if cc != b"LIST":
            continue
        kind = bytes(data[ps:ps + 4])
        if kind == b"hdrl":
            for c2, p2, s2 in _walk(data, ps + 4, ps + sz):
                if c2 == b"avih":
                    (usec,) = struct.unpack_from("<I", data, p2)
                    if usec:
                        fps = 1e6 / usec
                elif c2 == b"LIST" and bytes(data[p2:p2 + 4]) == b"strl":
                    for c3, p3, s3 in _walk(data, p2 + 4, p2 + s2):
                        if c3 == b"strh" and bytes(data[p3:p3 + 4]) == b"vids":
                            handler = bytes(data[p3 + 4:p3 + 8])
                            sc, rt = struct.unpack_from("<II", data, p3 + 20)
                            if sc and rt:
                                fps = rt / sc
                        elif c3 == b"strf" and s3 >= 20 and handler is not None:
                            handler = bytes(data[p3 + 16:p3 + 20]) or handler
        elif kind == b"movi":
            for c2, p2, s2 in _walk(data, ps + 4, ps + sz):
                if c2[2:4] in (b"dc", b"db") and s2 > 0:
                    spans.append((p2, s2))
    if handler is None or handler.upper() not in (b"MJPG", b"JPEG"):
        raise ValueError("%s: the video stream is %r, only Motion-JPEG (MJPG) AVI can be decoded without OpenCV" % (path, handler))

    return float(fps or 25.0), MjpegFrames(data, spans), len(spans)


class MjpegFrames:
    """Random-access sequence of the decoded frames (every MJPG frame is a key frame): a rank of a multi-GPU run
    decodes only the frames of its own batches (video.FrameSource)."""

    def __init__(self, data, spans):
        self._data, self._spans = data, spans

    def __len__(self):
        return len(self._spans)

    def compressed(self, i):
        """the JPEG bytes of frame i, not decoded (jpeg.decode_batch_device takes them)"""
        ps, sz = self._spans[i]
        return bytes(self._data[ps:ps + sz])

    def __getitem__(self, i):
        from PIL import Image
        return np.asarray(Image.open(io.BytesIO(self.compressed(i))).convert("RGB"))

    def __iter__(self):
        return (self[i] for i in range(len(self)))
