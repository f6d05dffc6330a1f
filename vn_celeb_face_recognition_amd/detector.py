"""Host-side mirror of the reference's MTCNN detector plugin, backed by libvnface.so.

  MTCNN.__init__   <- /root/reference/models/mtcnn.py:200-227 (same kwargs; cfg/detection/mtcnn.json)
  MTCNN.detect     <- /root/reference/models/mtcnn.py:278-361
  MTCNN.inference  <- /root/reference/models/mtcnn.py:511-513
  MTCNN.forward / select_boxes / extract, fixed_image_standardization
                   <- /root/reference/models/mtcnn.py:229-276,363-518
  crop_rects, extract_face
                   <- /root/reference/models/mtcnn_utils/detect_face.py:309-377
  input handling   <- /root/reference/models/mtcnn_utils/detect_face.py:26-46

The cascade itself (pyramid, P/R/O-Net, NMS, crop/resize, box arithmetic) runs in HIP kernels
behind vnf_mtcnn_detect; frames are uploaded once and stay resident for the alignment warp
(`last_frames_device`).  Results are returned per image as lists of arrays -- the reference's
np.array() of ragged per-image lists raises on NumPy >= 1.24.

Face crops (`mtcnn(img)`, `extract`, `extract_face`) are one vnf_extract_faces launch per call on those resident
frames: the crop rectangles are float32 host arithmetic (`crop_rects`), everything that touches pixels is the kernel,
and the faces come back as cuda tensors (DESIGN.md section 8 lists what differs from the reference).
"""
import ctypes
import os

import numpy as np
import torch

from . import _lib

_WEIGHTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "weights_mtcnn")


def _load_net(name):
    # models/mtcnn.py:32-36 (state_dict files vendored from facenet-pytorch, MIT)
    return torch.load(os.path.join(_WEIGHTS, name + ".pt"), map_location="cpu", weights_only=True)


def _is_batch(img):
    # mtcnn.py:396-400,461-465: a list / tuple or a 4-D array / tensor is a batch, anything else one image
    return isinstance(img, (list, tuple)) or (isinstance(img, (np.ndarray, torch.Tensor)) and len(img.shape) == 4)


def _image_size(img):
    """(width, height) of one image in any input form (detect_face.py:335-339)."""
    if isinstance(img, (np.ndarray, torch.Tensor)):
        return int(img.shape[1]), int(img.shape[0])
    return img.size


def crop_rects(boxes, image_size, margin, width, height):
    """The integer crop rectangles of extract_face (detect_face.py:358-368): boxes (n,4) x1,y1,x2,y2 -> int32 (n,4).
    The margin is in pixels of the OUTPUT image, so it is scaled by box side / (image_size - margin), half of it goes to
    each side, and the result is clamped to the frame and truncated.  All of it in float32, in the reference's order of
    operations: what its scalar arithmetic on rows of a float32 box array gives under NumPy 2 (NumPy 1.x promoted to
    float64 there).  A rectangle that comes out empty -- the reference's interpolate raises on it -- is a ValueError
    that names the box."""
    b = np.asarray(boxes, dtype=np.float32).reshape(-1, 4)
    f32 = np.float32
    with np.errstate(all="ignore"):
        m0 = f32(margin) * (b[:, 2] - b[:, 0]) / f32(image_size - margin)
        m1 = f32(margin) * (b[:, 3] - b[:, 1]) / f32(image_size - margin)
        r = np.stack([np.maximum(b[:, 0] - m0 / f32(2), f32(0)), np.maximum(b[:, 1] - m1 / f32(2), f32(0)),
                      np.minimum(b[:, 2] + m0 / f32(2), f32(width)), np.minimum(b[:, 3] + m1 / f32(2), f32(height))], axis=1)
    bad = ~np.isfinite(r).all(axis=1)
    r = np.where(np.isfinite(r), r, 0).astype(np.int64).astype(np.int32)       # int(): truncation toward zero
    bad |= (r[:, 2] <= r[:, 0]) | (r[:, 3] <= r[:, 1])
    if bad.any():
        k = int(np.flatnonzero(bad)[0])
        raise ValueError("box %d %s gives an empty crop in a %dx%d image (image_size %d, margin %d)"
                         % (k, b[k].tolist(), width, height, image_size, margin))
    return r


_MAX_BIN = 1 << 15      # vnf_extract_faces: pixels per bin, exclusive


def extract_faces_device(frames, rects, image_size, standardize=True, dtype=torch.float32, want_u8=False):
    """vnf_extract_faces: frames cuda u8 (B,H,W,3); rects int (n,5) host rows [frame, x1, y1, x2, y2] -> (x, u8):
    x cuda (n,3,S,S) of `dtype` (float(byte), or (byte - 127.5) / 128 with standardize) and, with want_u8, the bytes
    (n,S,S,3) (else None).  The rows are checked here, where they can be seen; then one upload and one launch on the
    current stream."""
    if frames.device.type != "cuda":
        raise RuntimeError("extract_faces_device runs on MI355X only: frames must live on a cuda device (there is no CPU path)")
    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3:
        raise ValueError("frames must be uint8 (B,H,W,3), got %s %s" % (frames.dtype, tuple(frames.shape)))
    frames = frames.contiguous()
    b, h, w, _ = frames.shape
    s = int(image_size)
    rects = np.ascontiguousarray(rects, dtype=np.int32).reshape(-1, 5)
    n = len(rects)
    if n:
        fr, x1, y1, x2, y2 = (rects[:, i].astype(np.int64) for i in range(5))
        bad = (fr < 0) | (fr >= b) | (x1 < 0) | (y1 < 0) | (x2 <= x1) | (y2 <= y1) | (x2 > w) | (y2 > h)
        if bad.any():
            k = int(np.flatnonzero(bad)[0])
            raise ValueError("rectangle %d %s is empty or outside the %d frames of %dx%d" % (k, rects[k].tolist(), b, w, h))
        if s >= 1:
            deep = (-(-(y2 - y1) // s) + 1) * (-(-(x2 - x1) // s) + 1) >= _MAX_BIN
            if deep.any():
                k = int(np.flatnonzero(deep)[0])
                raise _lib.VnfError("VNF_E_INVALID: rectangle %d %s resampled to %d has bins of 2^15 pixels or more"
                                    % (k, rects[k].tolist(), s))
    dev = frames.device
    x = torch.empty((n, 3, s, s), dtype=dtype, device=dev)
    u8 = torch.empty((n, s, s, 3), dtype=torch.uint8, device=dev) if want_u8 else None
    if n:
        rdev = torch.from_numpy(rects).to(dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.load().vnf_extract_faces(
                ctypes.c_void_p(frames.data_ptr()), b, h, w, ctypes.c_void_p(rdev.data_ptr()), n, s, 1 if standardize else 0,
                ctypes.c_void_p(x.data_ptr()), _lib.torch_dtype_code(dtype),
                ctypes.c_void_p(u8.data_ptr()) if u8 is not None else None, _lib.current_stream_ptr()))
    return x, u8


def _save_face(face_u8, path):
    from PIL import Image
    d = os.path.dirname(path)
    if d:
        os.makedirs(d, exist_ok=True)
    Image.fromarray(face_u8).save(path)


def extract_face(img, box, image_size=160, margin=0, save_path=None):
    """detect_face.py:342-378 for one image in any input form and one box: the cuda (3,S,S) float32 tensor of the crop's
    bytes (not standardised), resampled on the device the image lives on (the current cuda device for host images).
    Every input form takes the reference's tensor path (area resampling)."""
    if isinstance(img, torch.Tensor) and img.device.type == "cuda":
        frames = img
    else:
        if not torch.cuda.is_available():
            raise RuntimeError("extract_face runs on MI355X only (there is no CPU path)")
        a = img if isinstance(img, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(img)))
        frames = a.to(torch.device("cuda", torch.cuda.current_device()))
    if frames.dim() != 3 or frames.shape[2] != 3:
        raise ValueError("expected one HWC RGB image, got shape %s" % (tuple(frames.shape),))
    frames = frames.to(torch.uint8).unsqueeze(0)
    h, w = int(frames.shape[1]), int(frames.shape[2])
    r = crop_rects(np.asarray(box, dtype=np.float32).reshape(1, 4), image_size, margin, w, h)
    x, u8 = extract_faces_device(frames, np.concatenate([np.zeros((1, 1), np.int32), r], axis=1), image_size,
                                 standardize=False, want_u8=save_path is not None)
    if save_path is not None:
        _save_face(u8[0].cpu().numpy(), save_path)
    return x[0]


def fixed_image_standardization(image_tensor):
    # mtcnn.py:516-518
    return (image_tensor - 127.5) / 128.0


class _Detector:
    """What the detector plugins share: the library handle and its life time, the input forms, and the two result paths
    of a detection -- host arrays with the capacity retry (`_detect_device`) and device tensors (`results_device`).  A
    subclass names its two library functions and brings `_ensure(b, h, w)`, which creates the handle."""
    _detect_fn = None       # vnf_*_detect
    _results_fn = None      # vnf_*_results_device
    _handle = None
    _handle_key = None
    _frames = None

    def eval(self):
        return self

    def to(self, device):
        self.device = torch.device(device)
        return self

    def __del__(self):
        try:
            self._drop()
        except Exception:
            pass

    def _drop(self):
        if self._handle is not None:
            _lib.load().vnf_destroy(self._handle)
            self._handle = None

    # ---- input handling (detect_face.py:26-46)
    def _to_device_frames(self, img):
        single = False
        if isinstance(img, torch.Tensor):
            t = img
            if t.dim() == 3:
                t, single = t.unsqueeze(0), True
        elif isinstance(img, np.ndarray):
            a = img
            if a.ndim == 3:
                a, single = a[None], True
            t = torch.from_numpy(np.ascontiguousarray(a))
        else:
            if not isinstance(img, (list, tuple)):
                img, single = [img], True
            arrs = [np.asarray(i) for i in img]
            if any(a.shape != arrs[0].shape for a in arrs):
                raise Exception("MTCNN batch processing only compatible with equal-dimension images.")
            t = torch.from_numpy(np.stack([np.uint8(a) for a in arrs]))
        if t.dim() != 4 or t.shape[3] != 3:
            raise ValueError("expected HWC RGB images, got shape %s" % (tuple(t.shape),))
        if t.dtype != torch.uint8:
            t = t.to(torch.uint8)
        return t.to(self.device, non_blocking=False).contiguous(), single

    def last_frames_device(self):
        """(B,H,W,3) uint8 cuda tensor of the frames of the last detect() call (kept for the warp)."""
        return self._frames

    def _grow(self, lib):
        """A detection failed with VNF_E_CAPACITY although the output arrays were large enough: a subclass that can
        enlarge its handle for it does so and returns True (the batch then runs again)."""
        return False

    def _detect_device(self, frames, cap):
        """frames: (B,H,W,3) u8 cuda; cap: first size of the output arrays, grown to what the library reports.  Returns
        (counts list, boxes (n,4), probs (n,), points (n,5,2)) on host."""
        b, h, w, _ = frames.shape
        hd = self._ensure(b, h, w)
        lib = _lib.load()
        while True:
            counts = np.zeros(b, dtype=np.int32)
            boxes = np.empty((cap, 4), dtype=np.float32)
            probs = np.empty((cap,), dtype=np.float32)
            points = np.empty((cap, 10), dtype=np.float32)
            n_out = ctypes.c_int32(0)
            with torch.cuda.device(frames.device):
                rc = getattr(lib, self._detect_fn)(hd, ctypes.c_void_p(frames.data_ptr()), b, h, w, counts.ctypes.data,
                                                   boxes.ctypes.data, probs.ctypes.data, points.ctypes.data, cap,
                                                   ctypes.byref(n_out), _lib.current_stream_ptr())
            if rc == -4 and n_out.value > cap:
                cap = int(n_out.value)
                continue
            if rc == -4 and self._grow(lib):
                hd = self._ensure(b, h, w)
                continue
            _lib.check(rc)
            n = n_out.value
            return counts.tolist(), boxes[:n], probs[:n], points[:n].reshape(n, 5, 2)

    def _require_handle(self):
        if self._handle is None:
            raise RuntimeError("results_device(): no detection has run on this detector yet")
        return self._handle

    def results_device(self, n, device=None):
        """Device-resident copy of the last detect_device() on this handle: (frame_idx (n,) int32, boxes (n,4),
        probs (n,), points (n,10)) cuda tensors filled on the current stream -- the inputs of vnf_align, without
        the host round trip."""
        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        fidx = torch.empty((n,), dtype=torch.int32, device=dev)
        boxes = torch.empty((n, 4), dtype=torch.float32, device=dev)
        probs = torch.empty((n,), dtype=torch.float32, device=dev)
        points = torch.empty((n, 10), dtype=torch.float32, device=dev)
        if n:
            with torch.cuda.device(dev):
                _lib.check(getattr(_lib.load(), self._results_fn)(
                    self._require_handle(), ctypes.c_void_p(fidx.data_ptr()), ctypes.c_void_p(boxes.data_ptr()),
                    ctypes.c_void_p(probs.data_ptr()), ctypes.c_void_p(points.data_ptr()), n, _lib.current_stream_ptr()))
        return fidx, boxes, probs, points


class MTCNN(_Detector):
    _detect_fn, _results_fn = "vnf_mtcnn_detect", "vnf_mtcnn_results_device"

    def __init__(self, image_size=160, margin=0, min_face_size=20, thresholds=[0.6, 0.7, 0.7], factor=0.709,
                 post_process=True, select_largest=True, selection_method=None, keep_all=False, device=None,
                 max_batch=16, max_height=1080, max_width=1920, state_dicts=None, max_candidates=0):
        self.image_size = image_size
        self.margin = margin
        self.min_face_size = int(min_face_size)
        self.thresholds = [float(t) for t in thresholds]
        self.factor = float(factor)
        self.post_process = post_process
        self.select_largest = select_largest
        self.keep_all = keep_all
        self.selection_method = selection_method or ('largest' if select_largest else 'probability')
        self.training = False
        self._sd = state_dicts or tuple(_load_net(n) for n in ("pnet", "rnet", "onet"))
        self._cap = [int(max_batch), int(max_height), int(max_width)]
        self._max_candidates = int(max_candidates)    # vnf_mtcnn_cfg.max_candidates: rows per frame of the stage tables (0: 2048); grows on overflow
        self.device = torch.device('cpu')
        if device is not None:
            self.to(device)

    def _ensure(self, b, h, w):
        if self.device.type != "cuda":
            raise RuntimeError("MTCNN runs on MI355X only: construct it with device='cuda:0' (there is no CPU path)")
        self._cap = [max(self._cap[0], b), max(self._cap[1], h), max(self._cap[2], w)]
        dev = self.device.index if self.device.index is not None else torch.cuda.current_device()
        key = (dev, tuple(self._cap))
        if self._handle is not None and self._handle_key == key:
            return self._handle
        self._drop()
        lib = _lib.load()
        with torch.cuda.device(dev):
            _lib.check(lib.vnf_init(dev))
            cfg = _lib.MtcnnCfg()
            cfg.min_face_size = self.min_face_size
            for i in range(3):
                cfg.thresholds[i] = self.thresholds[i]
            cfg.factor = self.factor
            cfg.select_largest = 1 if self.select_largest else 0
            cfg.max_batch, cfg.max_height, cfg.max_width = self._cap
            cfg.max_candidates = self._max_candidates
            (dp, np_, kp), (dr, nr, kr), (do, no, ko) = (_lib.make_descs(sd) for sd in self._sd)
            h_ = ctypes.c_void_p()
            _lib.check(lib.vnf_mtcnn_create(dp, np_, dr, nr, do, no, ctypes.byref(cfg), ctypes.byref(h_)))
            del kp, kr, ko
        self._handle, self._handle_key = h_, key
        return h_

    def detect_device(self, frames):
        """frames: (B,H,W,3) u8 cuda.  Returns (counts list, boxes (n,4), probs (n,), points (n,5,2)) on host."""
        return self._detect_device(frames, 256)

    def _grow(self, lib):
        if b"candidate table overflow" not in lib.vnf_last_error() or self._max_candidates >= (1 << 20):
            return False
        # a frame with more stage-1 survivors than the stage tables have rows (the reference has no cap,
        # detect_face.py:79-93): grow the tables and run the batch again -- like a vector, never a truncation
        self._max_candidates = max(4096, 2 * max(self._max_candidates, 2048))
        self._handle_key = None
        return True

    def stage_times(self, frames, reps=5):
        """Per-stage device time of one detection (vnf_mtcnn_stage_times: HIP events between the stages on the
        current stream).  frames: (B,H,W,3) u8 cuda.  Returns {stage: {"ms": median over reps, "bytes": algorithmic
        bytes of the launch}}; kernels stages carry their kernel's name (pyramid, pnet_conv1_pool, ...)."""
        b, h, w, _ = frames.shape
        hd = self._ensure(b, h, w)
        lib = _lib.load()
        acc = {}
        for _ in range(reps):
            buf = ctypes.create_string_buffer(1 << 14)
            with torch.cuda.device(frames.device):
                _lib.check(lib.vnf_mtcnn_stage_times(hd, ctypes.c_void_p(frames.data_ptr()), b, h, w, buf, len(buf),
                                                     _lib.current_stream_ptr()))
            seen = {}
            for line in buf.value.decode().splitlines():
                name, ms, nbytes = line.split()
                e = seen.setdefault(name, [0.0, 0.0])     # chunked stages repeat: sum within one call
                e[0] += float(ms)
                e[1] += float(nbytes)
            for name, (ms, nbytes) in seen.items():
                acc.setdefault(name, {"ms": [], "bytes": nbytes})["ms"].append(ms)
        return {k: {"ms": float(np.median(v["ms"])), "bytes": v["bytes"]} for k, v in acc.items()}

    def debug_stage3(self, boxes, onet_out):
        """O-stage decode alone (vnf_mtcnn_debug_stage3) on a caller-made single-frame candidate table: boxes (n,4)
        before bbreg, onet_out (n,15) [prob, reg x4, landmark x x5, landmark y x5] -> (boxes (k,4), probs (k,),
        points (k,5,2)) after threshold, bbreg, "Min" NMS and the area ordering.  Test hook for tied scores."""
        boxes = np.ascontiguousarray(boxes, dtype=np.float32).reshape(-1, 4)
        oo = np.ascontiguousarray(onet_out, dtype=np.float32).reshape(-1, 15)
        n = boxes.shape[0]
        hd = self._ensure(1, 64, 64)
        fin = np.empty((max(n, 1), 15), dtype=np.float32)
        n_out = ctypes.c_int32(0)
        dev = self.device.index if self.device.index is not None else torch.cuda.current_device()
        with torch.cuda.device(dev):
            _lib.check(_lib.load().vnf_mtcnn_debug_stage3(hd, boxes.ctypes.data, oo.ctypes.data, n, fin.ctypes.data,
                                                          fin.shape[0], ctypes.byref(n_out), _lib.current_stream_ptr()))
        fin = fin[:n_out.value]
        return fin[:, :4].copy(), fin[:, 4].copy(), fin[:, 5:].reshape(-1, 5, 2).copy()

    def detect(self, img, landmarks=False):
        frames, single = self._to_device_frames(img)
        return self._detect_frames(frames, single, landmarks)

    def _detect_frames(self, frames, single, landmarks):
        self._frames = frames
        counts, bx, pr, pt = self.detect_device(frames)
        boxes, probs, points = [], [], []
        o = 0
        for c in counts:
            if c == 0:
                boxes.append([]); probs.append([]); points.append([])   # mtcnn.py:330-333
            else:
                boxes.append(bx[o:o + c].copy()); probs.append(pr[o:o + c].copy()); points.append(pt[o:o + c].copy())
            o += c
        if single:
            boxes, probs, points = boxes[0], probs[0], points[0]
        if landmarks:
            return boxes, probs, points
        return boxes, probs

    def inference(self, rgb_image, landmark=True):
        return self.detect(rgb_image, landmark)

    # ---- selection (mtcnn.py:363-456)
    def select_boxes(self, all_boxes, all_probs, all_points, imgs, method='probability', threshold=0.9, center_weight=2.0):
        """One box per image by `method`: 'probability', 'largest', 'largest_over_threshold' (largest among probs >
        threshold) or 'center_weighted_size' (area minus center_weight x squared distance of the box centre from the
        image centre).  Returns (boxes, probs, points): per image a (1,4) / (1,) / (1,5,2) array, or None / [None] / None
        for an image without a (qualifying) box; lists in batch mode, the single image's entries (prob a scalar or
        None) otherwise.  Two reference defects are not reproduced: 'largest_over_threshold' filters probs and points
        with the boxes (mtcnn.py:431-442 filters the boxes only), and the image size is taken from any input form
        (mtcnn.py:425 reads PIL's .width)."""
        batch_mode = _is_batch(imgs)
        if not batch_mode:
            imgs, all_boxes, all_probs, all_points = [imgs], [all_boxes], [all_probs], [all_points]
        if method not in ('probability', 'largest', 'largest_over_threshold', 'center_weighted_size'):
            raise ValueError("select_boxes: unknown method %r" % (method,))
        sel_boxes, sel_probs, sel_points = [], [], []
        for boxes, probs, points, img in zip(all_boxes, all_probs, all_points, imgs):
            boxes, probs, points = np.array(boxes), np.array(probs), np.array(points)
            if len(boxes) and method == 'largest_over_threshold':
                keep = probs > threshold
                boxes, probs, points = boxes[keep], probs[keep], points[keep]
            if len(boxes) == 0:
                sel_boxes.append(None); sel_probs.append([None]); sel_points.append(None)
                continue
            area = (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])
            if method == 'probability':
                score = probs
            elif method == 'center_weighted_size':
                w, h = _image_size(img)
                offsets = np.stack([(boxes[:, 0] + boxes[:, 2]) / 2, (boxes[:, 1] + boxes[:, 3]) / 2], axis=1) - (w / 2, h / 2)
                score = area - np.sum(np.power(offsets, 2.0), 1) * center_weight
            else:
                score = area
            first = np.argsort(score)[::-1][[0]]
            sel_boxes.append(boxes[first]); sel_probs.append(probs[first]); sel_points.append(points[first])
        if not batch_mode:
            return sel_boxes[0], sel_probs[0][0], sel_points[0]
        return sel_boxes, sel_probs, sel_points

    # ---- extraction (mtcnn.py:458-509)
    def extract(self, img, batch_boxes, save_path, dtype=torch.float32):
        """Faces of `img` at `batch_boxes` (as detect() or select_boxes() return them): per image a cuda (n,3,S,S) tensor
        with keep_all, else (3,S,S) of row 0, or None for an image without boxes; a list in batch mode.  Values are
        float(byte), or (byte - 127.5) / 128 with post_process, in `dtype` (float32; bfloat16 / float16 for an encoder's
        16-bit input).  One upload of the rectangle table and one launch for all images; the results are views of one
        buffer.  save_path: a string (single image) or a list with one entry per image (None entries allowed); face
        i > 0 of an image goes to <name>_<i+1><ext>.  The saved picture holds the un-standardised bytes."""
        if self.device.type != "cuda":
            raise RuntimeError("MTCNN runs on MI355X only: construct it with device='cuda:0' (there is no CPU path)")
        frames, single = self._to_device_frames(img)
        return self._extract_frames(frames, single, batch_boxes, save_path, dtype)

    def _extract_frames(self, frames, single, batch_boxes, save_path, dtype=torch.float32):
        b, h, w, _ = frames.shape
        if single:
            batch_boxes = [batch_boxes]
        if len(batch_boxes) != b:
            raise ValueError("extract: %d images but %d box entries" % (b, len(batch_boxes)))
        if save_path is None:
            paths = [None] * b
        else:
            paths = [save_path] if isinstance(save_path, str) else list(save_path)
            if len(paths) != b:
                raise ValueError("extract: save_path needs one entry per image (%d images, %d paths)" % (b, len(paths)))
        rects, counts = [], []
        for k, box_im in enumerate(batch_boxes):
            n = 0 if box_im is None else len(box_im)
            if n:
                box_im = np.asarray(box_im, dtype=np.float32).reshape(-1, 4)
                if not self.keep_all:
                    box_im = box_im[[0]]
                r = crop_rects(box_im, self.image_size, self.margin, w, h)
                rects.append(np.concatenate([np.full((len(r), 1), k, np.int32), r], axis=1))
                n = len(r)
            counts.append(n)
        rects = np.concatenate(rects) if rects else np.zeros((0, 5), np.int32)
        want_u8 = any(p is not None and c for p, c in zip(paths, counts))
        x, u8 = extract_faces_device(frames, rects, self.image_size, standardize=self.post_process, dtype=dtype, want_u8=want_u8)
        u8_host = u8.cpu().numpy() if want_u8 else None          # the call's only device-to-host copy
        faces, o = [], 0
        for c, path in zip(counts, paths):
            if c == 0:
                faces.append(None)
                continue
            if path is not None:
                for i in range(c):
                    _save_face(u8_host[o + i], path if i == 0 else "%s_%d%s" % (os.path.splitext(path)[0], i + 1, os.path.splitext(path)[1]))
            faces.append(x[o:o + c] if self.keep_all else x[o])
            o += c
        return faces[0] if single else faces

    # ---- mtcnn.py:229-276
    def forward(self, img, save_path=None, return_prob=False, extract_face=True):
        """Detect, select (without keep_all) and extract: (faces, boxes) or (faces, boxes, probs) -- this fork returns
        the boxes too (mtcnn.py:273-276).  faces are cuda float32 tensors on the detector's device, ready for the
        encoder; the frames are uploaded once for detection and cropping."""
        frames, single = self._to_device_frames(img)
        batch_boxes, batch_probs, batch_points = self._detect_frames(frames, single, True)
        if not self.keep_all:
            batch_boxes, batch_probs, batch_points = self.select_boxes(batch_boxes, batch_probs, batch_points,
                                                                       frames[0] if single else frames,
                                                                       method=self.selection_method)
        faces = self._extract_frames(frames, single, batch_boxes, save_path) if extract_face else None
        if return_prob:
            return faces, batch_boxes, batch_probs
        return faces, batch_boxes

    __call__ = forward

    def debug_pnet_level(self, img, level):
        """Dense pyramid level, P-Net prob and reg maps of one level for one image (staged parity tests)."""
        frames, _ = self._to_device_frames(img)
        b, h, w, _ = frames.shape
        hd = self._ensure(1, h, w)
        lib = _lib.load()
        big = h * w + 16
        lvl = np.empty(3 * big, np.float32); prob = np.empty(big, np.float32); reg = np.empty(4 * big, np.float32)
        dims = (ctypes.c_int32 * 4)()
        with torch.cuda.device(frames.device):
            _lib.check(lib.vnf_mtcnn_debug_pnet(hd, ctypes.c_void_p(frames.data_ptr()), h, w, level, lvl.ctypes.data,
                                                prob.ctypes.data, reg.ctypes.data, dims, _lib.current_stream_ptr()))
        hs, ws, oh, ow = (int(d) for d in dims)
        return (lvl[:3 * hs * ws].reshape(3, hs, ws), prob[:oh * ow].reshape(oh, ow), reg[:4 * oh * ow].reshape(4, oh, ow))

    def debug_net(self, frames, net, rects, counts):
        """R-Net (net 2) or O-Net (net 3) alone, through the cascade's own launch sequence (vnf_mtcnn_debug_net), on a
        caller-made candidate table: frames (b,H,W,3) u8, rects (total,4) int32 y, ey, x, ex as pad() returns them
        (frame 0's rows first), counts (b,) rectangles per frame.  Returns the (total,nf) fp32 table, rows [prob,
        values...] (nf 5 / 15); the kernels' status word of the call is left in `debug_status`."""
        frames, _ = self._to_device_frames(frames)
        b, h, w, _ = frames.shape
        rects = np.ascontiguousarray(rects, dtype=np.int32).reshape(-1, 4)
        counts = np.ascontiguousarray(counts, dtype=np.int32).reshape(-1)
        if len(counts) != b or int(counts.sum()) != len(rects):
            raise ValueError("debug_net: %d frames, %d counts that sum to %d, %d rectangles" % (b, len(counts), int(counts.sum()), len(rects)))
        hd = self._ensure(min(b, self._cap[0]), min(h, self._cap[1]), min(w, self._cap[2]))   # beyond the capacity: the library refuses
        table = np.zeros((len(rects), 5 if net == 2 else 15), dtype=np.float32)
        status = ctypes.c_int32(0)
        with torch.cuda.device(frames.device):
            _lib.check(_lib.load().vnf_mtcnn_debug_net(hd, int(net), ctypes.c_void_p(frames.data_ptr()), b, h, w, rects.ctypes.data,
                                                       counts.ctypes.data, table.ctypes.data, ctypes.byref(status),
                                                       _lib.current_stream_ptr()))
        self._frames = frames
        self.debug_status = int(status.value)
        return table

    def debug_net_tap(self, net, name):
        """One buffer of the last chunk of the previous debug_net on this net (vnf_mtcnn_debug_net_tap): (raw int32 array
        (n,H,W,C), split, c0) -- split: a word is a split-f16 (hi, lo) pair instead of an fp32 value; c0: dense index
        of the chunk's first candidate.  Names: crops, pool1, conv2, pool2, conv3, pool3, conv4, dense, heads."""
        hd = self._ensure(1, 12, 12)   # the handle of the previous call (the capacity only ever grows), or a fresh one: the library refuses
        lib = _lib.load()
        dims = (ctypes.c_int32 * 6)()
        _lib.check(lib.vnf_mtcnn_debug_net_tap(hd, int(net), name.encode(), None, 0, dims))
        n, H, W, C, split, c0 = (int(d) for d in dims)
        raw = np.empty((n, H, W, C), dtype=np.int32)
        dev = self.device.index if self.device.index is not None else torch.cuda.current_device()
        with torch.cuda.device(dev):
            _lib.check(lib.vnf_mtcnn_debug_net_tap(self._handle, int(net), name.encode(), raw.ctypes.data, raw.nbytes, dims))
        return raw, bool(split), c0
