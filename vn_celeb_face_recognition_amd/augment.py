"""transforms_facenet_aug on the device: /root/reference/data_loader/__init__.py:27-34,52-65,84-89.

  transforms_facenet_aug = RandomRotation((-10, 10), resample=BICUBIC) -> RandomCrop(160, padding=2, pad_if_needed=True)
                           -> RandomHorizontalFlip(0.5) -> np.float32 -> (v - 127.5) / 128 -> CHW

The reference runs it per image in PIL / torchvision on the host.  Here the random draws stay on the host (torch's
global CPU generator, in a pinned order) and everything that touches pixels is one kernel, vnf_augment_faces
(csrc/augment.hip), over a data set that lives on the device as u8.

This module holds three things:
  - the SPECIFICATION of the pixel work, pillow_facenet_aug: a NumPy restatement of what Pillow's Image.rotate(angle,
    BICUBIC), ImageOps.expand, Image.crop and Image.transpose(FLIP_LEFT_RIGHT) compute, byte for byte (checked against
    Pillow in tests/test_augment_host.py; the kernel is checked against the same bytes);
  - the draw order, draw_facenet_aug_params ("parity unpinned", DESIGN.md 3: torchvision is not available to replay);
  - the device entry, augment_faces_device, and the transforms_dict names train.py accepts.

The target size T is the encoder's input size (160 for InceptionResnetV1, 112 for iresnet100), where the reference
fixes 160 (data_loader/__init__.py:9)."""
import ctypes
import math

import numpy as np
import torch

from . import _lib

PADDING = 2          # RandomCrop(padding=2)
DEGREES = (-10.0, 10.0)
FLIP_P = 0.5


class AugParam(ctypes.Structure):
    """vnf_aug_param (include/vnface.h): the rotation matrix of one sample, its crop origin (row i, column j) in the
    padded image, the flip flag and the padding P per side."""
    _fields_ = [("m", ctypes.c_double * 6), ("i", ctypes.c_int32), ("j", ctypes.c_int32), ("flip", ctypes.c_int32),
                ("pad", ctypes.c_int32)]


AUG_PARAM_DTYPE = np.dtype([("m", np.float64, (6,)), ("i", np.int32), ("j", np.int32), ("flip", np.int32),
                            ("pad", np.int32)])
assert AUG_PARAM_DTYPE.itemsize == ctypes.sizeof(AugParam) == 64


def crop_padding(s, t):
    """RandomCrop(t, padding=2, pad_if_needed=True) on an s x s image: zero border per side.  pad_if_needed pads BOTH
    sides by the whole shortfall of the already padded image (torchvision transforms.py RandomCrop.forward)."""
    return PADDING + max(0, t - (s + 2 * PADDING))


def rotate_matrix(angle, s):
    """The affine matrix Image.rotate(angle) hands to Image.transform for an s x s image (PIL/Image.py rotate):
    output pixel centre -> input position, rotation about (s/2, s/2)."""
    angle = angle % 360.0
    a = -math.radians(angle)
    m = [round(math.cos(a), 15), round(math.sin(a), 15), 0.0, round(-math.sin(a), 15), round(math.cos(a), 15), 0.0]
    cx = cy = s / 2.0
    m[2] = m[0] * -cx + m[1] * -cy + m[2]
    m[5] = m[3] * -cx + m[4] * -cy + m[5]
    m[2] += cx
    m[5] += cy
    return m


def _bicubic(v1, v2, v3, v4, d):
    # libImaging/Geometry.c BICUBIC (a = -1), in this operation order
    p1 = v2
    p2 = -v1 + v3
    p3 = 2 * (v1 - v2) + v3 - v4
    p4 = -v1 + v2 - v3 + v4
    return p1 + d * (p2 + d * (p3 + d * p4))


def pillow_rotate_bicubic(face, m):
    """ImagingGenericTransform with affine_transform + bicubic_filter32RGB (libImaging/Geometry.c) on an (S,S,3) u8
    image: fill 0, taps clamped in x, the first row clamped and each later row outside the image repeating the row
    before it, double arithmetic, truncation (not rounding) to u8."""
    face = np.asarray(face)
    s = face.shape[0]
    if face.shape != (s, s, 3) or face.dtype != np.uint8:
        raise ValueError("expected a square (S,S,3) uint8 image, got %s %s" % (face.shape, face.dtype))
    src = face.astype(np.float64)
    ys, xs = np.meshgrid(np.arange(s, dtype=np.float64) + 0.5, np.arange(s, dtype=np.float64) + 0.5, indexing="ij")
    xin = m[0] * xs + m[1] * ys + m[2]
    yin = m[3] * xs + m[4] * ys + m[5]
    inside = (xin >= 0.0) & (xin < s) & (yin >= 0.0) & (yin < s)
    xin = xin - 0.5
    yin = yin - 0.5
    x0 = np.floor(xin)
    y0 = np.floor(yin)
    dx = (xin - x0)[..., None]
    dy = (yin - y0)[..., None]
    x = x0.astype(np.int64) - 1
    y = y0.astype(np.int64) - 1
    cols = [np.clip(x + k, 0, s - 1) for k in range(4)]

    def row(r):
        return _bicubic(src[r, cols[0]], src[r, cols[1]], src[r, cols[2]], src[r, cols[3]], dx)

    v = [row(np.clip(y, 0, s - 1))]
    for k in (1, 2, 3):
        ok = ((y + k >= 0) & (y + k < s))[..., None]
        v.append(np.where(ok, row(np.clip(y + k, 0, s - 1)), v[-1]))
    out = _bicubic(v[0], v[1], v[2], v[3], dy)
    res = np.where(out <= 0.0, 0.0, np.where(out >= 255.0, 255.0, np.trunc(out)))
    return np.where(inside[..., None], res, 0.0).astype(np.uint8)


def pillow_facenet_aug(face, angle, i, j, flip, t):
    """The specification: (S,S,3) u8 face -> (t,t,3) u8, rotated by `angle` degrees, zero-padded, cropped at row i /
    column j of the padded image, mirrored when flip.  Normalisation is left to the caller ((v - 127.5) / 128)."""
    face = np.asarray(face)
    s = face.shape[0]
    p = crop_padding(s, t)
    if not (0 <= i <= s + 2 * p - t and 0 <= j <= s + 2 * p - t):
        raise ValueError("crop origin (%d, %d) outside [0, %d]" % (i, j, s + 2 * p - t))
    rot = pillow_rotate_bicubic(face, rotate_matrix(angle, s))
    padded = np.zeros((s + 2 * p, s + 2 * p, 3), np.uint8)
    padded[p:p + s, p:p + s] = rot
    out = padded[i:i + t, j:j + t]
    return np.ascontiguousarray(out[:, ::-1] if flip else out)


def normalise(u8_hwc):
    """np.float32 -> fix_std -> to_tensor of data_loader/__init__.py:27-34 for (..., H, W, 3) u8: (..., 3, H, W) f32."""
    a = (np.asarray(u8_hwc).astype(np.float32) - np.float32(127.5)) / np.float32(128.0)
    return np.ascontiguousarray(np.moveaxis(a, -1, -3))


def draw_facenet_aug_params(n, s, t):
    """The random state of n samples, drawn per sample from torch's global CPU generator in the order torchvision's
    transforms consume it: RandomRotation.get_params (torch.empty(1).uniform_(-10, 10)), RandomCrop.get_params
    (torch.randint(0, h - t + 1, (1,)) for the row, then the same for the column; neither is drawn when the padded image
    is exactly t x t), RandomHorizontalFlip (torch.rand(1) < 0.5).  Returns (params, angles): params is an
    AUG_PARAM_DTYPE array for augment_faces_device, angles the drawn degrees (float64) for the specification."""
    p = crop_padding(s, t)
    size = s + 2 * p
    if size < t:
        raise ValueError("padded size %d is smaller than the crop %d" % (size, t))
    params = np.zeros(n, AUG_PARAM_DTYPE)
    angles = np.zeros(n, np.float64)
    for k in range(n):
        angle = float(torch.empty(1).uniform_(DEGREES[0], DEGREES[1]).item())
        if size == t:
            i = j = 0
        else:
            i = int(torch.randint(0, size - t + 1, size=(1,)).item())
            j = int(torch.randint(0, size - t + 1, size=(1,)).item())
        flip = bool(torch.rand(1) < FLIP_P)
        angles[k] = angle
        params[k] = (rotate_matrix(angle, s), i, j, int(flip), p)
    return params, angles


def identity_params(n, s, t):
    """transforms_default as augmentation parameters: no rotation, the crop exactly on the image, no flip."""
    if s != t:
        raise ValueError("the default transform does not resize: faces are %dx%d, the encoder takes %dx%d" % (s, s, t, t))
    p = crop_padding(s, t)
    params = np.zeros(n, AUG_PARAM_DTYPE)
    params["m"] = rotate_matrix(0.0, s)
    params["i"] = params["j"] = params["pad"] = p
    return params


def make_params(angles, i, j, flip, s, t):
    """AUG_PARAM_DTYPE array from explicit per-sample values (tests, tools)."""
    angles = np.atleast_1d(np.asarray(angles, np.float64))
    params = np.zeros(len(angles), AUG_PARAM_DTYPE)
    params["m"] = [rotate_matrix(float(a), s) for a in angles]
    params["i"], params["j"], params["flip"] = i, j, np.asarray(flip, np.int32)
    params["pad"] = crop_padding(s, t)
    return params


def check_params(params, s, t):
    """The host check of vnf_augment_faces' per-sample values, which the library cannot see (they live in device
    memory by the time it is called): padding >= 0 and every crop origin inside [0, S + 2 pad - T]."""
    hi = s + 2 * params["pad"].astype(np.int64) - t
    bad = (params["pad"] < 0) | (params["i"] < 0) | (params["j"] < 0) | (params["i"] > hi) | (params["j"] > hi)
    if bad.any():
        k = int(np.flatnonzero(bad)[0])
        raise ValueError("augmentation parameter %d: crop origin (%d, %d) with padding %d is outside [0, %d] (S=%d, T=%d)"
                         % (k, params["i"][k], params["j"][k], params["pad"][k], hi[k], s, t))


def augment_faces_device(faces_dev, index, params, t, dtype=torch.float32, want_u8=False):
    """vnf_augment_faces: faces_dev cuda u8 (n_faces,S,S,3); index None or int32 (n,) of rows of faces_dev (host or
    cuda); params an AUG_PARAM_DTYPE array (or a cuda u8 tensor of its bytes) of n entries -> cuda (n,3,t,t) of `dtype`,
    and the augmented bytes (n,t,t,3) u8 when want_u8.  One launch on the current stream; the only other device work
    is the upload of params and index."""
    if faces_dev.device.type != "cuda":
        raise RuntimeError("augment_faces_device runs on MI355X only: faces must live on a cuda device (there is no CPU path)")
    if faces_dev.dtype != torch.uint8 or faces_dev.dim() != 4 or faces_dev.shape[1] != faces_dev.shape[2] or faces_dev.shape[3] != 3:
        raise ValueError("faces must be uint8 (n_faces,S,S,3), got %s %s" % (faces_dev.dtype, tuple(faces_dev.shape)))
    dev = faces_dev.device
    faces_dev = faces_dev.contiguous()
    if isinstance(params, torch.Tensor):
        pdev = params.to(dev).contiguous()
        n = pdev.numel() // AUG_PARAM_DTYPE.itemsize
    else:
        params = np.ascontiguousarray(params, dtype=AUG_PARAM_DTYPE)
        n = len(params)
        check_params(params, int(faces_dev.shape[1]), int(t))
        pdev = torch.from_numpy(params.view(np.uint8).reshape(-1).copy()).to(dev)
    idev = None
    if index is not None:
        idev = torch.as_tensor(index).to(device=dev, dtype=torch.int32).contiguous()
        if idev.numel() != n:
            raise ValueError("index has %d entries, params %d" % (idev.numel(), n))
    elif n != faces_dev.shape[0]:
        raise ValueError("without an index there is one parameter set per face: %d faces, %d params" % (faces_dev.shape[0], n))
    x = torch.empty((n, 3, t, t), dtype=dtype, device=dev)
    u8 = torch.empty((n, t, t, 3), dtype=torch.uint8, device=dev) if want_u8 else None
    with torch.cuda.device(dev):
        _lib.check(_lib.load().vnf_augment_faces(
            ctypes.c_void_p(faces_dev.data_ptr()), int(faces_dev.shape[0]), int(faces_dev.shape[1]),
            ctypes.c_void_p(idev.data_ptr()) if idev is not None else None,
            ctypes.c_void_p(pdev.data_ptr()) if n else None, n, int(t), ctypes.c_void_p(x.data_ptr()),
            _lib.torch_dtype_code(dtype), ctypes.c_void_p(u8.data_ptr()) if u8 is not None else None,
            _lib.current_stream_ptr()))
    return (x, u8) if want_u8 else x


class FacenetAug:
    """transforms_dict['facenet_aug'] for a batch: draws, then the kernel."""
    name = "facenet_aug"
    random = True

    def params(self, n, s, t):
        return draw_facenet_aug_params(n, s, t)[0]


class DefaultTransform:
    """transforms_dict['default'] (normalise only) for a batch: the same kernel with identity parameters."""
    name = "default"
    random = False

    def params(self, n, s, t):
        return identity_params(n, s, t)


def _rank1_aug():
    raise NotImplementedError(
        "transforms 'rank1_aug' is imgaug's pipeline (data_loader/__init__.py:10-25,45-49: hue / blur / sharpen / emboss "
        "on the host plus per-image prewhitening); imgaug is not a dependency of this build and none of it has a device "
        "kernel here.  Use 'facenet_aug' or 'default' (DESIGN.md 8)")


transforms_dict = {"default": DefaultTransform, "facenet_aug": FacenetAug, "rank1_aug": _rank1_aug}


def get_transform(name):
    if name not in transforms_dict:
        raise KeyError("unknown transforms %r (known: %s)" % (name, ", ".join(sorted(transforms_dict))))
    return transforms_dict[name]()
