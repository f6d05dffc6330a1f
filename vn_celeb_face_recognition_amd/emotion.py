"""Host-side mirror of the reference's emotion network plugin, backed by libvnface.so.

  resnet_2branch_50     <-  models/resnet_2_branch.py:12-89 (ResNet2Branch: ResNet-50 with a class head `fc` and a
                            projection head `proj`)
  pillow_bilinear_resize <- the Resize(224) of data_loader/__init__.py:74-81 on a square face, restated in NumPy:
                            the specification of the vnf_emotion_prep kernel

`model(x)` on a (N,3,224,224) cuda tensor returns `(x_cls, x_proj)` like the reference's forward; `model.recognize`
is the resident path (u8 faces -> transform -> network -> top-k in one enqueue).  All arithmetic runs in HIP kernels;
there is no CPU path.
"""
import ctypes
import math
from collections import OrderedDict

import numpy as np
import torch

from . import _lib
from .encoders import _DTYPES, _Encoder
from .weights import generate_state_dict, rn50_2b_spec

EMOTION_MEAN = (0.485, 0.456, 0.406)
EMOTION_STD = (0.229, 0.224, 0.225)
EMOTION_SIZE = 224
_PRECISION_BITS = 22


def _resample_coeffs(in_size, out_size):
    """Pillow's bilinear resampling windows for in_size -> out_size: (first source index (out,), window length (out,),
    22-bit fixed-point weights (out, ksize) int64, zero beyond the window).  Triangle filter with support
    max(in/out, 1); weights normalised in double, then int(k * 2^22 + 0.5)."""
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = 1.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    lo = np.zeros(out_size, np.int64)
    cnt = np.zeros(out_size, np.int64)
    kk = np.zeros((out_size, ksize), np.int64)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        ss = 1.0 / filterscale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = []
        for x in range(xmax):
            a = abs((x + xmin - center + 0.5) * ss)
            w.append(1.0 - a if a < 1.0 else 0.0)
        ww = sum(w)
        for x in range(xmax):
            k = w[x] / ww if ww != 0.0 else w[x]
            kk[xx, x] = int(-0.5 + k * (1 << _PRECISION_BITS)) if k < 0 else int(0.5 + k * (1 << _PRECISION_BITS))
        lo[xx], cnt[xx] = xmin, xmax
    return lo, cnt, kk


def _resample_axis1(a, out_size):
    """One 8-bit Pillow pass along axis 1 of a (R, in, C) u8 array: acc = 2^21 + sum(pixel * k), clip8(acc >> 22)."""
    in_size = a.shape[1]
    lo, cnt, kk = _resample_coeffs(in_size, out_size)
    acc = np.full((a.shape[0], out_size, a.shape[2]), 1 << (_PRECISION_BITS - 1), np.int64)
    src = a.astype(np.int64)
    for t in range(kk.shape[1]):
        idx = np.minimum(lo + t, in_size - 1)          # taps beyond a window carry weight 0
        acc += src[:, idx, :] * kk[:, t][None, :, None]
    return np.clip(acc >> _PRECISION_BITS, 0, 255).astype(np.uint8)


def pillow_bilinear_resize(face_u8, size=EMOTION_SIZE):
    """PIL.Image.fromarray(face).resize((size, size), Image.BILINEAR) byte for byte, for an (H,W,3) u8 array: two
    separable passes, horizontal first, the intermediate clipped to u8."""
    a = np.ascontiguousarray(face_u8, dtype=np.uint8)
    if a.ndim != 3:
        raise ValueError("expected an (H,W,C) uint8 image, got shape %s" % (a.shape,))
    h = _resample_axis1(a, size)                                             # (H, size, C)
    return np.ascontiguousarray(_resample_axis1(h.transpose(1, 0, 2), size).transpose(1, 0, 2))


def _strip_module(state_dict):
    """The reference saves the emotion network from nn.DataParallel (resnet_2_branch.py:85-87): drop 'module.'."""
    return OrderedDict((k[7:] if k.startswith("module.") else k, v) for k, v in state_dict.items())


class ResNet2Branch(_Encoder):
    """nn.Module-shaped wrapper around a vnf emotion handle (ResNet-50, heads fc and proj)."""
    _arch = _lib.VNF_ARCH_RN50_2B
    input_size = EMOTION_SIZE

    def __init__(self, num_classes=1000, num_projections=300, compute_dtype="f16x2", max_batch=256, seed=0):
        if compute_dtype not in _DTYPES:
            raise ValueError("unknown compute_dtype %r" % (compute_dtype,))
        self.num_classes = int(num_classes)
        self.num_projections = int(num_projections)
        self._out_dim = self.num_classes
        super().__init__(device=None, compute_dtype=compute_dtype, max_batch=max_batch)
        self._sd = generate_state_dict("rn50_2b", seed, num_classes=self.num_classes, num_projections=self.num_projections)

    def _spec(self):
        return rn50_2b_spec(self.num_classes, self.num_projections)

    def load_state_dict(self, state_dict, strict=True):
        sd = _strip_module(state_dict)
        for name, shape, kind in self._spec():
            if kind != "nbt" and name in sd and tuple(sd[name].shape) != tuple(shape):
                raise RuntimeError("size mismatch for %s: checkpoint %s, model %s" % (name, tuple(sd[name].shape), tuple(shape)))
        return super().load_state_dict(sd, strict=strict)

    def _create(self, lib, descs, n, h):
        return lib.vnf_emotion_create(descs, n, self.num_classes, self.num_projections, _DTYPES[self.compute_dtype],
                                      self.max_batch, ctypes.byref(h))

    def set_contexts(self, n):
        if int(n) != 1:
            raise NotImplementedError("the emotion network keeps one activation-buffer set")

    def embed_stream(self, batches, lanes=3):
        raise NotImplementedError("embed_stream is the embedding encoders' throughput mode ((N,512) embeddings over several "
                                  "activation contexts); the emotion network keeps one buffer set: call the model or "
                                  "recognize() batch by batch on one stream")

    def forward(self, x):
        """(N,3,224,224) cuda, normalised -> (x_cls (N,num_classes), x_proj (N,num_projections)), cuda fp32."""
        h = self._ensure_handle()
        if x.dim() != 4 or tuple(x.shape[1:]) != (3, self.input_size, self.input_size):
            raise ValueError("expected (N,3,%d,%d) input, got %s" % (self.input_size, self.input_size, tuple(x.shape)))
        if x.device.type != "cuda":
            raise RuntimeError("input tensor must live on the model's cuda device")
        x = x.contiguous()
        n = x.shape[0]
        cls = torch.empty((n, self.num_classes), dtype=torch.float32, device=x.device)
        proj = torch.empty((n, self.num_projections), dtype=torch.float32, device=x.device)
        lib = _lib.load()
        with torch.cuda.device(x.device):
            for n0 in range(0, n, self.max_batch):
                nn = min(self.max_batch, n - n0)
                _lib.check(lib.vnf_emotion_forward(h, ctypes.c_void_p(x[n0:n0 + nn].data_ptr()), nn,
                                                   _lib.torch_dtype_code(x.dtype), ctypes.c_void_p(cls[n0:].data_ptr()),
                                                   ctypes.c_void_p(proj[n0:].data_ptr()), _lib.current_stream_ptr()))
        return cls, proj

    def recognize(self, faces_u8, topk=6, want_logits=False):
        """Resident path of recognize_emotion: faces_u8 (N,S,S,3) u8 cuda, S <= 224 -> (idx (N,k) int32, prob (N,k)
        fp32[, logits (N,num_classes)]) on the device; transform, network and top-k are enqueued together."""
        h = self._ensure_handle()
        if faces_u8.dim() != 4 or faces_u8.shape[3] != 3 or faces_u8.shape[1] != faces_u8.shape[2] or faces_u8.dtype != torch.uint8:
            raise ValueError("expected (N,S,S,3) uint8 faces, got %s %s" % (tuple(faces_u8.shape), faces_u8.dtype))
        if faces_u8.device.type != "cuda":
            raise RuntimeError("faces must live on the model's cuda device")
        faces_u8 = faces_u8.contiguous()
        n, s, k = faces_u8.shape[0], faces_u8.shape[1], int(topk)
        idx = torch.empty((n, k), dtype=torch.int32, device=faces_u8.device)
        prob = torch.empty((n, k), dtype=torch.float32, device=faces_u8.device)
        cls = torch.empty((n, self.num_classes), dtype=torch.float32, device=faces_u8.device) if want_logits else None
        lib = _lib.load()
        with torch.cuda.device(faces_u8.device):
            for n0 in range(0, max(n, 1), self.max_batch):
                nn = min(self.max_batch, n - n0)
                _lib.check(lib.vnf_emotion_recognize(
                    h, ctypes.c_void_p(faces_u8[n0:n0 + nn].data_ptr()) if nn else None, nn, s, k,
                    ctypes.c_void_p(idx[n0:].data_ptr()) if nn else None, ctypes.c_void_p(prob[n0:].data_ptr()) if nn else None,
                    ctypes.c_void_p(cls[n0:].data_ptr()) if (want_logits and nn) else None, _lib.current_stream_ptr()))
        return (idx, prob, cls) if want_logits else (idx, prob)


def emotion_prep_device(faces_u8, dtype=torch.float32):
    """vnf_emotion_prep: (N,S,S,3) u8 cuda faces -> trans_emotion_inf as one (N,3,224,224) cuda tensor of `dtype`."""
    if faces_u8.dim() != 4 or faces_u8.shape[3] != 3 or faces_u8.shape[1] != faces_u8.shape[2] or faces_u8.dtype != torch.uint8:
        raise ValueError("expected (N,S,S,3) uint8 faces, got %s %s" % (tuple(faces_u8.shape), faces_u8.dtype))
    if faces_u8.device.type != "cuda":
        raise RuntimeError("the face transform kernel runs on MI355X only (pipeline.trans_emotion_inf is the host mirror)")
    faces_u8 = faces_u8.contiguous()
    n, s = faces_u8.shape[0], faces_u8.shape[1]
    out = torch.empty((n, 3, EMOTION_SIZE, EMOTION_SIZE), dtype=dtype, device=faces_u8.device)
    with torch.cuda.device(faces_u8.device):
        _lib.check(_lib.load().vnf_emotion_prep(ctypes.c_void_p(faces_u8.data_ptr()) if n else None, n, s,
                                                ctypes.c_void_p(out.data_ptr()) if n else None, _lib.torch_dtype_code(dtype),
                                                _lib.current_stream_ptr()))
    return out


def softmax_topk_device(logits, topk):
    """vnf_softmax_topk: (N,C) fp32 cuda logits -> (idx (N,k) int32, prob (N,k) fp32), descending, ties lower index first."""
    if logits.dim() != 2 or logits.device.type != "cuda":
        raise ValueError("expected (N,C) cuda logits")
    logits = logits.float().contiguous()
    n, c = logits.shape
    k = int(topk)
    idx = torch.empty((n, k), dtype=torch.int32, device=logits.device)
    prob = torch.empty((n, k), dtype=torch.float32, device=logits.device)
    with torch.cuda.device(logits.device):
        _lib.check(_lib.load().vnf_softmax_topk(ctypes.c_void_p(logits.data_ptr()) if n else None, n, c, k,
                                                ctypes.c_void_p(idx.data_ptr()) if n else None,
                                                ctypes.c_void_p(prob.data_ptr()) if n else None, _lib.current_stream_ptr()))
    return idx, prob


def resnet_2branch_50(pretrained=False, checkpoint_path=None, num_classes=1000, num_projections=300, compute_dtype="f16x2",
                      max_batch=256, seed=0, **kwargs):
    """Drop-in for models.resnet_2branch_50 (resnet_2_branch.py:73-89); kwargs of cfg/emotion/resnet50_2_branch.json.
    Without a checkpoint the weights are the deterministic generator's (the reference would keep torch's random init).
    checkpoint_path: a file holding {'state_dict': ...} whose keys carry DataParallel's 'module.' prefix (85-87), loaded
    without executing pickled code.  pretrained=True would download the ImageNet ResNet-50 in the reference."""
    if kwargs:
        raise TypeError("unexpected keyword arguments: %s" % sorted(kwargs))
    if pretrained:
        raise FileNotFoundError("resnet_2branch_50(pretrained=True) downloads ImageNet weights in the reference: no network "
                                "access, pass checkpoint_path instead")
    m = ResNet2Branch(num_classes=num_classes, num_projections=num_projections, compute_dtype=compute_dtype,
                      max_batch=max_batch, seed=seed)
    if checkpoint_path is not None:
        print('Loaded emotion model from checkpoint path {}'.format(checkpoint_path))
        cp = torch.load(checkpoint_path, map_location="cpu", weights_only=True)
        if not (isinstance(cp, dict) and isinstance(cp.get("state_dict"), dict)):
            raise RuntimeError("emotion checkpoint %r holds no 'state_dict'" % (checkpoint_path,))
        m.load_state_dict(cp["state_dict"], strict=True)
    return m
