"""Host-side mirror of the reference's MLP identity classifier, backed by libvnface.so.

  MLPModel            <-  /root/reference/models/mlp_model.py:4-15
  load_model_classify <-  /root/reference/demo_image.py:16-21   (checkpoint dict of
                          trainer/base_trainer.py:91-98: needs 'epoch' and 'state_dict')
  check_targets / logits_eval <- /root/reference/trainer/classification_trainer.py:42-80 (what _validate_epoch does
                          with a batch of model outputs: nll_loss, accuracy, argmax, exp)
"""
import ctypes
from collections import OrderedDict

import numpy as np
import torch

from . import _lib
from .weights import generate_state_dict


class MLPModel:
    """MLPModel(input_dim, num_classes): __call__((F,input_dim)) -> (F,num_classes) log-probs."""

    def __init__(self, input_dim, num_classes, max_batch=1024, seed=0):
        self.input_dim = int(input_dim)
        self.num_classes = int(num_classes)
        self.max_batch = int(max_batch)
        self.training = False
        self.device = torch.device("cpu")
        self._handle = None
        self._handle_dev = None
        # the reference starts from torch's random init; a deterministic generator stands in
        self._sd = generate_state_dict("mlp", seed, input_dim=self.input_dim, num_classes=self.num_classes)

    def eval(self):
        self.training = False
        return self

    def to(self, device):
        self.device = torch.device(device)
        return self

    def state_dict(self):
        return OrderedDict((k, torch.from_numpy(np.ascontiguousarray(v)) if isinstance(v, np.ndarray) else v)
                           for k, v in self._sd.items())

    def load_state_dict(self, state_dict, strict=True):
        want = {"dense_1.weight": (2048, self.input_dim), "dense_1.bias": (2048,),
                "dense_2.weight": (self.num_classes, 2048), "dense_2.bias": (self.num_classes,)}
        for k, shp in want.items():
            if k not in state_dict:
                raise RuntimeError("Missing key(s) in state_dict: %s" % k)
            if tuple(state_dict[k].shape) != shp:
                raise RuntimeError("size mismatch for %s: %s vs %s" % (k, tuple(state_dict[k].shape), shp))
        if strict and set(state_dict) - set(want):
            raise RuntimeError("Unexpected key(s) in state_dict: %s" % sorted(set(state_dict) - set(want)))
        self._sd = OrderedDict((k, state_dict[k]) for k in want)
        self._drop()
        return self

    def _drop(self):
        if self._handle is not None:
            _lib.load().vnf_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self._drop()
        except Exception:
            pass

    def _ensure(self):
        if self.device.type != "cuda":
            raise RuntimeError("MLPModel runs on MI355X only: move it to a cuda device (there is no CPU path)")
        dev = self.device.index if self.device.index is not None else torch.cuda.current_device()
        if self._handle is not None and self._handle_dev == dev:
            return self._handle
        self._drop()
        lib = _lib.load()
        with torch.cuda.device(dev):
            _lib.check(lib.vnf_init(dev))
            descs, n, keep = _lib.make_descs(self._sd)
            h = ctypes.c_void_p()
            _lib.check(lib.vnf_mlp_create(descs, n, self.input_dim, self.num_classes, self.max_batch, ctypes.byref(h)))
            del keep
        self._handle, self._handle_dev = h, dev
        return h

    def classify(self, emb, want_logp=True):
        """(F,input_dim) fp32 cuda -> (logp (F,C) or None, argmax (F,) int32, prob (F,) fp32)."""
        h = self._ensure()
        if emb.device.type != "cuda":
            raise RuntimeError("embeddings must live on the classifier's cuda device")
        emb = emb.float().contiguous()
        f = emb.shape[0]
        logp = torch.empty((f, self.num_classes), dtype=torch.float32, device=emb.device) if want_logp else None
        amax = torch.empty((f,), dtype=torch.int32, device=emb.device)
        prob = torch.empty((f,), dtype=torch.float32, device=emb.device)
        lib = _lib.load()
        with torch.cuda.device(emb.device):
            for f0 in range(0, f, self.max_batch):
                nn = min(self.max_batch, f - f0)
                _lib.check(lib.vnf_classify(h, ctypes.c_void_p(emb[f0:].data_ptr()), nn,
                                            ctypes.c_void_p(logp[f0:].data_ptr()) if want_logp else None,
                                            ctypes.c_void_p(amax[f0:].data_ptr()), ctypes.c_void_p(prob[f0:].data_ptr()),
                                            _lib.current_stream_ptr()))
        return logp, amax, prob

    def forward(self, emb):
        return self.classify(emb, want_logp=True)[0]

    __call__ = forward


def load_model_classify(checkpoint_path, model):
    """demo_image.py:16-21.  The checkpoint is a plain dict (epoch, state_dict, optimizer state,
    config); weights_only loading refuses anything that would execute code."""
    cp = torch.load(checkpoint_path, map_location="cpu", weights_only=True)
    print("Loading checkpoint: {} ... after training for {} epochs.".format(checkpoint_path, cp['epoch']))
    model.load_state_dict(cp['state_dict'])
    return model


def check_targets(target, num_classes):
    """Class labels of a batch as an int64 CPU tensor, checked on the host before they are uploaded: the device kernels
    cannot refuse a label, torch's nll_loss raises on one outside [0, C) (trainer/classification_trainer.py:53)."""
    t = torch.as_tensor(target).detach().cpu()
    if t.numel() == 0:      # an empty list comes as float32
        return torch.zeros((0,), dtype=torch.int64)
    if t.dtype.is_floating_point or t.dtype == torch.bool:
        raise TypeError("class labels must be integers, got %s" % t.dtype)
    t = t.to(torch.int64).reshape(-1)
    if t.numel() and (int(t.min()) < 0 or int(t.max()) >= int(num_classes)):
        bad = int(t.max()) if int(t.max()) >= int(num_classes) else int(t.min())
        raise IndexError("Target %d is out of bounds." % bad)
    return t


_EVAL_OUTPUTS = ("logp", "amax", "prob", "nll", "hit", "sums")


def logits_eval(logits, target=None, want=("amax", "prob", "nll", "hit", "sums")):
    """vnf_logits_eval on a cuda (n,C) fp32 matrix of logits (or log-probabilities: log_softmax leaves them as they are,
    up to rounding) whose rows may be strided.  target: integer labels, checked on the host by check_targets before
    they reach the device.  Returns {name: cuda tensor} for the names in `want`:
    logp (n,C), amax (n) int32, prob (n), nll (n), hit (n) int32, sums (2) = {sum nll, sum hit}."""
    if logits.device.type != "cuda":
        raise RuntimeError("logits_eval runs on MI355X only: the logits must live on a cuda device (there is no CPU path)")
    unknown = set(want) - set(_EVAL_OUTPUTS)
    if unknown:
        raise ValueError("unknown outputs: %s" % sorted(unknown))
    if logits.dim() != 2 or logits.dtype != torch.float32:
        raise ValueError("expected (n,C) fp32 logits, got %s %s" % (tuple(logits.shape), logits.dtype))
    n, c = int(logits.shape[0]), int(logits.shape[1])
    if c < 1:
        raise ValueError("logits need at least one column")
    if logits.stride(1) != 1 or (n > 1 and logits.stride(0) < c):
        logits = logits.contiguous()
    ld = int(logits.stride(0)) if n > 1 else c
    needs_t = [k for k in ("nll", "hit", "sums") if k in want]
    if needs_t and target is None:
        raise ValueError("%s need a target" % ", ".join(needs_t))
    t = None
    if target is not None:
        t = check_targets(target, c).to(logits.device)
        if t.numel() != n:
            raise ValueError("%d targets for %d rows" % (t.numel(), n))
    dev = logits.device
    out = {}
    if "logp" in want:
        out["logp"] = torch.empty((n, c), dtype=torch.float32, device=dev)
    if "amax" in want:
        out["amax"] = torch.empty((n,), dtype=torch.int32, device=dev)
    for k in ("prob", "nll"):
        if k in want:
            out[k] = torch.empty((n,), dtype=torch.float32, device=dev)
    if "hit" in want:
        out["hit"] = torch.empty((n,), dtype=torch.int32, device=dev)
    if "sums" in want:
        out["sums"] = torch.zeros((2,), dtype=torch.float32, device=dev)

    def ptr(k):
        return ctypes.c_void_p(out[k].data_ptr()) if k in out else None
    with torch.cuda.device(dev):
        _lib.check(_lib.load().vnf_logits_eval(
            ctypes.c_void_p(logits.data_ptr()), n, c, ld, ctypes.c_void_p(t.data_ptr()) if t is not None else None,
            ptr("logp"), ptr("amax"), ptr("prob"), ptr("nll"), ptr("hit"), ptr("sums"), _lib.current_stream_ptr()))
    return out
