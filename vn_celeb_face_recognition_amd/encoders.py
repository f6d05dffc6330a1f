"""Host-side mirrors of the reference's encoder plugins, backed by libvnface.so.

  InceptionResnetV1  <-  /root/reference/models/inception_resnet_v1.py:184-303
  iresnet100         <-  /root/reference/models/iresnet_encoder.py:64-196
  resnet101          <-  /root/reference/models/resnet_encoder.py:98-254 (use_se=True: the SE-IR ResNet-101)

Same constructor kwargs, `.to()`, `.eval()`, `load_state_dict()`, and `__call__((N,3,S,S)) ->
(N,512)` on the same device (demo_image.py:30-34, find_embedding.py:58).  All arithmetic runs in
hand-written HIP kernels; torch only owns the input/output device memory and the stream.
With their own `logits` head (InceptionResnetV1(classify=True, ...), iresnet100(n_classes=...):
inception_resnet_v1.py:260-265,298-300, iresnet_encoder.py:100-103,155-157) the models return (N,C)
log-probabilities, `.logprobs(x)` adds argmax and probability, `.embed(x)` still gives the embeddings.
`.features(x)` gives the (N,512) rows the head reads, head or no head; with freeze_weights that head is what
trainer.TrainableHead trains (the backbone stays as it is: nothing here runs backward through an encoder).
There is no CPU path: calling a model that is not on a CUDA(ROCm) device raises.
"""
import ctypes
import os
from collections import OrderedDict

import numpy as np
import torch

from . import _lib
from .weights import generate_state_dict

_DTYPES = {"bf16": _lib.VNF_BF16, "f16": _lib.VNF_F16, "fp16": _lib.VNF_F16, "f16x2": _lib.VNF_F16X2, "f32": _lib.VNF_F32,
           "fp32": _lib.VNF_F32, torch.bfloat16: _lib.VNF_BF16, torch.float16: _lib.VNF_F16,
           torch.float32: _lib.VNF_F32}


def _torch_home():
    # models/inception_resnet_v1.py:334-341
    return os.path.expanduser(os.getenv("TORCH_HOME", os.path.join(os.getenv("XDG_CACHE_HOME", "~/.cache"), "torch")))


def _load_checkpoint_file(path):
    """Flat state_dict or {'state_dict': ...}, loaded without executing pickled code."""
    cp = torch.load(path, map_location="cpu", weights_only=True)
    if isinstance(cp, dict) and "state_dict" in cp and isinstance(cp["state_dict"], dict):
        cp = cp["state_dict"]
    return cp


class _Encoder:
    """nn.Module-shaped wrapper around a vnf encoder handle."""
    _arch = None
    arch_name = None    # type(model).__name__ of the reference's module: what a checkpoint's "arch" holds
    input_size = None
    freeze_weights = False   # only `logits` may train (trainer.TrainableHead)
    _out_dim = 512      # columns of the tensor vnf_encoder_profile writes

    def __init__(self, device=None, compute_dtype="f16x2", max_batch=256):
        self._sd = None
        self._num_classes = None    # width of the model's own `logits` head; None: an embedding model
        self._handle = None
        self._handle_key = None
        self.compute_dtype = compute_dtype
        self.max_batch = int(max_batch)
        self.training = False
        self.device = torch.device("cpu")
        if device is not None:
            self.to(device)

    @property
    def head_classes(self):
        """Width of the model's own `logits` head, or None for an embedding model."""
        return self._num_classes

    # ---- nn.Module surface used by the reference's callers
    def eval(self):
        self.training = False
        return self

    def train(self, mode=True):
        if mode:
            raise NotImplementedError("inference-only encoder (training is out of scope, SURVEY.md 8)")
        return self

    def to(self, device):
        self.device = torch.device(device)
        return self

    def cuda(self, device=None):
        return self.to("cuda" if device is None else device)

    def parameters(self):
        return iter(())

    def state_dict(self):
        return OrderedDict((k, torch.from_numpy(np.ascontiguousarray(v)) if isinstance(v, np.ndarray) else v)
                           for k, v in self._sd.items())

    def load_state_dict(self, state_dict, strict=True):
        expected = [k for k in self._expected_keys()]
        missing = [k for k in expected if k not in state_dict]
        if strict and missing:
            raise RuntimeError("Missing key(s) in state_dict: %s" % ", ".join(missing[:8]))
        if self._num_classes is not None and "logits.weight" in state_dict:
            shp = tuple(state_dict["logits.weight"].shape)
            if shp != (self._num_classes, 512):
                raise RuntimeError("size mismatch for logits.weight: %s vs %s" % (shp, (self._num_classes, 512)))
        sd = OrderedDict(self._sd) if (self._sd is not None and not strict) else OrderedDict()
        for k, v in state_dict.items():
            sd[k] = v
        self._sd = sd
        self._drop_handle()
        return self

    def __del__(self):
        try:
            self._drop_handle()
        except Exception:
            pass

    def _drop_handle(self):
        if self._handle is not None:
            _lib.load().vnf_destroy(self._handle)
            self._handle = None

    def _expected_keys(self):
        return [n for n, _, kind in self._spec() if kind != "nbt"]

    def _ensure_handle(self):
        if self.device.type != "cuda":
            raise RuntimeError("%s runs on MI355X only: move it to a cuda device (there is no CPU path)"
                               % type(self).__name__)
        key = (self.device.index or 0, self.compute_dtype, self.max_batch, self._num_classes)
        if self._handle is not None and self._handle_key == key:
            return self._handle
        self._drop_handle()
        lib = _lib.load()
        dev = self.device.index if self.device.index is not None else torch.cuda.current_device()
        with torch.cuda.device(dev):
            _lib.check(lib.vnf_init(dev))
            descs, n, keep = _lib.make_descs(self._sd)
            h = ctypes.c_void_p()
            _lib.check(self._create(lib, descs, n, h))
            del keep
        self._handle, self._handle_key = h, key
        return h

    def _create(self, lib, descs, n, h):
        if self._num_classes is not None:
            return lib.vnf_encoder_create_classifier(self._arch, descs, n, _DTYPES[self.compute_dtype], self.max_batch,
                                                     self._num_classes, ctypes.byref(h))
        return lib.vnf_encoder_create(self._arch, descs, n, _DTYPES[self.compute_dtype], self.max_batch, ctypes.byref(h))

    def __call__(self, x):
        return self.forward(x)

    def _checked_input(self, x):
        if x.dim() != 4 or x.shape[1] != 3 or x.shape[2] != self.input_size or x.shape[3] != self.input_size:
            raise ValueError("expected (N,3,%d,%d) input, got %s" % (self.input_size, self.input_size, tuple(x.shape)))
        if x.device.type != "cuda":
            raise RuntimeError("input tensor must live on the encoder's cuda device")
        return x.contiguous()

    def forward(self, x):
        """(N,3,S,S) -> (N,512) embeddings; a model with its own head (classify=True / n_classes): (N,C) log-probabilities."""
        if self._num_classes is not None:
            return self.logprobs(x)[0]
        return self.embed(x)

    def logprobs(self, x):
        """Model with a `logits` head: (N,3,S,S) cuda -> (logp (N,C) fp32, argmax (N,) int32, prob (N,) fp32 = exp(logp[argmax])),
        all cuda (vnf_encoder_logprobs)."""
        if self._num_classes is None:
            raise RuntimeError("%s was built without a classification head (classify=True / n_classes)" % type(self).__name__)
        h = self._ensure_handle()
        x = self._checked_input(x)
        n = x.shape[0]
        logp = torch.empty((n, self._num_classes), dtype=torch.float32, device=x.device)
        amax = torch.empty((n,), dtype=torch.int32, device=x.device)
        prob = torch.empty((n,), dtype=torch.float32, device=x.device)
        lib = _lib.load()
        with torch.cuda.device(x.device):
            for n0 in range(0, n, self.max_batch):
                nn = min(self.max_batch, n - n0)
                _lib.check(lib.vnf_encoder_logprobs(h, ctypes.c_void_p(x[n0:n0 + nn].data_ptr()), nn, _lib.torch_dtype_code(x.dtype),
                                                    ctypes.c_void_p(logp[n0:].data_ptr()), ctypes.c_void_p(amax[n0:].data_ptr()),
                                                    ctypes.c_void_p(prob[n0:].data_ptr()), _lib.current_stream_ptr()))
        return logp, amax, prob

    def embed(self, x):
        """(N,3,S,S) cuda -> (N,512) fp32 embeddings (vnf_embed), head or no head."""
        h = self._ensure_handle()
        x = self._checked_input(x)
        n = x.shape[0]
        out = torch.empty((n, 512), dtype=torch.float32, device=x.device)
        lib = _lib.load()
        with torch.cuda.device(x.device):
            for n0 in range(0, n, self.max_batch):
                nn = min(self.max_batch, n - n0)
                xs = x[n0:n0 + nn]
                _lib.check(lib.vnf_embed(h, ctypes.c_void_p(xs.data_ptr()), nn, _lib.torch_dtype_code(x.dtype),
                                         ctypes.c_void_p(out[n0:].data_ptr()), _lib.current_stream_ptr()))
        return out

    def features(self, x):
        """(N,3,S,S) cuda -> (N,512) fp32 cuda: the rows the `logits` layer reads (vnf_encoder_features) -- last_bn's
        output before the normalisation (InceptionResnetV1), `features` (IResNet-100); head or no head."""
        h = self._ensure_handle()
        x = self._checked_input(x)
        n = x.shape[0]
        out = torch.empty((n, 512), dtype=torch.float32, device=x.device)
        lib = _lib.load()
        with torch.cuda.device(x.device):
            for n0 in range(0, n, self.max_batch):
                nn = min(self.max_batch, n - n0)
                _lib.check(lib.vnf_encoder_features(h, ctypes.c_void_p(x[n0:n0 + nn].data_ptr()), nn, _lib.torch_dtype_code(x.dtype),
                                                    ctypes.c_void_p(out[n0:].data_ptr()), _lib.current_stream_ptr()))
        return out

    def set_streams(self, max_streams):
        """Cap the encoder's internal batch split (vnf_encoder_set_streams): 1 when other work shares the GPU."""
        _lib.check(_lib.load().vnf_encoder_set_streams(self._ensure_handle(), int(max_streams)))

    def set_contexts(self, n):
        """Rotate consecutive calls over n private activation-buffer sets (vnf_encoder_set_contexts), so calls issued
        on different streams overlap on the GPU."""
        _lib.check(_lib.load().vnf_encoder_set_contexts(self._ensure_handle(), int(n)))

    def embed_stream(self, batches, lanes=3):
        """Throughput mode over an iterable of independent (N,3,S,S) batches (host or cuda tensors): batch i runs on
        stream i % lanes over the encoder's activation contexts, so up to `lanes` batches are in flight on the GPU;
        yields (index, embeddings (N,512) cuda, ready_event) in order -- wait on / synchronise the event before
        reading.  What find_embedding.py's loop over a directory becomes (find_embedding.py:44-59)."""
        dev = self.device if isinstance(self.device, torch.device) else torch.device(self.device)
        lanes = max(1, min(4, int(lanes)))
        if lanes > 1:
            self.set_streams(1)
            self.set_contexts(lanes)
        from .streams import side_streams
        streams = side_streams(dev, lanes)      # process-wide stream objects (streams.py: hardware-queue binding)
        start = torch.cuda.current_stream(dev).record_event()
        for s_ in streams:
            s_.wait_event(start)
        inflight = []
        for i, x in enumerate(batches):
            s_ = streams[i % lanes]
            with torch.cuda.stream(s_):
                x = x.to(dev, non_blocking=True)
                emb = self.embed(x)
                ev = s_.record_event()
            x.record_stream(s_)
            inflight.append((i, emb, ev))
            if len(inflight) >= lanes:
                yield inflight.pop(0)
        for item in inflight:
            yield item

    # ---- extras used by tests / bench
    def tap(self, name, n):
        """Copy an internal activation of the last forward (first n images) to a (n,C,H,W) fp32 array."""
        h = self._ensure_handle()
        lib = _lib.load()
        shape = (ctypes.c_int64 * 4)()
        lib.vnf_encoder_tap(h, name.encode(), n, None, 0, shape)  # query shape (returns capacity error)
        total = int(shape[0] * shape[1] * shape[2] * shape[3])
        if total <= 0:
            _lib.check(lib.vnf_encoder_tap(h, name.encode(), n, None, 0, shape))
        buf = np.empty(total, dtype=np.float32)
        torch.cuda.synchronize()
        _lib.check(lib.vnf_encoder_tap(h, name.encode(), n, buf.ctypes.data, total, shape))
        return buf.reshape(tuple(int(s) for s in shape))

    def profile(self, x):
        """Per-launch device-time table of one forward (text)."""
        h = self._ensure_handle()
        x = x.contiguous()
        out = torch.empty((x.shape[0], self._out_dim), dtype=torch.float32, device=x.device)
        buf = ctypes.create_string_buffer(1 << 16)
        with torch.cuda.device(x.device):
            _lib.check(_lib.load().vnf_encoder_profile(h, ctypes.c_void_p(x.data_ptr()), x.shape[0],
                                                       _lib.torch_dtype_code(x.dtype), ctypes.c_void_p(out.data_ptr()),
                                                       _lib.current_stream_ptr(), buf, len(buf)))
        return buf.value.decode()

    def flops_per_image(self):
        h = self._ensure_handle()
        a, e = ctypes.c_double(), ctypes.c_double()
        _lib.check(_lib.load().vnf_encoder_flops(h, ctypes.byref(a), ctypes.byref(e)))
        return a.value, e.value


class InceptionResnetV1(_Encoder):
    """Drop-in for models.InceptionResnetV1 (inception_resnet_v1.py:202).

    compute_dtype (build extension; may also be given in the -eargs JSON): "f16x2" (default) is the parity path --
    split-f16 operands on the 16-bit MFMA, <= 1e-4 embedding L2 against the reference (measured ~1.5e-6), the same
    default in every CLI so embeddings the MLP is trained on and embeddings it classifies come from one arithmetic;
    "bf16" / "f16" trade accuracy (5e-3 / 6e-4) for 2.8x the throughput; "f32" is the exact fp32 fma chain.

    pretrained: None -> deterministic generator weights (seed 0; the reference would leave
    torch's random init); 'vggface2' / 'casia-webface' -> the file the reference caches under
    $TORCH_HOME/checkpoints (never downloaded here); or a path to a local state_dict file
    (build extension).

    classify=True: the model ends in its `logits` layer and returns log-probabilities.  With num_classes the head is a
    fresh generator-seeded (num_classes, 512) layer (the reference: torch's random init) until load_state_dict brings a
    trained one; without it the head is the pretrained file's own.  The head runs in exact fp32 in every compute_dtype.

    freeze_weights (build extension; the reference has no such flag and would fine-tune every layer): with classify, only
    `logits` may train -- the model train.py accepts for head training (trainer.TrainableHead).
    """
    _arch = _lib.VNF_ARCH_IRV1
    arch_name = "InceptionResnetV1"
    input_size = 160
    _FILES = {"vggface2": "20180402-114759-vggface2.pt", "casia-webface": "20180408-102900-casia-webface.pt"}

    def __init__(self, pretrained=None, classify=False, num_classes=None, dropout_prob=0.6, device=None,
                 compute_dtype="f16x2", max_batch=256, seed=0, freeze_weights=False):
        if pretrained is None and classify and num_classes is None:
            # inception_resnet_v1.py:214-215
            raise Exception('If "pretrained" is not specified and "classify" is True, "num_classes" must be specified')
        self.pretrained = pretrained
        self.classify = classify
        self.num_classes = num_classes
        self.freeze_weights = bool(freeze_weights and classify)
        super().__init__(device=None, compute_dtype=compute_dtype, max_batch=max_batch)
        if pretrained is None:
            self._sd = generate_state_dict("irv1", seed)
        else:
            path = pretrained
            if pretrained in self._FILES:
                path = os.path.join(_torch_home(), "checkpoints", self._FILES[pretrained])
            if not os.path.exists(path):
                raise FileNotFoundError(
                    "pretrained weights %r not found at %s (no network: place the file there or pass a local path)"
                    % (pretrained, path))
            self.load_state_dict(_load_checkpoint_file(path), strict=False)
        if classify:
            if num_classes is not None:
                # a fresh head (inception_resnet_v1.py:264-265 replaces the file's, whatever its width): the reference
                # leaves torch's random init, here the generator's draw; load_state_dict replaces it
                head = generate_state_dict("irv1", seed, num_classes=int(num_classes))
                self._sd["logits.weight"], self._sd["logits.bias"] = head["logits.weight"], head["logits.bias"]
                self._num_classes = int(num_classes)
            else:
                # the file's own head (:260-262: 8631 classes for vggface2, 10575 for casia-webface)
                if "logits.weight" not in self._sd or "logits.bias" not in self._sd:
                    raise RuntimeError("classify=True without num_classes needs the `logits` layer of the pretrained file: %r "
                                       "has none" % (pretrained,))
                self._num_classes = int(self._sd["logits.weight"].shape[0])
        if device is not None:
            self.to(device)

    def _spec(self):
        from .weights import irv1_spec
        return irv1_spec(num_classes=self._num_classes)


class _IResNet100(_Encoder):
    _arch = _lib.VNF_ARCH_IR100
    arch_name = "IResNet"
    input_size = 112

    def _spec(self):
        from .weights import iresnet_spec
        return iresnet_spec(n_classes=self._num_classes)


def iresnet100(pretrained=False, progress=True, freeze_weights=False, checkpoint_path="", compute_dtype="f16x2",
               max_batch=256, seed=0, n_classes=None, **kwargs):
    """Drop-in for models.iresnet100 (iresnet_encoder.py:162-181,194-196); kwargs of
    cfg/embedding/iresnet100_enc.json.  pretrained=True needs checkpoint_path (a file holding
    {'state_dict': ...}); the URL branch of the reference cannot run offline.  n_classes (iresnet_encoder.py:100-103):
    the model gets a `logits` layer (generator weights until a checkpoint brings its own) and returns log-probabilities.
    freeze_weights with n_classes (iresnet_encoder.py:174-179): only `logits` may train, which trainer.TrainableHead does."""
    if kwargs:
        raise TypeError("unexpected keyword arguments: %s" % sorted(kwargs))
    m = _IResNet100(compute_dtype=compute_dtype, max_batch=max_batch)
    if n_classes is not None:
        m._num_classes = int(n_classes)
    m._sd = generate_state_dict("iresnet100", seed, n_classes=m._num_classes)
    if pretrained:
        if not checkpoint_path:
            raise FileNotFoundError("iresnet100(pretrained=True) needs checkpoint_path: no network access")
        print("Loaded encoder state dict from checkpoint path {}".format(checkpoint_path))
        m.load_state_dict(_load_checkpoint_file(checkpoint_path), strict=False)
    if freeze_weights and n_classes is not None:
        print("Freezing weights !")    # iresnet_encoder.py:174-179: only `logits` trains (trainer.TrainableHead)
        m.freeze_weights = True
    return m


class _SEIResNet101(_Encoder):
    _arch = _lib.VNF_ARCH_SEIR101
    input_size = 112

    def _spec(self):
        from .weights import seir_spec
        return seir_spec()


def resnet101(use_se=False, pretrained=False, img_size=112, cp_path=None, compute_dtype="f16x2", max_batch=256, seed=0):
    """Drop-in for models.resnet101 (resnet_encoder.py:246-254); kwargs of cfg/embedding/resnet101_se.json.  Only the
    squeeze-and-excitation variant at 112 x 112 is built: the one every config of the reference names
    (cfg/train_cfg_aug_emb_classify.json:80-88) and the only one with a published checkpoint.  (N,3,112,112) -> (N,512)
    unit rows.  Without cp_path the weights are the deterministic generator's (the reference: torch's random init);
    cp_path is a plain state_dict file, loaded strictly as the reference loads it -- a missing key raises.
    compute_dtype / max_batch / seed are build extensions, as for the other encoders."""
    if not use_se:
        raise NotImplementedError("resnet101(use_se=False) is not built: only the SE-IR ResNet-101 (use_se=True), the variant "
                                  "the reference's configs name and the only one with a published checkpoint")
    if pretrained:
        raise NotImplementedError("resnet101(pretrained=True) downloads torchvision's ImageNet ResNet-101, whose keys are not "
                                  "this network's (resnet_encoder.py:248-249) and which cannot be fetched here: pass cp_path")
    if img_size != 112:
        raise NotImplementedError("resnet101(img_size=%r): only the 112 x 112 network (fc over 512 x 7 x 7) is built" % (img_size,))
    m = _SEIResNet101(compute_dtype=compute_dtype, max_batch=max_batch)
    m._sd = generate_state_dict("seir101", seed)
    if cp_path:
        if not os.path.exists(cp_path):
            raise FileNotFoundError("resnet101: checkpoint %s not found" % cp_path)
        m.load_state_dict(torch.load(cp_path, map_location="cpu", weights_only=True), strict=True)
    return m
