"""MLP training on precomputed embeddings: host-side mirror of the reference's training stack, with
the optimisation step itself in libvnface.so (csrc/mlp_train.hip):

  VNCelebEmbDataset       <- /root/reference/data_loader/vn_celeb_dataset.py:12-47, vn_celeb_emb_dataset.py:6-23
  TrainableMLP            <- /root/reference/models/mlp_model.py:4-15 (+ torch.optim.Adam, train.py:60-62)
  ReduceLROnPlateau       <- torch.optim.lr_scheduler.ReduceLROnPlateau as train.py:64-66 configures it
  MetricTracker           <- /root/reference/utils/utils.py:13-37
  ClassificationTrainer   <- /root/reference/trainer/base_trainer.py:11-190, classification_trainer.py:5-98
  VNCelebDataset          <- /root/reference/data_loader/vn_celeb_dataset.py:12-47
  AugClassificationTrainer <- /root/reference/trainer/online_aug_trainer.py:6-97 (images -> augmentation -> frozen
                             encoder -> MLP step, all on the device: augment.py, csrc/augment.hip)

  TrainableHead           <- models/iresnet_encoder.py:174-179 (freeze_weights: `logits` alone trains)
                             under trainer/classification_trainer.py:9-40 on a VNCelebDataset
                             (cfg/train_cfg_img_classify.json): images -> augmentation -> frozen encoder's features ->
                             fused grad + Adam step of the head (csrc/head_train.hip)

  EvalModel, write_result_csv, ClassificationTrainer.eval
                          <- /root/reference/trainer/base_trainer.py:177-200, classification_trainer.py:42-80 (evaluation of
                             a trained model: MLPModel or an encoder with its own head; csrc/head_eval.hip)

Same config keys (cfg/train_cfg_emb_classify.json), same checkpoint dict (base_trainer.py:83-105: arch, epoch,
state_dict, optimizer in torch.optim.Adam's state_dict layout, monitor_best, config), same log_loss.txt.  torch is
plumbing: the DataLoader / sampler (batch order), the initial weights (nn.Linear's init) and the dropout draws come from
torch's CPU generator in the reference's order, so a run seeded like train.py:16-20 follows the reference's loss curve."""
import csv
import ctypes
import json
import logging
import os
from collections import OrderedDict
from datetime import datetime
from pathlib import Path

import numpy as np
import torch

from . import _lib

PARAMS = ("dense_1.weight", "dense_1.bias", "dense_2.weight", "dense_2.bias")
HEAD_PARAMS = ("logits.weight", "logits.bias")
_X_DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16, "fp16": torch.float16}   # 16-bit storage paths take 16-bit images


class VNCelebEmbDataset(torch.utils.data.Dataset):
    """label json {class: [image names]} + <data_dir>/<stem>.npz (arr_0) -> (embedding, label, path)."""

    def __init__(self, data_dir, label_file, transforms=None):
        self.data_dir = Path(data_dir)
        with open(label_file) as fp:
            self.label_dict = json.load(fp)
        self.transforms = transforms
        self.n_samples = sum(len(v) for v in self.label_dict.values())
        self.n_classes = len(self.label_dict)
        self.img_names, self.labels = [], []
        for k, v in self.label_dict.items():
            names = sorted(v)
            self.img_names += names
            self.labels += len(names) * [int(k)]

    def __len__(self):
        return self.n_samples

    def __getitem__(self, index):
        emb_path = self.data_dir / "{}.npz".format(self.img_names[index].split(".")[0])
        emb = np.load(str(emb_path))["arr_0"]
        data = self.transforms(emb) if self.transforms else torch.from_numpy(emb)
        return data, self.labels[index], str(emb_path)


class VNCelebDataset(torch.utils.data.Dataset):
    """label json {class: [image names]} + <data_dir>/<image name> -> (index, label, path).

    The reference decodes and transforms one image per __getitem__ on the host (vn_celeb_dataset.py:22-33).  Here every
    image is decoded once, at construction, and the whole set is one u8 array (N,S,S,3) that faces_device() keeps
    resident on the GPU; an item is the ROW of that array, so a DataLoader built from the config's own arguments still
    does the sampling (torch's sampler, torch's generator) while the pixels never leave the device.  Deviation
    (DESIGN.md 8): the images must be square and all of one size -- aligned face crops, what find_embedding.py and
    the demos' alignment write -- since one batch is one kernel launch over one array; anything else raises."""

    def __init__(self, data_dir, label_file, transforms=None):
        from PIL import Image
        self.data_dir = Path(data_dir)
        with open(label_file) as fp:
            self.label_dict = json.load(fp)
        self.transforms = transforms
        self.n_samples = sum(len(v) for v in self.label_dict.values())
        self.n_classes = len(self.label_dict)
        self.img_names, self.labels = [], []
        for k, v in self.label_dict.items():
            names = sorted(v)
            self.img_names += names
            self.labels += len(names) * [int(k)]
        faces = []
        for name in self.img_names:
            with Image.open(str(self.data_dir / name)) as im:
                a = np.asarray(im.convert("RGB"))
            if a.shape[0] != a.shape[1]:
                raise ValueError("%s is %dx%d: VNCelebDataset takes square face crops" % (name, a.shape[1], a.shape[0]))
            if faces and a.shape != faces[0].shape:
                raise ValueError("%s is %dx%d but %s is %dx%d: all images of a VNCelebDataset must have one size"
                                 % (name, a.shape[1], a.shape[0], self.img_names[0], faces[0].shape[1], faces[0].shape[0]))
            faces.append(a)
        self.faces = np.stack(faces) if faces else np.zeros((0, 0, 0, 3), np.uint8)
        self.size = int(self.faces.shape[1])
        self._dev = None

    def __len__(self):
        return self.n_samples

    def __getitem__(self, index):
        return index, self.labels[index], str(self.data_dir / self.img_names[index])

    def faces_device(self, device):
        """The data set as one cuda u8 tensor (N,S,S,3), uploaded at first use."""
        device = torch.device(device)
        if self._dev is None or self._dev.device != device:
            self._dev = torch.from_numpy(self.faces).to(device)
        return self._dev


def _check_labels(target, num_classes):
    """torch's nll_loss raises on a label outside [0, C) (trainer/classification_trainer.py:22 F.nll_loss): so does this,
    before any launch.  Returns the labels as an int64 host tensor."""
    th = torch.as_tensor(target).to(dtype=torch.int64)
    if th.numel() and (int(th.min()) < 0 or int(th.max()) >= num_classes):
        raise IndexError("Target %d is out of bounds." % int(th.max() if int(th.max()) >= num_classes else th.min()))
    return th


def _rows(ds, data):
    """What a loader over `ds` yields as `data` (the sampler's indices) -> int64 host tensor; an index outside `ds` raises."""
    index = torch.as_tensor(data, dtype=torch.int64)
    if index.numel() and (int(index.min()) < 0 or int(index.max()) >= len(ds)):
        raise IndexError("sample index outside the data set")
    return index


class _AdamTrained:
    """What TrainableMLP and TrainableHead share: a library handle that owns a set of Adam-trained tensors
    (csrc/adam_params.h), its mode, checkpoint access (vnf_trainer_*) and torch.optim.Adam's state_dict layout.  A
    subclass names its tensors: _shapes (state_dict key -> shape), _slots ((index in the Adam group, key), ...) and
    _n_group_params (the size of that group)."""

    def __init__(self, device, lr, betas, eps, weight_decay, max_batch):
        self.lr, self.betas, self.eps, self.weight_decay = float(lr), tuple(betas), float(eps), float(weight_decay)
        self.max_batch = int(max_batch)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("training runs on MI355X only (there is no CPU path)")
        self.training = True

    def _create(self, fn, state_dict, *args):
        """The handle: library function `fn`(initial values of `state_dict`, *args, max_batch, Adam's constants)."""
        lib = _lib.load()
        dev = self.device.index if self.device.index is not None else torch.cuda.current_device()
        with torch.cuda.device(dev):
            _lib.check(lib.vnf_init(dev))
            descs, n, keep = _lib.make_descs(state_dict)
            h = ctypes.c_void_p()
            _lib.check(getattr(lib, fn)(descs, n, *args, self.max_batch, self.betas[0], self.betas[1], self.eps, self.weight_decay,
                                        ctypes.byref(h)))
            del keep
        self._h = h
        self._loss = torch.zeros(1, dtype=torch.float32, device=self.device)
        self._hits = torch.zeros(1, dtype=torch.int32, device=self.device)

    def __del__(self):
        try:
            if getattr(self, "_h", None) is not None:
                _lib.load().vnf_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def train(self, mode=True):
        self.training = bool(mode)
        return self

    def eval(self):
        return self.train(False)

    def to(self, device):
        return self

    def _run(self, fn, x, t, b, *extra):
        """Library function `fn`(handle, x, t, b, *extra, loss, hits, stream) -> (mean NLL, correct count)."""
        with torch.cuda.device(self.device):
            _lib.check(getattr(_lib.load(), fn)(
                self._h, ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(t.data_ptr()), b, *extra,
                ctypes.c_void_p(self._loss.data_ptr()), ctypes.c_void_p(self._hits.data_ptr()), _lib.current_stream_ptr()))
        return float(self._loss.item()), int(self._hits.item())

    # ---- checkpoint access
    def _get(self, name, kind):
        a = np.empty(self._shapes[name], dtype=np.float32)
        _lib.check(_lib.load().vnf_trainer_get(self._h, name.encode(), kind, a.ctypes.data, a.size))
        return torch.from_numpy(a)

    def _set(self, name, kind, value):
        a = np.ascontiguousarray(torch.as_tensor(value).detach().cpu().float().numpy())
        if a.shape != self._shapes[name]:
            raise RuntimeError("size mismatch for %s: %s vs %s" % (name, a.shape, self._shapes[name]))
        _lib.check(_lib.load().vnf_trainer_set(self._h, name.encode(), kind, a.ctypes.data, a.size))

    def _step_count(self, value=None):
        c = ctypes.c_int64(0 if value is None else int(value))
        _lib.check(_lib.load().vnf_trainer_step_count(self._h, ctypes.byref(c), 0 if value is None else 1))
        return int(c.value)

    def optimizer_state_dict(self):
        """torch.optim.Adam.state_dict() layout over the reference's `Adam(model.parameters())` group, so the reference's
        resume_checkpoint (base_trainer.py:73-80) can load it into a torch Adam and vice versa.  MLPModel: params 0..3 in
        state_dict order.  A frozen encoder: every parameter of the module is in the group, only the two of `logits` ever
        got a gradient and therefore a state entry."""
        step = float(self._step_count())
        state = {i: {"step": torch.tensor(step), "exp_avg": self._get(k, 1), "exp_avg_sq": self._get(k, 2)}
                 for i, k in self._slots} if step > 0 else {}
        group = torch.optim.Adam([torch.zeros(1)], lr=self.lr, betas=self.betas, eps=self.eps,
                                 weight_decay=self.weight_decay).state_dict()["param_groups"][0]
        group["params"] = list(range(self._n_group_params))
        return {"state": state, "param_groups": [group]}

    def load_optimizer_state_dict(self, osd):
        g = osd["param_groups"][0]
        self.lr = float(g["lr"])
        if osd["state"]:
            for i, k in self._slots:
                self._set(k, 1, osd["state"][i]["exp_avg"])
                self._set(k, 2, osd["state"][i]["exp_avg_sq"])
            self._step_count(int(float(osd["state"][self._slots[0][0]]["step"])))


class TrainableMLP(_AdamTrained):
    """MLPModel(input_dim, num_classes) + its Adam state, resident on the GPU (vnf_mlp_trainer_create, vnf_mlp_train_step).
    Initial weights are drawn exactly as `nn.Linear(input_dim, 2048); nn.Linear(2048, num_classes)` draws them (same
    generator calls)."""

    def __init__(self, input_dim, num_classes, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_batch=1024,
                 device="cuda:0"):
        self.input_dim, self.num_classes = int(input_dim), int(num_classes)
        super().__init__(device, lr, betas, eps, weight_decay, max_batch)
        d1, d2 = torch.nn.Linear(self.input_dim, 2048), torch.nn.Linear(2048, self.num_classes)
        sd = OrderedDict([("dense_1.weight", d1.weight), ("dense_1.bias", d1.bias), ("dense_2.weight", d2.weight),
                          ("dense_2.bias", d2.bias)])
        self._shapes = {k: tuple(v.shape) for k, v in sd.items()}
        self._slots, self._n_group_params = tuple(enumerate(PARAMS)), len(PARAMS)
        self._create("vnf_mlp_trainer_create", OrderedDict((k, v.detach()) for k, v in sd.items()), self.input_dim, self.num_classes)

    def step(self, data, target, train):
        """One batch: forward + loss (+ backward + Adam when train).  Returns (mean NLL, correct count).  In training
        mode the dropout factors of F.dropout(x, 0.5) are drawn from torch's CPU generator, as the reference's forward
        on a CPU tensor would draw them (models/mlp_model.py:12)."""
        b = int(data.shape[0])
        x = data.to(self.device, dtype=torch.float32).contiguous()
        t = _check_labels(target, self.num_classes).to(self.device).contiguous()
        mask = None
        if train:
            mask = (torch.empty((b, 2048), dtype=torch.float32).bernoulli_(0.5) / 0.5).to(self.device)
        return self._run("vnf_mlp_train_step", x, t, b, ctypes.c_void_p(mask.data_ptr()) if mask is not None else None, self.lr,
                         1 if train else 0)

    def state_dict(self):
        return OrderedDict((k, self._get(k, 0)) for k in PARAMS)

    def load_state_dict(self, sd):
        for k in PARAMS:
            if k not in sd:
                raise RuntimeError("Missing key(s) in state_dict: %s" % k)
            self._set(k, 0, sd[k])


def head_param_layout(spec):
    """(P, index of logits.weight, index of logits.bias) in `Adam(model.parameters())` of the reference module whose
    state_dict `spec` (weights.py) lists: parameters() follows the state_dict's order without the BatchNorms' running
    statistics and step counters, and freeze_weights (iresnet_encoder.py:174-179) leaves every parameter in the group."""
    params = [name for name, _, kind in spec if kind not in ("bn_m", "bn_v", "nbt")]
    return len(params), params.index(HEAD_PARAMS[0]), params.index(HEAD_PARAMS[1])


class TrainableHead(_AdamTrained):
    """The `logits` layer of a frozen encoder + its Adam state, resident on the GPU (vnf_head_trainer_create, vnf_head_train_step): the
    counterpart of TrainableMLP for iresnet100(n_classes=..., freeze_weights=True) / InceptionResnetV1(classify=True,
    freeze_weights=True).  The encoder only ever runs forward, in eval mode; the initial head is the encoder's own."""

    def __init__(self, encoder, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_batch=1024):
        if encoder.head_classes is None:
            raise RuntimeError("%s was built without a classification head (classify=True / n_classes)" % type(encoder).__name__)
        self.encoder, self.num_classes = encoder, int(encoder.head_classes)
        super().__init__(encoder.device, lr, betas, eps, weight_decay, max_batch)
        self.encoder.eval()
        self.arch_name = encoder.arch_name
        self.input_size = encoder.input_size
        self.x_dtype = _X_DTYPES.get(encoder.compute_dtype, torch.float32)
        self.n_params, self._iw, self._ib = head_param_layout(encoder._spec())
        self._shapes = {HEAD_PARAMS[0]: (self.num_classes, 512), HEAD_PARAMS[1]: (self.num_classes,)}
        self._slots, self._n_group_params = ((self._iw, HEAD_PARAMS[0]), (self._ib, HEAD_PARAMS[1])), self.n_params
        esd = encoder.state_dict()
        self._create("vnf_head_trainer_create", OrderedDict((k, esd[k]) for k in HEAD_PARAMS), self.num_classes)

    def train(self, mode=True):
        """The head's mode.  The backbone stays in eval mode whatever this says: frozen means frozen."""
        return super().train(mode)

    def features(self, x):
        """(N,3,S,S) cuda -> (N,512) fp32 cuda: what the head reads (encoders._Encoder.features)."""
        return self.encoder.features(x)

    def step(self, features, target, train):
        """One batch of features (b,512): forward + loss (+ the fused gradient / Adam launch when train).  Returns
        (mean NLL, correct count)."""
        b = int(features.shape[0])
        if features.dim() != 2 or features.shape[1] != 512:
            raise ValueError("expected (b,512) features, got %s" % (tuple(features.shape),))
        th = _check_labels(target, self.num_classes)
        if th.numel() != b:
            raise ValueError("%d targets for a batch of %d" % (th.numel(), b))
        x = features.to(self.device, dtype=torch.float32).contiguous()
        return self._run("vnf_head_train_step", x, th.to(self.device).contiguous(), b, self.lr, 1 if train else 0)

    def state_dict(self):
        """The encoder's full state_dict with `logits.*` replaced by the trained values."""
        sd = self.encoder.state_dict()
        for k in HEAD_PARAMS:
            sd[k] = self._get(k, 0)
        return sd

    def load_state_dict(self, sd):
        """The backbone goes into the encoder (strictly, as nn.Module.load_state_dict), `logits.*` into the trainer."""
        self.encoder.load_state_dict(sd)
        for k in HEAD_PARAMS:
            self._set(k, 0, sd[k])


class EvalModel:
    """A trained model under evaluation (eval.py): an inference MLPModel (classifier.py) or an encoder with its own
    `logits` head (encoders.py), anything that maps a cuda batch to cuda (n,C) log-probabilities.  evaluate() is the
    device step of _validate_epoch (classification_trainer.py:50-72): log-probabilities + targets -> the batch sums
    and, when asked, the per-row prediction and probability (vnf_logits_eval); the (n,C) matrix stays on the device."""

    def __init__(self, model, num_classes, device="cuda:0"):
        self.model, self.num_classes = model, int(num_classes)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("evaluation runs on MI355X only (there is no CPU path)")
        self.model.to(self.device)
        self.model.eval()
        self.training = False
        self.input_size = getattr(model, "input_size", None)   # encoders: side of the images they take
        self.x_dtype = _X_DTYPES.get(getattr(model, "compute_dtype", None), torch.float32)

    def eval(self):
        return self

    def train(self, mode=True):
        if mode:
            raise NotImplementedError("EvalModel evaluates; train.py trains (TrainableMLP)")
        return self

    def to(self, device):
        return self

    def state_dict(self):
        return self.model.state_dict()

    def load_state_dict(self, sd):
        self.model.load_state_dict(sd)

    def load_optimizer_state_dict(self, osd):
        pass    # a checkpoint's Adam state has no use in evaluation

    def evaluate(self, data, target, rows=False):
        """One batch -> (sum of the rows' NLL, correct count, predictions (n,) int32 cuda, probabilities (n,) fp32 cuda);
        the last two are None unless `rows`.  The host reads the two sums (and nothing else)."""
        from .classifier import check_targets, logits_eval
        t = check_targets(target, self.num_classes)
        x = data.to(self.device)
        if x.shape[0] != t.numel():
            raise ValueError("%d targets for a batch of %d" % (t.numel(), x.shape[0]))
        if x.shape[0] == 0:
            e = torch.zeros((0,), device=self.device)
            return 0.0, 0, (e.to(torch.int32) if rows else None), (e if rows else None)
        logp = self.model(x)
        want = ("nll", "hit", "sums") + (("amax", "prob") if rows else ())
        r = logits_eval(logp, t, want=want)
        sums = r["sums"].cpu()
        return float(sums[0]), int(sums[1]), r.get("amax"), r.get("prob")


def write_result_csv(rows, path):
    """result.csv of BaseTrainer.eval(save_result=True) (base_trainer.py:182-192): rows of (path, target, prediction,
    probability) under the header Path,Target,Prediction,Probability, no index column, as DataFrame.to_csv writes them
    (minimal quoting, "\n" line ends, floats by their shortest round-trip repr)."""
    with open(path, "w", newline="") as f:
        w = csv.writer(f, lineterminator="\n")
        w.writerow(["Path", "Target", "Prediction", "Probability"])
        for pth, tgt, pred, prob in rows:
            w.writerow([str(pth), int(tgt), int(pred), repr(float(prob))])


class ReduceLROnPlateau:
    """torch.optim.lr_scheduler.ReduceLROnPlateau (cooldown 0, eps 1e-8) acting on TrainableMLP.lr."""

    def __init__(self, model, mode="min", factor=0.1, patience=10, threshold=1e-4, threshold_mode="rel", cooldown=0,
                 min_lr=0.0, eps=1e-8, verbose=False):
        self.model, self.mode, self.factor, self.patience = model, mode, factor, patience
        self.threshold, self.threshold_mode, self.cooldown, self.min_lr, self.eps = threshold, threshold_mode, cooldown, min_lr, eps
        self.best = float("inf") if mode == "min" else -float("inf")
        self.num_bad_epochs, self.cooldown_counter = 0, 0

    def _better(self, a, best):
        if self.mode == "min":
            return a < (best * (1.0 - self.threshold) if self.threshold_mode == "rel" else best - self.threshold)
        return a > (best * (self.threshold + 1.0) if self.threshold_mode == "rel" else best + self.threshold)

    def step(self, metric):
        current = float(metric)
        if self._better(current, self.best):
            self.best, self.num_bad_epochs = current, 0
        else:
            self.num_bad_epochs += 1
        if self.cooldown_counter > 0:
            self.cooldown_counter -= 1
            self.num_bad_epochs = 0
        if self.num_bad_epochs > self.patience:
            new_lr = max(self.model.lr * self.factor, self.min_lr)
            if self.model.lr - new_lr > self.eps:
                self.model.lr = new_lr
            self.cooldown_counter, self.num_bad_epochs = self.cooldown, 0


class MetricTracker:
    def __init__(self, *keys):
        self.keys = keys
        self.reset()

    def reset(self):
        self.total = {k: 0.0 for k in self.keys}
        self.counts = {k: 0 for k in self.keys}

    def update(self, key, value, n=1):
        self.total[key] += value * n
        self.counts[key] += n

    def avg(self, key):
        return self.total[key] / self.counts[key] if self.counts[key] else 0

    def result(self):
        return {k: self.avg(k) for k in self.keys}


class ClassificationTrainer:
    def __init__(self, config, model, lr_scheduler, run_id=None):
        self.config, self.model, self.lr_scheduler = config, model, lr_scheduler
        tc = config["trainer"]
        self.start_epoch, self.epochs = 1, tc["epochs"]
        self.tracked_metric, self.mode_monitor = tc["tracked_metric"]
        self.early_stop, self.save_step, self.log_step = tc["patience"], tc["save_period"], tc["log_step"]
        self.loss_name, self.metric_names = config["loss"], list(config["metrics"])
        if self.loss_name != "neg_log_llhood" or self.metric_names != ["accuracy"]:
            raise NotImplementedError("the fused step computes NLLLoss and accuracy (losses/__init__.py, metrics.py)")
        self.train_loss, self.train_metrics = MetricTracker(self.loss_name), MetricTracker(*self.metric_names)
        self.val_loss, self.val_metrics = MetricTracker(self.loss_name), MetricTracker(*self.metric_names)
        run_id = run_id or datetime.now().strftime(r"%m%d_%H%M%S")
        self.save_dir = Path(tc["save_dir"]) / "models" / run_id
        self.log_dir = Path(tc["save_dir"]) / "logs" / run_id
        os.makedirs(self.save_dir, exist_ok=True)
        os.makedirs(self.log_dir, exist_ok=True)
        logging.basicConfig(level=logging.INFO)
        self.logger = logging.getLogger("trainer")
        self.do_val, self.val_step = tc["do_validation"], tc["validation_step"]
        self.mnt_best = float("inf") if self.mode_monitor == "min" else -float("inf")
        self._kept = {}    # _kept_rows: the frozen encoder's output for a whole data set under the default transform, by `train`
        if tc["resume_path"] != "":
            self.resume_checkpoint(tc["resume_path"])

    def setup_loader(self, train_loader, val_loader):
        self.train_loader, self.val_loader = train_loader, val_loader

    def _images(self, ds, data, transform):
        """Rows `data` of the resident image set through `transform`, as the model's input tensor."""
        from . import augment
        index = _rows(ds, data)
        t = getattr(self.model, "input_size", None)
        if t is None:
            raise NotImplementedError("VNCelebDataset under ClassificationTrainer needs a model that takes images")
        if ds.size != t:
            raise ValueError("the images are %dx%d but the model takes %dx%d: transforms.resize is not built (DESIGN.md 8)"
                             % (ds.size, ds.size, t, t))
        params = augment.get_transform(transform).params(int(index.numel()), ds.size, t)
        return augment.augment_faces_device(ds.faces_device(self.model.device), index, params, t, dtype=self.model.x_dtype)

    def _head_features(self, ds, data, train):
        """A TrainableHead's input: the frozen encoder's features of rows `data`.  The default transform draws nothing and
        the backbone never changes, so under it the features of the whole set are computed once and kept: always for
        validation (train.py:30-34), for training when transforms.name is default."""
        tf = self.config.get("transforms")
        name = (tf.get("name") if isinstance(tf, dict) else tf) if train else "default"
        if name != "default":
            return self.model.features(self._images(ds, data, name))
        return self._kept_rows(train, ds, lambda index: self.model.features(self._images(ds, index, "default")),
                               self.model.encoder.max_batch, data)

    def _kept_rows(self, key, ds, embed_fn, batch, data):
        """Rows `data` of embed_fn (row indices -> cuda (n,512)) over all of `ds`, which is computed once, `batch` rows (the
        encoder's max_batch) at a time, and kept under `key`."""
        if key not in self._kept:
            self._kept[key] = torch.cat([embed_fn(torch.arange(i, min(i + batch, len(ds)))) for i in range(0, len(ds), batch)]) \
                if len(ds) else torch.zeros((0, 512), device=self.model.device)
        return self._kept[key][_rows(ds, data).to(self._kept[key].device)]

    def _batch_input(self, data, train):
        """What the loader yields -> what the model takes: the embeddings themselves; for a VNCelebDataset (rows of the
        resident image set) the frozen encoder's features when the model is a TrainableHead in the training loop, and
        under evaluation the images through the default transform (eval.py:24-40)."""
        ds = (self.train_loader if train else self.val_loader).dataset
        if isinstance(ds, VNCelebDataset) and isinstance(self.model, TrainableHead):
            return self._head_features(ds, data, train)
        if isinstance(ds, VNCelebDataset) and not train:
            return self._images(ds, data, "default")
        return data

    def resume_checkpoint(self, checkpoint_path):
        cp = torch.load(checkpoint_path, map_location="cpu", weights_only=True)
        self.logger.info("Loading checkpoint: {} ...".format(checkpoint_path))
        self.start_epoch = cp["epoch"] + 1
        self.mnt_best = cp["monitor_best"]
        self.model.load_state_dict(cp["state_dict"])
        self.model.load_optimizer_state_dict(cp["optimizer"])
        self.logger.info("Checkpoint loaded. Resume training from epoch {}".format(self.start_epoch))

    def save_checkpoint(self, epoch, save_best):
        state = {"arch": getattr(self.model, "arch_name", "MLPModel"), "epoch": epoch, "state_dict": self.model.state_dict(),
                 "optimizer": self.model.optimizer_state_dict(), "monitor_best": self.mnt_best, "config": self.config}
        filename = str(self.save_dir / "checkpoint-epoch{}.pth".format(epoch))
        torch.save(state, filename)
        self.logger.info("Saving checkpoint: {} ...".format(filename))
        if save_best:
            torch.save(state, str(self.save_dir / "model_best.pth"))
            self.logger.info("Saving current best: model_best.pth ...")

    def _train_epoch(self, epoch):
        self.model.train()
        for t in (self.train_loss, self.train_metrics, self.val_loss, self.val_metrics):
            t.reset()
        for batch_idx, (data, target, _id) in enumerate(self.train_loader):
            data = self._batch_input(data, train=True)
            loss, hits = self.model.step(data, target, train=True)
            self.train_loss.update(self.loss_name, loss)
            self.train_metrics.update("accuracy", hits / data.size(0), n=data.size(0))
            if batch_idx % self.log_step == 0:
                self.logger.info("Train Epoch: {} [{}]/[{}] with NLLLoss, Loss: {:.6f}".format(
                    epoch, batch_idx, len(self.train_loader), self.train_loss.avg(self.loss_name)))
                self.logger.info("accuracy: {:.6f}".format(self.train_metrics.avg("accuracy")))
        log = self.train_loss.result()
        log.update(self.train_metrics.result())
        if self.do_val and (epoch % self.val_step == 0):
            log.update(self._validate_epoch(epoch))
        if isinstance(self.lr_scheduler, ReduceLROnPlateau):
            self.lr_scheduler.step(self.val_loss.avg(self.loss_name))
        return log

    def _evaluator(self, save_result):
        """Who scores a validation batch: the model itself when it is an EvalModel; None for the training model inside
        the training loop (its own forward + loss, TrainableMLP.step / TrainableHead.step); and, when the rows are wanted
        from a training model, an inference model of its current weights: an MLPModel, or the encoder with the current head."""
        if hasattr(self.model, "evaluate"):
            return self.model
        if not save_result:
            return None
        if isinstance(self.model, TrainableHead):
            enc = self.model.encoder
            enc.load_state_dict(self.model.state_dict())
            return EvalModel(enc, self.model.num_classes, device=self.model.device)
        from .classifier import MLPModel
        mlp = MLPModel(self.model.input_dim, self.model.num_classes, max_batch=self.model.max_batch)
        mlp.load_state_dict(self.model.state_dict())
        return EvalModel(mlp, self.model.num_classes, device=self.model.device)

    def _validate_epoch(self, epoch, save_result=False):
        """classification_trainer.py:42-80: the loss is the mean of the batch means, the accuracy is weighted by batch
        size; with save_result also [paths, targets, predictions, probabilities] per batch."""
        self.model.eval()
        self.val_loss.reset()
        self.val_metrics.reset()
        self.logger.info("Validation: ")
        evaluator = self._evaluator(save_result)
        result = []
        head_rows = evaluator is not None and isinstance(self.model, TrainableHead)   # the encoder itself scores: it takes images
        for batch_idx, (data, target, id_img) in enumerate(self.val_loader):
            data = self._images(self.val_loader.dataset, data, "default") if head_rows else self._batch_input(data, train=False)
            n = data.size(0)
            if evaluator is None:
                loss, hits = self.model.step(data, target, train=False)
            else:
                sum_nll, hits, amax, prob = evaluator.evaluate(data, target, rows=save_result)
                loss = float(np.float32(sum_nll) / np.float32(n))    # F.nll_loss's mean, in fp32
                if save_result:
                    result.append([id_img, torch.as_tensor(target), amax.cpu(), prob.cpu().tolist()])
            self.val_loss.update(self.loss_name, loss)
            self.val_metrics.update("accuracy", hits / n, n=n)
        log = self.val_loss.result()
        log.update(self.val_metrics.result())
        val_log = {"val_{}".format(k): v for k, v in log.items()}
        if save_result:
            return val_log, result
        return val_log

    def eval(self, save_result=False):
        """base_trainer.py:177-200: one pass over val_loader; with save_result also <save_dir>/models/<run_id>/result.csv."""
        if save_result:
            log, result = self._validate_epoch(1, save_result)
            res_path = str(self.save_dir / "result.csv")
            ids, targets, predictions, probs = [], [], [], []
            for batch_pred in result:
                ids += list(batch_pred[0])
                targets += list(batch_pred[1].cpu().numpy())
                predictions += list(batch_pred[2].cpu().numpy())
                probs += list(batch_pred[3])
            write_result_csv(zip(ids, targets, predictions, probs), res_path)
            print("Saved prediction to {}.".format(res_path))
        else:
            log = self._validate_epoch(1)
        for key, value in log.items():
            self.logger.info("    {:15s}: {}".format(str(key), value))
        return log

    def train(self, track4plot=False):
        not_improve_count = 0
        if track4plot:
            self.track4plot = str(self.log_dir / "log_loss.txt")
            with open(self.track4plot, "a") as f:
                f.write(",".join(["Epoch", "Train_loss", "Validation_loss"]) + "\n")
        for epoch in range(self.start_epoch, self.epochs + 1):
            result = self._train_epoch(epoch)
            if track4plot:
                with open(self.track4plot, "a") as f:
                    f.write(",".join(str(x) for x in [epoch, result.get(self.loss_name), result.get("val_" + self.loss_name)]) + "\n")
            log = {"epoch": epoch}
            log.update(result)
            for key, value in log.items():
                self.logger.info("    {:15s}: {}".format(str(key), value))
            best = False
            tracked = log.get(self.tracked_metric)
            if tracked:
                improved = (self.mode_monitor == "min" and tracked < self.mnt_best) or \
                           (self.mode_monitor == "max" and tracked > self.mnt_best)
                if improved:
                    self.mnt_best, not_improve_count, best = tracked, 0, True
                else:
                    not_improve_count += 1
            if not_improve_count > self.early_stop:
                self.logger.info("Validation performance didn't improve for {} epochs. Training stops.".format(self.early_stop))
                break
            if epoch % self.save_step == 0:
                self.save_checkpoint(epoch, save_best=best)


class AugClassificationTrainer(ClassificationTrainer):
    """trainer/online_aug_trainer.py:6-97: the frozen encoder of trainer.encoders[trainer.chosen_idx_enc] embeds every
    batch inside the loop.  A training batch is: rows of the resident data set (VNCelebDataset) -> the draws of
    `transforms.name` -> vnf_augment_faces -> encoder -> the fused MLP step; a validation batch takes the default
    transform (train.py:30-34).  Nothing between the sampler's indices and the loss scalar touches the host.  The
    encoder is frozen and the default transform draws nothing, so the validation embeddings are computed once and
    kept.  Log lines, checkpoints, scheduler and early stop are ClassificationTrainer's."""

    def __init__(self, config, model, lr_scheduler, run_id=None):
        super().__init__(config, model, lr_scheduler, run_id=run_id)
        from . import augment, models
        tc = config["trainer"]
        info = tc["encoders"][tc["chosen_idx_enc"]]
        self.encoder = getattr(models, info["name"])(**info.get("args", {}))
        self.encoder.to(self.model.device)
        self.encoder.eval()
        tf = config["transforms"]
        if tf.get("resize"):
            raise NotImplementedError("transforms.resize is not built: crop the faces at the encoder's input size (DESIGN.md 8)")
        self.transform = augment.get_transform(tf["name"])
        self.val_transform = augment.get_transform("default")
        self.x_dtype = _X_DTYPES.get(self.encoder.compute_dtype, torch.float32)   # the encoder's own input dtype

    def embed(self, dataset, index, transform):
        """Rows `index` of `dataset` through `transform` and the encoder: cuda (n,512) fp32."""
        from . import augment
        t = self.encoder.input_size
        faces = dataset.faces_device(self.model.device)
        index = _rows(dataset, index)
        params = transform.params(int(index.numel()), dataset.size, t)
        return self.encoder(augment.augment_faces_device(faces, index, params, t, dtype=self.x_dtype))

    def _batch_input(self, data, train):
        if train:
            return self.embed(self.train_loader.dataset, data, self.transform)
        ds = self.val_loader.dataset
        return self._kept_rows(train, ds, lambda index: self.embed(ds, index, self.val_transform), self.encoder.max_batch, data)
