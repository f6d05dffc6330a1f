"""GPU: training the `logits` head of a frozen encoder (csrc/head_train.hip, trainer.TrainableHead,
train.py's third route) against the float64 CPU oracle of tests/head_train_oracle.py."""
import copy
import ctypes
import json
import os
import sys
from collections import OrderedDict

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from aug_golden import aug_train_config, write_face_dataset
from conftest import GOLDEN, REPO, seeded_normal
from head_train_oracle import CASES, LR, MIN_GAP, WEIGHT_DECAY, case_inputs, oracle_run

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


class _HeadOnly:
    """What TrainableHead asks of an encoder, without a backbone: a `logits` layer behind one frozen tensor."""
    arch_name, input_size, compute_dtype, max_batch = "HeadOnly", 112, "f32", 8

    def __init__(self, w, bias):
        self.device = torch.device(DEV)
        self.head_classes = int(w.shape[0])
        self._sd = OrderedDict([("stem.weight", torch.arange(4.0)), ("logits.weight", w.clone()), ("logits.bias", bias.clone())])

    def eval(self):
        return self

    def _spec(self):
        return [(k, tuple(v.shape), "conv") for k, v in self._sd.items()]

    def state_dict(self):
        return OrderedDict(self._sd)

    def load_state_dict(self, sd):
        self._sd = OrderedDict((k, sd[k]) for k in self._sd)


def _head(w, bias, max_batch=64, lr=LR, weight_decay=WEIGHT_DECAY):
    from vn_celeb_face_recognition_amd.trainer import TrainableHead
    return TrainableHead(_HeadOnly(w, bias), lr=lr, weight_decay=weight_decay, max_batch=max_batch)


def _bits(head):
    return [head._get(k, kind).numpy().view(np.uint32).copy() for k in ("logits.weight", "logits.bias") for kind in (0, 1, 2)] \
        + [head._step_count()]


def _same_bits(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def _check_against_oracle(tag, got_w, got_b, got_loss, want, got_v=None):
    """The bars of the step-parity check (W and bias together, against the float64 oracle): >= 99.9 % of the elements
    within 2e-7, every element within 1e-4, each step's loss within 2e-5 relative, exp_avg_sq within rtol 2e-3 / atol 1e-12."""
    d = torch.cat([(got_w.double() - want["weight"]).abs().flatten(), (got_b.double() - want["bias"]).abs().flatten()])
    share = float((d <= 2e-7).double().mean())
    lerr = max(abs(g - w) / abs(w) for g, w in zip(got_loss, want["loss"]))
    print("%s: |param - oracle| max %.3e, 99.9th pct %.3e, within 2e-7: %.5f %%; loss rel err max %.3e"
          % (tag, float(d.max()), float(torch.quantile(d, 0.999)) if d.numel() > 1 else float(d.max()), 100 * share, lerr))
    if got_v is not None:
        for k, v in got_v.items():
            ref = want["exp_avg_sq_" + k]
            print("%s: exp_avg_sq %s max rel err %.3e" % (tag, k, float(((v.double() - ref).abs() / ref.abs().clamp_min(1e-30)).max())))
            assert torch.allclose(v.double(), ref, rtol=2e-3, atol=1e-12), k
    assert share >= 0.999, share
    assert float(d.max()) <= 1e-4
    assert lerr <= 2e-5


# ------------------------------------------------------------------------------------------------ 1. step parity
@pytest.fixture(scope="module")
def oracles():
    out = {}
    for c, b in CASES:
        w, bias, batches = case_inputs(c, b)
        out[(c, b)] = (w, bias, batches, oracle_run(w, bias, batches))
    return out


@pytest.mark.parametrize("c,b", CASES)
def test_step_matches_the_float64_oracle(oracles, c, b):
    w, bias, batches, want = oracles[(c, b)]
    assert want["gap"] > MIN_GAP, want["gap"]          # the precondition of equal hit counts, asserted and not skipped
    head = _head(w, bias, max_batch=b)
    got = [head.step(f.to(DEV), t, train=True) for f, t in batches]
    assert [h for _, h in got] == want["hits"]
    assert head._step_count() == len(batches)
    _check_against_oracle("C=%d b=%d" % (c, b), head._get("logits.weight", 0), head._get("logits.bias", 0), [l for l, _ in got], want,
                          {"weight": head._get("logits.weight", 2), "bias": head._get("logits.bias", 2)})
    moved = float((head._get("logits.weight", 0) - w).abs().max())
    assert moved > 1e-3, moved                          # six steps of lr 1e-3 move the weights by ~6e-3: the bars see a wrong update


# ------------------------------------------------------------------------------------------------ 2. eval step
@pytest.mark.parametrize("c,b", [(17, 5), (1020, 37)])
def test_eval_step_leaves_the_state_alone(c, b):
    w, bias, batches = case_inputs(c, b, steps=2)
    head = _head(w, bias, max_batch=b)
    head.step(batches[0][0].to(DEV), batches[0][1], train=True)       # moments and step count are not all zero
    before = _bits(head)
    f, t = batches[1][0].to(DEV), batches[1][1]
    ev = head.step(f, t, train=False)
    assert _same_bits(before, _bits(head)) and head._step_count() == 1
    assert head.step(f, t, train=False) == ev
    assert head.step(f, t, train=True) == ev            # the forward of a training step on the same batch
    assert not _same_bits(before, _bits(head)) and head._step_count() == 2


# ------------------------------------------------------------------------------------------------ 3. repeatability, resume
def test_repeatable_resumable_and_guarded():
    from vn_celeb_face_recognition_amd import _lib
    c, b = 1020, 37
    w, bias, batches = case_inputs(c, b)
    a, a2 = _head(w, bias, max_batch=b), _head(w, bias, max_batch=b)
    la = [a.step(f.to(DEV), t, train=True) for f, t in batches]
    la2 = [a2.step(f.to(DEV), t, train=True) for f, t in batches]
    assert la == la2 and _same_bits(_bits(a), _bits(a2))
    # three steps, checkpoint into a fresh head, three more
    first = _head(w, bias, max_batch=b)
    l1 = [first.step(f.to(DEV), t, train=True) for f, t in batches[:3]]
    osd, sd = first.optimizer_state_dict(), first.state_dict()
    assert sorted(osd["state"]) == [1, 2] and osd["param_groups"][0]["params"] == [0, 1, 2] and list(sd) == ["stem.weight", "logits.weight", "logits.bias"]
    assert float(osd["state"][1]["step"]) == 3.0 and sorted(osd["state"][2]) == ["exp_avg", "exp_avg_sq", "step"]
    fresh = _head(torch.zeros_like(w), torch.zeros_like(bias), max_batch=b, lr=0.5)
    fresh.load_state_dict(sd)
    fresh.load_optimizer_state_dict(osd)
    assert fresh.lr == LR
    l2 = [fresh.step(f.to(DEV), t, train=True) for f, t in batches[3:]]
    assert l1 + l2 == la and _same_bits(_bits(fresh), _bits(a))
    # labels outside [0, C) raise before any launch; a batch beyond max_batch is refused
    before = _bits(a)
    f, t = batches[0]
    for bad in (c, -1):
        tb = t.clone()
        tb[5] = bad
        with pytest.raises(IndexError, match="Target %d is out of bounds" % bad):
            a.step(f.to(DEV), tb, train=True)
    with pytest.raises(_lib.VnfError, match="max_batch"):
        a.step(torch.zeros((b + 1, 512), device=DEV), torch.zeros(b + 1, dtype=torch.int64), train=True)
    assert _same_bits(before, _bits(a))


# ------------------------------------------------------------------------------------------------ 4. vnf_encoder_features
@pytest.mark.parametrize("dt,kw", [("f32", {"n_classes": 5}), ("f16x2", {})])      # with and without a head
def test_features_ir100_are_the_embeddings(dt, kw):
    from vn_celeb_face_recognition_amd import _lib, models
    x = seeded_normal((3, 3, 112, 112), 31).to(DEV)
    m = models.iresnet100(compute_dtype=dt, max_batch=2, **kw).to(DEV).eval()       # batch 3 over max_batch 2: two calls
    f = m.features(x)
    assert f.shape == (3, 512) and f.dtype == torch.float32 and torch.equal(f, m.embed(x))
    assert float(f.abs().max()) > 0 and bool(torch.isfinite(f).all())
    out = torch.empty((3, 512), device=DEV)
    lib = _lib.load()
    rc = lib.vnf_encoder_features(m._ensure_handle(), ctypes.c_void_p(x.data_ptr()), 3, _lib.VNF_F32, ctypes.c_void_p(out.data_ptr()),
                                  _lib.current_stream_ptr())
    assert rc == -4                                     # VNF_E_CAPACITY
    assert lib.vnf_encoder_features(m._ensure_handle(), None, 0, _lib.VNF_F32, None, _lib.current_stream_ptr()) == 0


@pytest.mark.parametrize("dt", ["f32", "f16x2"])
def test_features_irv1_are_what_the_head_reads(dt):
    from vn_celeb_face_recognition_amd import models
    x = seeded_normal((3, 3, 160, 160), 32).to(DEV)
    m = models.InceptionResnetV1(pretrained=None, classify=True, num_classes=7, compute_dtype=dt, max_batch=4).to(DEV).eval()
    f = m.features(x)
    sd = m.state_dict()
    want = F.log_softmax(f.cpu().double() @ sd["logits.weight"].double().T + sd["logits.bias"].double(), dim=1)
    logp = m.logprobs(x)[0].cpu().double()
    err, scale = float((logp - want).abs().max()), float(want.abs().max())
    nerr = float((F.normalize(f, p=2, dim=1) - m.embed(x)).abs().max())
    print("irv1 %s: logprobs vs log_softmax(features W^T + b) %.3e (max |logp| %.2f); normalize(features) vs embed %.3e" % (dt, err, scale, nerr))
    assert err <= 1e-4 * scale
    assert nerr <= 1e-6
    assert float(f.norm(dim=1).min()) > 1.5             # the features themselves, not the unit rows
    if dt == "f32":                                     # a handle without a head gives the same rows
        plain = models.InceptionResnetV1(pretrained=None, compute_dtype=dt, max_batch=4).to(DEV).eval()
        assert torch.equal(plain.features(x), f)


# ------------------------------------------------------------------------------------------------ 5. end to end
def _head_train_config(root, transforms, epochs, save_period):
    cfg = aug_train_config(root, transforms=transforms, epochs=epochs, n_cls=3)
    cfg["model"] = {"name": "iresnet100", "args": {"n_classes": 3, "freeze_weights": True, "compute_dtype": "f32"}}
    cfg["transforms"]["encoder_img_size"] = 112
    cfg["train_data_loader"]["args"]["batch_size"] = 5           # 12 images: batches of 5, 5, 2
    cfg["val_data_loader"]["args"]["batch_size"] = 4
    cfg["trainer"] = {k: v for k, v in cfg["trainer"].items() if k not in ("chosen_idx_enc", "encoders")}
    cfg["trainer"].update(name="ClassificationTrainer", save_period=save_period)
    cfg["optimizer"]["args"] = {"lr": LR, "weight_decay": WEIGHT_DECAY}
    return cfg


def test_train_py_head_route_end_to_end(tmp_path, monkeypatch):
    sys.path.insert(0, REPO)
    import eval as ev
    import train
    from vn_celeb_face_recognition_amd.trainer import TrainableHead
    from vn_celeb_face_recognition_amd.weights import generate_state_dict
    ref = json.load(open(os.path.join(GOLDEN, "head_train_ref.json")))
    root = str(tmp_path)
    write_face_dataset(root, size=112, n_cls=3, per_cls_train=4, per_cls_val=2)
    calls = []
    step = TrainableHead.step

    def recording(self, features, target, train):
        r = step(self, features, target, train)
        calls.append((features.detach().cpu().clone(), torch.as_tensor(target).clone(), bool(train), r))
        return r
    monkeypatch.setattr(TrainableHead, "step", recording)
    cfg = _head_train_config(root, "default", epochs=2, save_period=2)
    tr = train.main(copy.deepcopy(cfg), run_id="head")
    train_calls = [c for c in calls if c[2]]
    assert len(train_calls) == 6 and len(calls) == 6 + 2 * 2 and [c[0].shape[0] for c in train_calls] == [5, 5, 2] * 2
    # the kept features: a row's features are the same bits in both epochs
    assert torch.equal(torch.cat([c[0] for c in train_calls[:3]]).sort(dim=0).values, torch.cat([c[0] for c in train_calls[3:]]).sort(dim=0).values)
    init = generate_state_dict("iresnet100", 0, as_torch=True, n_classes=3)
    want = oracle_run(init["logits.weight"], init["logits.bias"], [(c[0], c[1]) for c in train_calls])
    cp = torch.load(str(tr.save_dir / "checkpoint-epoch2.pth"), map_location="cpu", weights_only=True)
    sd = cp["state_dict"]
    _check_against_oracle("train.py, 6 steps", sd["logits.weight"], sd["logits.bias"], [c[3][0] for c in train_calls], want)
    assert [c[3][1] for c in train_calls] == want["hits"] or want["gap"] <= MIN_GAP
    # the checkpoint is the reference's
    assert list(cp) == ref["checkpoint_keys"] and cp["arch"] == ref["arch"] and cp["epoch"] == 2 and cp["config"] == cfg
    assert sorted(cp["optimizer"]["state"]) == ref["state_indices"]
    assert sorted(cp["optimizer"]["param_groups"][0]) == ref["group_keys"]
    assert cp["optimizer"]["param_groups"][0]["params"] == list(range(ref["P"]))
    assert sorted(cp["optimizer"]["state"][ref["state_indices"][0]]) == ref["state_entry_keys"]
    assert float(cp["optimizer"]["state"][ref["state_indices"][1]]["step"]) == 6.0
    assert set(sd) == set(init) and not torch.equal(sd["logits.weight"], init["logits.weight"])
    assert all(torch.equal(torch.as_tensor(sd[k]), torch.as_tensor(init[k])) for k in init if not k.startswith("logits."))
    # eval.py on the same validation set reproduces the trainer's best validation loss from model_best.pth
    ecfg = {k: copy.deepcopy(v) for k, v in cfg.items() if k not in ("train_dataset", "train_data_loader", "optimizer", "lr_scheduler")}
    ecfg["trainer"].update(resume_path=str(tr.save_dir / "model_best.pth"), save_result=True)
    best = torch.load(ecfg["trainer"]["resume_path"], map_location="cpu", weights_only=True)
    assert best["monitor_best"] == tr.mnt_best and best["epoch"] == 2
    et = ev.main(ecfg, run_id="head_eval")
    got = et.val_loss.avg("neg_log_llhood")
    print("eval.py on model_best.pth: val_neg_log_llhood %.9g, the trainer's best %.9g" % (got, tr.mnt_best))
    assert abs(got - tr.mnt_best) <= 1e-5 * abs(tr.mnt_best)
    assert os.path.exists(str(et.save_dir / "result.csv"))


def test_train_py_head_route_facenet_aug_repeats_bitwise(tmp_path):
    sys.path.insert(0, REPO)
    import train
    root = str(tmp_path)
    write_face_dataset(root, size=112, n_cls=3, per_cls_train=4, per_cls_val=2)
    cfg = _head_train_config(root, "facenet_aug", epochs=2, save_period=100)     # no checkpoint is written
    curves = []
    for run in ("a", "b"):
        tr = train.main(copy.deepcopy(cfg), run_id=run)
        curves.append(open(str(tr.log_dir / "log_loss.txt")).read())
        assert not os.path.exists(str(tr.save_dir / "model_best.pth"))
    lines = curves[0].splitlines()
    assert lines[0] == "Epoch,Train_loss,Validation_loss" and len(lines) == 3 and all(np.isfinite(float(v)) for ln in lines[1:] for v in ln.split(","))
    assert curves[0] == curves[1]
