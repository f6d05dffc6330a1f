"""Host side of head training: train.py's third route and what it refuses, and the optimizer layout of
trainer.TrainableHead against the reference's own (tests/golden/head_train_ref.json, tools/make_head_train_golden.py)."""
import copy
import json
import os
import sys

import pytest
import torch

from conftest import GOLDEN, REPO


def _shipped():
    with open(os.path.join(REPO, "cfg", "train_cfg_img_classify.json")) as f:
        return json.load(f)


def _train():
    sys.path.insert(0, REPO)
    import train
    return train


def test_shipped_config_takes_the_head_route(monkeypatch):
    train = _train()
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    cfg = _shipped()
    frozen = [m for m in cfg["model"]["some_models"] if m["args"].get("freeze_weights")]
    assert cfg["model"]["name"] == "iresnet100" and cfg["transforms"]["name"] == "facenet_aug" and len(frozen) >= 1
    assert {m["name"] for m in frozen} >= {"InceptionResnetV1"}
    assert cfg["optimizer"] == {"name": "Adam", "args": {"lr": 0.001, "weight_decay": 1e-04}}
    for model in [cfg["model"]] + frozen:
        c = copy.deepcopy(cfg)
        c["model"] = copy.deepcopy(model)
        assert train.head_config(c) is True
        with pytest.raises(SystemExit, match="no GPU is visible"):     # past every check up to the one for a GPU
            train.main(c)
    # the other two shipped configurations do not take it
    for name in ("train_cfg_emb_classify.json", "train_cfg_aug_emb_classify.json"):
        with open(os.path.join(REPO, "cfg", name)) as f:
            assert train.head_config(json.load(f)) is False


@pytest.mark.parametrize("edit,word", [
    (lambda c: c["transforms"].update(name="rank1_aug"), "rank1_aug"),
    (lambda c: c["transforms"].update(resize=True), "resize"),
    (lambda c: c["transforms"].update(name="emotion_inf"), "default or facenet_aug"),
    (lambda c: c["optimizer"].update(name="SGD"), "Adam"),
    (lambda c: c["lr_scheduler"].update(name="MultiStepLR"), "ReduceLROnPlateau"),
    (lambda c: c["trainer"].update(device="CPU"), "trainer.device must be GPU"),
    (lambda c: c.update(model={"name": "InceptionResnetV1", "args": {"pretrained": None, "classify": True, "num_classes": 5}}), "MLPModel"),
    (lambda c: c["model"]["args"].update(freeze_weights=False), "MLPModel"),
    (lambda c: c["model"]["args"].pop("n_classes"), "MLPModel"),
    (lambda c: c["trainer"].update(name="AugClassificationTrainer"), "MLPModel"),
    (lambda c: c["val_dataset"].update(name="VNCelebEmbDataset"), "MLPModel"),
])
def test_train_py_refuses_by_name(monkeypatch, edit, word):
    train = _train()
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    cfg = _shipped()
    edit(cfg)
    with pytest.raises(SystemExit) as ei:
        train.main(cfg)
    assert word in str(ei.value), str(ei.value)


def test_optimizer_layout_is_the_reference_s():
    from vn_celeb_face_recognition_amd import models
    from vn_celeb_face_recognition_amd.trainer import HEAD_PARAMS, head_param_layout
    from vn_celeb_face_recognition_amd.weights import iresnet_spec
    with open(os.path.join(GOLDEN, "head_train_ref.json")) as f:
        ref = json.load(f)
    assert ref["params_are_range"] and ref["state_names"] == list(HEAD_PARAMS)
    P, iw, ib = head_param_layout(iresnet_spec(n_classes=12))
    assert P == ref["P"] and [iw, ib] == ref["state_indices"]
    assert len(iresnet_spec(n_classes=12)) == ref["n_state_dict_keys"]
    # the width of the head does not move the indices
    assert head_param_layout(iresnet_spec(n_classes=1020)) == (P, iw, ib)
    enc = models.iresnet100(n_classes=12, freeze_weights=True)
    assert enc.arch_name == ref["type_name"] == ref["arch"] == "IResNet" and enc.freeze_weights is True
    assert models.InceptionResnetV1(pretrained=None, classify=True, num_classes=5, freeze_weights=True).arch_name == "InceptionResnetV1"
    # what TrainableHead writes for a state entry and for the group: torch's own Adam names
    group = torch.optim.Adam([torch.zeros(1)], lr=1e-3, weight_decay=1e-4).state_dict()["param_groups"][0]
    assert sorted(group) == ref["group_keys"]
    assert ref["state_entry_keys"] == ["exp_avg", "exp_avg_sq", "step"]
    assert ref["checkpoint_keys"] == ["arch", "epoch", "state_dict", "optimizer", "monitor_best", "config"]


def test_trainable_head_has_no_cpu_path():
    from vn_celeb_face_recognition_amd import models
    from vn_celeb_face_recognition_amd.trainer import TrainableHead
    with pytest.raises(RuntimeError, match="MI355X only"):
        TrainableHead(models.iresnet100(n_classes=3, freeze_weights=True))
    with pytest.raises(RuntimeError, match="without a classification head"):
        TrainableHead(models.iresnet100())
