"""Host side of the encoders' classification heads and of eval.py: weight specs, constructor rules, refusals, the
result.csv writer and the target check.  No GPU."""
import copy
import json
import os
import sys

import numpy as np
import pytest
import torch

from conftest import REPO

from vn_celeb_face_recognition_amd import weights as W
from vn_celeb_face_recognition_amd.encoders import InceptionResnetV1, iresnet100


# ------------------------------------------------------------------------------------------ weight specs
def test_irv1_head_spec_leaves_every_other_tensor_bit_identical():
    base = W.generate_state_dict("irv1", 0)
    head = W.generate_state_dict("irv1", 0, num_classes=7)
    assert list(head)[:len(base)] == list(base) and list(head)[len(base):] == ["logits.weight", "logits.bias"]
    for k, v in base.items():
        assert v.dtype == head[k].dtype and v.tobytes() == head[k].tobytes(), k
    assert head["logits.weight"].shape == (7, 512) and head["logits.bias"].shape == (7,)
    assert head["logits.weight"].dtype == np.float32 and np.isfinite(head["logits.weight"]).all()
    # the draw depends on the name and the seed only: another width is another tensor, another seed another draw
    assert W.generate_state_dict("irv1", 1, num_classes=7)["logits.bias"].tobytes() != head["logits.bias"].tobytes()


def test_iresnet_head_spec_leaves_every_other_tensor_bit_identical():
    base = W.iresnet_spec()
    head = W.iresnet_spec(n_classes=1020)
    assert head[:len(base)] == base
    assert head[len(base):] == [("logits.weight", (1020, 512), "linear"), ("logits.bias", (1020,), "bias")]
    # one block per stage is enough (generation is keyed per tensor name, and these are names of the full network too)
    sd0 = W.generate_state_dict("iresnet100", 0, layers=(1, 1, 1, 1))
    sd1 = W.generate_state_dict("iresnet100", 0, layers=(1, 1, 1, 1), n_classes=5)
    assert list(sd1)[:len(sd0)] == list(sd0)
    for k, v in sd0.items():
        assert v.tobytes() == sd1[k].tobytes(), k
    assert "logits.weight" not in sd0 and sd1["logits.weight"].shape == (5, 512)


@pytest.fixture
def no_ir100_draws(monkeypatch):
    """iresnet100() without the two seconds its 65 M generator weights take: these tests look at the wrapper only."""
    from collections import OrderedDict
    from vn_celeb_face_recognition_amd import encoders
    real = encoders.generate_state_dict
    monkeypatch.setattr(encoders, "generate_state_dict",
                        lambda arch, *a, **k: OrderedDict() if arch == "iresnet100" else real(arch, *a, **k))


def test_expected_keys_follow_the_head(no_ir100_draws):
    assert "logits.weight" not in InceptionResnetV1(pretrained=None)._expected_keys()
    m = InceptionResnetV1(pretrained=None, classify=True, num_classes=7)
    assert m._expected_keys()[-2:] == ["logits.weight", "logits.bias"] and m.head_classes == 7
    assert tuple(m.state_dict()["logits.weight"].shape) == (7, 512)
    r = iresnet100(n_classes=9)
    assert r._expected_keys()[-2:] == ["logits.weight", "logits.bias"] and r.head_classes == 9
    assert iresnet100().head_classes is None and "logits.bias" not in iresnet100()._expected_keys()


# ------------------------------------------------------------------------------------------ constructor rules
def test_classify_without_num_classes_raises_the_reference_text():
    with pytest.raises(Exception) as ei:
        InceptionResnetV1(pretrained=None, classify=True, num_classes=None)
    assert str(ei.value) == 'If "pretrained" is not specified and "classify" is True, "num_classes" must be specified'
    assert type(ei.value) is Exception


def test_named_pretrained_file_is_never_downloaded(tmp_path, monkeypatch):
    monkeypatch.setenv("TORCH_HOME", str(tmp_path))
    with pytest.raises(FileNotFoundError, match="vggface2"):
        InceptionResnetV1(pretrained="vggface2", classify=True)


def test_iresnet100_unknown_kwarg_and_freeze_message(capsys, no_ir100_draws):
    with pytest.raises(TypeError, match="bogus"):
        iresnet100(n_classes=4, bogus=1)
    iresnet100(n_classes=4, freeze_weights=True)
    assert capsys.readouterr().out == "Freezing weights !\n"
    iresnet100(freeze_weights=True)      # no head: as before, nothing is printed
    assert capsys.readouterr().out == ""


def _partial_file(tmp_path, with_logits):
    g = torch.Generator().manual_seed(3)
    sd = {"last_bn.weight": torch.ones(512)}
    if with_logits:
        sd["logits.weight"] = torch.randn((31, 512), generator=g)
        sd["logits.bias"] = torch.randn((31,), generator=g)
    path = str(tmp_path / ("head31.pt" if with_logits else "nohead.pt"))
    torch.save(sd, path)
    return path, sd


def test_head_comes_from_the_file_when_num_classes_is_not_given(tmp_path):
    path, sd = _partial_file(tmp_path, True)
    m = InceptionResnetV1(pretrained=path, classify=True)
    assert m.head_classes == 31 and m.num_classes is None
    assert torch.equal(m.state_dict()["logits.weight"], sd["logits.weight"])
    # num_classes given: a fresh, generator-seeded head replaces the file's (inception_resnet_v1.py:264-265)
    m5 = InceptionResnetV1(pretrained=path, classify=True, num_classes=5)
    assert m5.head_classes == 5 and tuple(m5.state_dict()["logits.weight"].shape) == (5, 512)
    want = W.generate_state_dict("irv1", 0, num_classes=5)["logits.weight"]
    assert np.array_equal(np.asarray(m5.state_dict()["logits.weight"]), want)
    # classify=False: the file's logits are carried along and build no head
    assert InceptionResnetV1(pretrained=path).head_classes is None
    # a later load_state_dict replaces the head; another width is a size mismatch
    new = dict(m5.state_dict())
    new["logits.weight"] = torch.zeros((5, 512))
    m5.load_state_dict(new, strict=False)
    assert float(m5.state_dict()["logits.weight"].abs().sum()) == 0.0
    with pytest.raises(RuntimeError, match="size mismatch for logits.weight"):
        m5.load_state_dict({"logits.weight": torch.zeros((6, 512)), "logits.bias": torch.zeros(6)}, strict=False)


def test_file_without_logits_cannot_classify(tmp_path):
    path, _ = _partial_file(tmp_path, False)
    with pytest.raises(RuntimeError, match="logits"):
        InceptionResnetV1(pretrained=path, classify=True)


def test_headed_models_have_no_cpu_path(no_ir100_draws):
    x = torch.zeros((1, 3, 160, 160))
    m = InceptionResnetV1(pretrained=None, classify=True, num_classes=7)
    with pytest.raises(RuntimeError, match="MI355X only"):
        m(x)
    with pytest.raises(RuntimeError, match="MI355X only"):
        m.logprobs(x)
    with pytest.raises(RuntimeError, match="MI355X only"):
        iresnet100(n_classes=7)(torch.zeros((1, 3, 112, 112)))
    with pytest.raises(RuntimeError, match="without a classification head"):
        InceptionResnetV1(pretrained=None).logprobs(x)


# ------------------------------------------------------------------------------------------ eval.py refusals
def _cfg(kind):
    name = {"emb": "train_cfg_emb_classify.json", "aug": "train_cfg_aug_emb_classify.json", "img": "eval_cfg_img_classify.json"}[kind]
    with open(os.path.join(REPO, "cfg", name)) as f:
        cfg = json.load(f)
    if kind != "img":
        cfg["trainer"]["resume_path"] = "saved/models/x/model_best.pth"
    return cfg


def _plan(cfg):
    sys.path.insert(0, REPO)
    import eval as ev
    return ev.plan(cfg)


def test_eval_accepts_the_three_shipped_configurations():
    assert [_plan(_cfg(k)) for k in ("emb", "aug", "img")] == ["emb", "aug", "img"]
    cfg = _cfg("img")
    cfg["model"] = copy.deepcopy(cfg["model"]["some_models"][1])
    assert cfg["model"]["name"] == "iresnet100" and _plan(cfg) == "img"


@pytest.mark.parametrize("kind,edit,word", [
    ("emb", lambda c: c["model"].update(name="resnet101"), "resnet101"),
    ("emb", lambda c: c["trainer"].update(name="TripletTrainer"), "TripletTrainer"),
    ("emb", lambda c: c["val_dataset"].update(name="VNCelebTestDataset"), "VNCelebTestDataset"),
    ("emb", lambda c: c.update(loss="cross_entropy"), "cross_entropy"),
    ("emb", lambda c: c.update(metrics=["accuracy", "top5"]), "top5"),
    ("emb", lambda c: c["trainer"].update(device="CPU"), "no CPU path"),
    ("emb", lambda c: c["trainer"].update(resume_path=""), "resume_path"),
    ("emb", lambda c: c["val_dataset"].update(name="VNCelebDataset"), "VNCelebDataset / ClassificationTrainer"),
    ("emb", lambda c: c["trainer"].update(name="AugClassificationTrainer"), "VNCelebEmbDataset / AugClassificationTrainer"),
    ("aug", lambda c: c["transforms"].update(resize=True), "transforms.resize"),
    ("aug", lambda c: c["transforms"].update(name="rank1_aug"), "rank1_aug"),
    ("aug", lambda c: c["trainer"].update(chosen_idx_enc=7), "chosen_idx_enc"),
    ("img", lambda c: c["val_dataset"].update(name="VNCelebEmbDataset"), "InceptionResnetV1 classifies face images"),
    ("img", lambda c: c["trainer"].update(name="AugClassificationTrainer"), "AugClassificationTrainer"),
    ("img", lambda c: c["model"]["args"].update(classify=False), "without classify"),
    ("img", lambda c: c.update(model={"name": "iresnet100", "args": {}}), "without n_classes"),
    ("img", lambda c: c["transforms"].update(resize=True), "transforms.resize"),
])
def test_eval_refuses_by_name(kind, edit, word):
    cfg = _cfg(kind)
    edit(cfg)
    with pytest.raises(SystemExit) as ei:
        _plan(cfg)
    assert word in str(ei.value), str(ei.value)


def test_train_py_still_refuses_the_image_classifier():
    sys.path.insert(0, REPO)
    import train
    with pytest.raises(SystemExit, match="MLPModel"):
        train.main(_cfg("img") | {"train_dataset": {"name": "VNCelebDataset", "args": {}}})


# ------------------------------------------------------------------------------------------ result.csv and targets
def test_result_csv_header_order_and_path_form(tmp_path):
    from vn_celeb_face_recognition_amd.trainer import VNCelebEmbDataset, write_result_csv
    labels = {"3": ["b.png", "a.jpg"], "0": ["c, d.png"]}
    (tmp_path / "val.json").write_text(json.dumps(labels))
    ds = VNCelebEmbDataset(str(tmp_path / "emb"), str(tmp_path / "val.json"))
    for name in ds.img_names:
        os.makedirs(str(tmp_path / "emb"), exist_ok=True)
        np.savez_compressed(str(tmp_path / "emb" / (name.split(".")[0] + ".npz")), np.zeros(4, np.float32))
    items = [ds[i] for i in range(len(ds))]
    assert [it[2] for it in items] == [str(tmp_path / "emb" / n) for n in ("a.npz", "b.npz", "c, d.npz")]
    rows = [(it[2], np.int64(it[1]), np.int32(p), float(np.float32(q))) for it, p, q in zip(items, (3, 1, 0), (0.25, 0.1, 1.0))]
    out = str(tmp_path / "result.csv")
    write_result_csv(iter(rows), out)
    text = open(out, newline="").read()
    assert "\r" not in text
    lines = text.split("\n")
    assert lines[0] == "Path,Target,Prediction,Probability" and lines[-1] == "" and len(lines) == 5
    assert lines[1] == "%s,3,3,0.25" % (tmp_path / "emb" / "a.npz")
    assert lines[2] == "%s,3,1,%s" % (tmp_path / "emb" / "b.npz", repr(float(np.float32(0.1))))
    assert lines[3] == '"%s",0,0,1.0' % (tmp_path / "emb" / "c, d.npz")     # minimal quoting, as DataFrame.to_csv


def test_targets_are_checked_on_the_host():
    from vn_celeb_face_recognition_amd.classifier import check_targets, logits_eval
    t = check_targets([0, 6, 3], 7)
    assert t.dtype == torch.int64 and t.device.type == "cpu" and t.tolist() == [0, 6, 3]
    assert check_targets(torch.tensor([2], dtype=torch.int32), 3).dtype == torch.int64
    assert check_targets([], 3).dtype == torch.int64 and check_targets([], 3).numel() == 0
    with pytest.raises(IndexError, match="Target 7 is out of bounds"):
        check_targets([0, 7], 7)
    with pytest.raises(IndexError, match="Target -1 is out of bounds"):
        check_targets(torch.tensor([3, -1]), 7)
    with pytest.raises(TypeError):
        check_targets(torch.tensor([0.5]), 7)
    with pytest.raises(RuntimeError, match="MI355X only"):
        logits_eval(torch.zeros((2, 3)), [0, 1])


def test_eval_model_has_no_cpu_path():
    from vn_celeb_face_recognition_amd.classifier import MLPModel
    from vn_celeb_face_recognition_amd.trainer import EvalModel
    with pytest.raises(RuntimeError, match="MI355X only"):
        EvalModel(MLPModel(512, 12), 12, device="cpu")
