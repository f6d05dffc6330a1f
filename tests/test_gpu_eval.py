"""GPU: eval.py as a command, in its three configurations: (a) MLPModel on embeddings against the reference trainer's own
eval(save_result=True) (tools/make_heads_golden.py eval), (b) MLPModel behind a frozen encoder on face images, (c) an
encoder with its own logits head."""
import csv
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, REPO, load_image

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _run_eval(cfg, cwd, tag="cfg"):
    """python eval.py -c <cfg> -d GPU in `cwd` -> (the logged figures, the csv path or None, the csv bytes or None)."""
    path = os.path.join(str(cwd), tag + ".json")
    with open(path, "w") as f:
        json.dump(cfg, f)
    r = subprocess.run([sys.executable, os.path.join(REPO, "eval.py"), "-c", path, "-d", "GPU"], cwd=str(cwd),
                       env=dict(os.environ, PYTHONPATH=REPO), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    log = {k: float(v) for k, v in re.findall(r"^INFO:trainer:    (val_\w+)\s*: (\S+)$", r.stderr, flags=re.M)}
    assert set(log) == {"val_neg_log_llhood", "val_accuracy"}, r.stderr
    assert re.search(r"^INFO:trainer:    val_neg_log_llhood: ", r.stderr, flags=re.M)       # '    {:15s}: {}'
    assert re.search(r"^INFO:trainer:    val_accuracy   : ", r.stderr, flags=re.M)
    m = re.search(r"^Saved prediction to (.*)\.$", r.stdout, flags=re.M)
    if not m:
        return log, None, None
    return log, m.group(1), open(m.group(1), "rb").read()


def _rows(data):
    rows = list(csv.reader(data.decode().splitlines()))
    assert rows[0] == ["Path", "Target", "Prediction", "Probability"]
    return [(p, int(t), int(a), float(q)) for p, t, a, q in rows[1:]]


def _mlp_checkpoint(path, seed, input_dim, num_classes):
    from vn_celeb_face_recognition_amd.weights import generate_state_dict
    sd = generate_state_dict("mlp", seed, as_torch=True, input_dim=input_dim, num_classes=num_classes)
    torch.save({"arch": "MLPModel", "epoch": 3, "state_dict": sd, "optimizer": {"state": {}, "param_groups": [{"lr": 1e-3}]},
                "monitor_best": 1.0}, path)
    return sd


# ------------------------------------------------------------------------------------------------ (a)
def test_eval_mlp_on_embeddings_matches_the_reference_trainer(tmp_path):
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import make_golden
    ref = json.load(open(os.path.join(GOLDEN, "eval_ref.json")))
    cfg = make_golden.write_mlp_train_case(str(tmp_path))
    cfg["trainer"].update(device="GPU", save_result=True, resume_path=str(tmp_path / "model_best.pth"))
    assert cfg["val_data_loader"]["args"]["batch_size"] == ref["batch_size"]
    _mlp_checkpoint(cfg["trainer"]["resume_path"], ref["mlp_seed"], **cfg["model"]["args"])
    log, path, data = _run_eval(cfg, tmp_path)
    assert os.path.dirname(path).startswith(os.path.join(cfg["trainer"]["save_dir"], "models")) and os.path.basename(path) == "result.csv"
    assert data.decode().splitlines()[0] == ref["header"] and b"\r" not in data
    got = _rows(data)
    emb_dir = cfg["val_dataset"]["args"]["data_dir"]
    assert [(p, t, a) for p, t, a, _ in got] == [(os.path.join(emb_dir, n), t, a) for n, t, a, _ in ref["rows"]]
    perr = max(abs(g[3] - r[3]) for g, r in zip(got, ref["rows"]))
    print("eval (a): loss %.9g (reference %.9g), accuracy %.6f, max probability error %.3e"
          % (log["val_neg_log_llhood"], ref["val_neg_log_llhood"], log["val_accuracy"], perr))
    assert perr <= 1e-4
    assert abs(log["val_neg_log_llhood"] - ref["val_neg_log_llhood"]) <= 1e-4
    assert log["val_accuracy"] == ref["val_accuracy"] and 0 < ref["val_accuracy"] < 1
    # save_result false: the same figures, no file
    cfg["trainer"]["save_result"] = False
    log2, path2, _ = _run_eval(cfg, tmp_path, "nosave")
    assert path2 is None and log2 == log


# ------------------------------------------------------------------------------------------------ (b), (c)
NAMES = {"0": ["f2.png", "f0.png"], "6": ["f1.png"], "1": ["f5.png", "f3.png", "f4.png"]}


def _face_case(tmp_path):
    """Six 160x160 cuts of one of the golden pictures as a VNCelebDataset directory; returns (dir, label file, the faces
    (6,160,160,3) u8 and their labels in the data set's order: classes in file order, names sorted inside a class)."""
    from PIL import Image
    img = load_image("mrDam_HaHo_recog.jpg")
    d = tmp_path / "faces"
    d.mkdir()
    for i in range(6):
        y, x = 20 + 37 * i, 40 + 61 * i
        Image.fromarray(np.ascontiguousarray(img[y:y + 160, x:x + 160])).save(str(d / ("f%d.png" % i)))
    lab = tmp_path / "val.json"
    lab.write_text(json.dumps(NAMES))
    order, labels = [], []
    for k, v in NAMES.items():
        order += sorted(v)
        labels += [int(k)] * len(v)
    faces = np.stack([np.asarray(Image.open(str(d / n)).convert("RGB")) for n in order])
    assert faces.shape == (6, 160, 160, 3)
    return str(d), str(lab), order, faces, labels


def _base_cfg(data_dir, label_file, save_dir, batch_size):
    return {"val_dataset": {"name": "VNCelebDataset", "args": {"data_dir": data_dir, "label_file": label_file}},
            "val_data_loader": {"name": "val", "args": {"batch_size": batch_size, "shuffle": False, "num_workers": 0}},
            "transforms": {"name": "default", "resize": False, "encoder_img_size": 160}, "metrics": ["accuracy"],
            "loss": "neg_log_llhood",
            "trainer": {"name": "ClassificationTrainer", "resume_path": "", "save_dir": save_dir, "device": "GPU", "log_step": 30,
                        "do_validation": True, "validation_step": 1, "epochs": 1, "tracked_metric": ["val_neg_log_llhood", "min"],
                        "patience": 10, "save_period": 1, "save_result": True, "track4plot": False}}


def _default(faces):
    return torch.from_numpy(((np.float32(faces) - 127.5) / 128).transpose(0, 3, 1, 2).copy()).to(DEV)


def test_eval_mlp_behind_a_frozen_encoder(tmp_path):
    from vn_celeb_face_recognition_amd import models
    data_dir, label_file, order, faces, labels = _face_case(tmp_path)
    cfg = _base_cfg(data_dir, label_file, str(tmp_path / "saved"), 4)
    cfg["model"] = {"name": "MLPModel", "args": {"input_dim": 512, "num_classes": 7}}
    cfg["trainer"].update(name="AugClassificationTrainer", chosen_idx_enc=0, resume_path=str(tmp_path / "mlp.pth"),
                          encoders=[{"name": "InceptionResnetV1", "args": {"pretrained": None, "max_batch": 8}}])
    sd = _mlp_checkpoint(cfg["trainer"]["resume_path"], 4, 512, 7)
    log, path, data = _run_eval(cfg, tmp_path)
    got = _rows(data)
    enc = models.InceptionResnetV1(pretrained=None, max_batch=8).to(DEV).eval()
    clf = models.MLPModel(512, 7, max_batch=8).to(DEV).eval()
    clf.load_state_dict(sd)
    logp, amax, prob = clf.classify(enc(_default(faces)))
    assert [p for p, _, _, _ in got] == [os.path.join(data_dir, n) for n in order]
    assert [t for _, t, _, _ in got] == labels
    assert [a for _, _, a, _ in got] == amax.tolist()
    # the evaluation takes exp(logp[argmax]) of the renormalised row: fp32 rounding of a value <= 1
    assert np.abs(np.array([q for _, _, _, q in got]) - prob.cpu().numpy()).max() <= 1e-6
    t = torch.tensor(labels, device=DEV)
    nll = -logp[torch.arange(6, device=DEV), t].double().cpu().numpy()
    want_loss = (nll[:4].mean() + nll[4:].mean()) / 2             # mean of the batch means (4 + 2 rows)
    print("eval (b): loss %.9g (direct %.9g), accuracy %.6f" % (log["val_neg_log_llhood"], want_loss, log["val_accuracy"]))
    assert abs(log["val_neg_log_llhood"] - want_loss) <= 1e-5 * max(1.0, want_loss)
    assert log["val_accuracy"] == float((amax.long() == t).sum()) / 6


def test_eval_encoder_with_its_own_head(tmp_path):
    from vn_celeb_face_recognition_amd import models
    data_dir, label_file, order, faces, labels = _face_case(tmp_path)
    cfg = _base_cfg(data_dir, label_file, str(tmp_path / "saved"), 4)
    cfg["model"] = {"name": "InceptionResnetV1", "args": {"pretrained": None, "classify": True, "num_classes": 7, "max_batch": 4}}
    log, path, data = _run_eval(cfg, tmp_path)
    model = models.InceptionResnetV1(pretrained=None, classify=True, num_classes=7, max_batch=4).to(DEV).eval()
    logp = model(_default(faces))
    t = torch.tensor(labels, device=DEV)
    nll = -logp[torch.arange(6, device=DEV), t].double().cpu().numpy()
    want_loss = (nll[:4].mean() + nll[4:].mean()) / 2             # mean of the batch means (4 + 2 rows)
    # eval.py scores the model's log-probabilities with vnf_logits_eval, whose log_softmax of a row that already sums to
    # one moves it by |log sum exp(logp)| <= a few 2^-24, and takes the batch mean in fp32: 1e-5 relative covers both
    print("eval (c): loss %.9g (direct %.9g), accuracy %.6f" % (log["val_neg_log_llhood"], want_loss, log["val_accuracy"]))
    assert abs(log["val_neg_log_llhood"] - want_loss) <= 1e-5 * max(1.0, want_loss)
    got = _rows(data)
    assert [p for p, _, _, _ in got] == [os.path.join(data_dir, n) for n in order] and [t_ for _, t_, _, _ in got] == labels
    assert [a for _, _, a, _ in got] == logp.argmax(dim=1).tolist()
    assert log["val_accuracy"] == float((logp.argmax(dim=1) == t).sum()) / 6
    # a second run writes the same bytes
    log2, path2, data2 = _run_eval(cfg, tmp_path, "again")
    assert data2 == data and log2 == log
