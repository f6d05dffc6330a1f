"""GPU: vnf_augment_faces against the Pillow-made golden file (byte for byte), its normalised outputs, its argument
checks, and AugClassificationTrainer against ClassificationTrainer on the same embeddings."""
import copy
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from aug_golden import aug_train_config, load_cases, write_face_dataset
from conftest import REPO
from vn_celeb_face_recognition_amd import _lib
from vn_celeb_face_recognition_amd import augment as A

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _groups():
    """The golden cases grouped by (S, T): faces (k,S,S,3), params, expected (k,T,T,3)."""
    out = {}
    for face, s, t, angle, i, j, flip, want in load_cases():
        out.setdefault((s, t), []).append((face, angle, i, j, flip, want))
    for (s, t), rows in out.items():
        faces = np.stack([r[0] for r in rows])
        params = A.make_params([r[1] for r in rows], [r[2] for r in rows], [r[3] for r in rows], [r[4] for r in rows], s, t)
        yield s, t, faces, params, np.stack([r[5] for r in rows])


def test_u8_out_equals_the_golden_with_zero_differing_bytes():
    seen = 0
    for s, t, faces, params, want in _groups():
        fdev = torch.from_numpy(faces).to(DEV)
        for dtype in (torch.float32, torch.bfloat16):
            x, u8 = A.augment_faces_device(fdev, None, params, t, dtype=dtype, want_u8=True)
            diff = int((u8.cpu().numpy() != want).sum())
            print("S=%d T=%d %s: %d differing bytes of %d" % (s, t, dtype, diff, want.size))
            assert diff == 0
        # through a shuffled index with repeats: row r of the output is face index[r] under params[r]
        k = len(faces)
        index = np.array([(3 * r + 1) % k for r in range(2 * k + 1)], np.int32)
        x, u8 = A.augment_faces_device(fdev, index, params[index], t, want_u8=True)
        diff = int((u8.cpu().numpy() != want[index]).sum())
        print("S=%d T=%d shuffled index %s: %d differing bytes" % (s, t, index.tolist(), diff))
        assert diff == 0
        # u8_out alone (x_out NULL is allowed by the ABI)
        u8b = torch.empty((k, t, t, 3), dtype=torch.uint8, device=DEV)
        pdev = torch.from_numpy(params.view(np.uint8).reshape(-1).copy()).to(DEV)
        _lib.check(_lib.load().vnf_augment_faces(ctypes.c_void_p(fdev.data_ptr()), k, s, None, ctypes.c_void_p(pdev.data_ptr()), k, t,
                                                 None, _lib.VNF_F32, ctypes.c_void_p(u8b.data_ptr()), _lib.current_stream_ptr()))
        assert int((u8b.cpu().numpy() != want).sum()) == 0
        seen += k
    assert seen == 8


def test_x_out_is_the_normalised_bytes_in_each_dtype():
    for s, t, faces, params, want in _groups():
        fdev = torch.from_numpy(faces).to(DEV)
        ref = torch.from_numpy(A.normalise(want))                   # (u8 - 127.5) / 128 in fp32, CHW
        x = A.augment_faces_device(fdev, None, params, t, dtype=torch.float32)
        assert x.shape == (len(faces), 3, t, t) and x.dtype == torch.float32
        assert torch.equal(x.cpu(), ref)
        for dtype in (torch.float16, torch.bfloat16):
            x = A.augment_faces_device(fdev, None, params, t, dtype=dtype)
            assert x.dtype == dtype and torch.equal(x.cpu(), ref.to(dtype))      # torch's cast rounds to nearest even


def test_odd_target_size_takes_the_unvectorised_stores():
    """T not a multiple of the kernel's 4-pixel groups: the tail of every row is written pixel by pixel."""
    face = load_cases()[0][0][:37, :37]
    s, t = 37, 50
    p = A.crop_padding(s, t)
    hi = s + 2 * p - t
    params = A.make_params([-6.25, 3.5], [1, hi], [hi, 0], [1, 0], s, t)
    want = np.stack([A.pillow_facenet_aug(face, -6.25, 1, hi, 1, t), A.pillow_facenet_aug(face, 3.5, hi, 0, 0, t)])
    fdev = torch.from_numpy(np.ascontiguousarray(face)[None]).to(DEV)
    for dtype in (torch.float32, torch.float16):
        x, u8 = A.augment_faces_device(fdev, [0, 0], params, t, dtype=dtype, want_u8=True)
        assert int((u8.cpu().numpy() != want).sum()) == 0
        assert torch.equal(x.cpu(), torch.from_numpy(A.normalise(want)).to(dtype))


def test_empty_batch_and_bad_arguments():
    lib = _lib.load()
    s = t = 160
    fdev = torch.zeros((2, s, s, 3), dtype=torch.uint8, device=DEV)
    params = A.identity_params(2, s, t)
    pdev = torch.from_numpy(params.view(np.uint8).reshape(-1).copy()).to(DEV)
    x = torch.full((2, 3, t, t), 7.0, device=DEV)

    def call(faces=fdev, n_faces=2, s_=s, index=None, prm=pdev, n=2, t_=t, out=x, dt=_lib.VNF_F32):
        return lib.vnf_augment_faces(ctypes.c_void_p(faces.data_ptr()) if faces is not None else None, n_faces, s_,
                                     ctypes.c_void_p(index.data_ptr()) if index is not None else None,
                                     ctypes.c_void_p(prm.data_ptr()) if prm is not None else None, n, t_,
                                     ctypes.c_void_p(out.data_ptr()), dt, None, _lib.current_stream_ptr())
    assert call(n=0) == 0 and call(n=0, prm=None, faces=None) == 0          # n == 0: a no-op
    torch.cuda.synchronize()
    assert float(x.min()) == 7.0 and float(x.max()) == 7.0
    E = -1                                                                # VNF_E_INVALID
    assert call(s_=0) == E and call(s_=1025) == E and call(t_=0) == E and call(t_=4096) == E
    assert call(prm=None) == E and call(faces=None) == E and call(n=-1) == E
    assert call(dt=_lib.VNF_F16X2) == E and call(dt=_lib.VNF_U8) == E
    assert call(n=1) == E                                                 # no index: one parameter set per face
    assert b"parameter set" in lib.vnf_last_error()
    assert call() == 0
    torch.cuda.synchronize()
    assert float(x.min()) == float(x.max()) == float((np.float32(0) - np.float32(127.5)) / np.float32(128))
    assert A.augment_faces_device(fdev, torch.zeros(0, dtype=torch.int32), params[:0], t).shape == (0, 3, t, t)
    # the per-sample values: the host layer refuses a crop outside the padded image ...
    bad = params.copy()
    bad["i"][1] = 5
    with pytest.raises(ValueError, match="outside"):
        A.augment_faces_device(fdev, None, bad, t)
    with pytest.raises(ValueError, match="index has"):
        A.augment_faces_device(fdev, [0], params, t)
    # ... and the kernel, which alone can see device memory, writes such a row (or a row whose index is outside the
    # data set) as the fill without reading anything
    faces = torch.full((2, s, s, 3), 200, dtype=torch.uint8, device=DEV)
    raw = torch.from_numpy(bad.view(np.uint8).reshape(-1).copy()).to(DEV)
    x, u8 = A.augment_faces_device(faces, None, raw, t, want_u8=True)
    assert int(u8[0].min()) == 200 and int(u8[1].max()) == 0
    ok = torch.from_numpy(params.view(np.uint8).reshape(-1).copy()).to(DEV)
    x, u8 = A.augment_faces_device(faces, torch.tensor([1, 2], dtype=torch.int32), ok, t, want_u8=True)
    assert int(u8[0].min()) == 200 and int(u8[1].max()) == 0


# ---------------------------------------------------------------- trainer

def _run_main(cfg, run_id, trainer_cls_name, record=None):
    """train.main with the epoch logs, the learning rate after every epoch and (record) every _batch_input recorded."""
    import train
    from vn_celeb_face_recognition_amd import trainer as T
    cls = getattr(T, trainer_cls_name)
    lrs, logs = [], []
    orig_epoch = T.ClassificationTrainer._train_epoch
    orig_input = cls._batch_input

    def epoch(self, e):
        r = orig_epoch(self, e)
        lrs.append(self.model.lr)
        logs.append(r)
        return r

    def batch_input(self, data, train):
        out = orig_input(self, data, train)
        if record is not None:
            record.append((train, data.clone(), out.clone()))
        return out
    T.ClassificationTrainer._train_epoch = epoch
    cls._batch_input = batch_input
    try:
        tr = train.main(copy.deepcopy(cfg), run_id=run_id)
    finally:
        T.ClassificationTrainer._train_epoch = orig_epoch
        cls._batch_input = orig_input
    return tr, logs, lrs


def _encoder():
    from vn_celeb_face_recognition_amd import models
    return models.InceptionResnetV1(pretrained=None, max_batch=32).to(DEV).eval()


def test_default_transform_trains_exactly_like_the_embedding_trainer(tmp_path):
    """transforms default: the loop is image -> normalise (the kernel with identity parameters) -> encoder -> MLP step.
    The embeddings it feeds equal the encoder's output on the same faces, and the whole run equals ClassificationTrainer
    on those embeddings saved as .npz -- bitwise, the encoder being batch-invariant: a face embeds to the
    same bits in a shuffled batch of 16 and in the bulk pass that writes the .npz files."""
    from vn_celeb_face_recognition_amd.trainer import VNCelebDataset
    root = str(tmp_path)
    write_face_dataset(root)
    cfg = aug_train_config(root, transforms="default", epochs=4)
    rec = []
    tr, logs, lrs = _run_main(cfg, "aug", "AugClassificationTrainer", record=rec)
    ds_t = VNCelebDataset(**cfg["train_dataset"]["args"])
    ds_v = VNCelebDataset(**cfg["val_dataset"]["args"])
    assert len(ds_t) == 48 and len(ds_v) == 24 and ds_t.size == 160
    enc = _encoder()
    os.makedirs(os.path.join(root, "emb"))
    emb = {}
    for ds in (ds_t, ds_v):
        e = enc(torch.from_numpy(A.normalise(ds.faces)).to(DEV)).cpu()
        for k, name in enumerate(ds.img_names):
            emb[(ds is ds_t, k)] = e[k]
            np.savez_compressed(os.path.join(root, "emb", name.split(".")[0] + ".npz"), e[k].numpy())
    # what the MLP step was fed
    n_train = 0
    for train_flag, idx, fed in rec:
        assert fed.is_cuda and fed.dtype == torch.float32 and fed.shape == (len(idx), 512)
        want = torch.stack([emb[(train_flag, int(k))] for k in idx])
        assert torch.equal(fed.cpu(), want)
        n_train += int(train_flag)
    assert n_train == 4 * 3
    # the same run on the saved embeddings
    cfg_e = copy.deepcopy(cfg)
    for k in ("train_dataset", "val_dataset"):
        cfg_e[k]["name"] = "VNCelebEmbDataset"
        cfg_e[k]["args"]["data_dir"] = os.path.join(root, "emb")
    cfg_e["transforms"] = "none"
    cfg_e["trainer"]["name"] = "ClassificationTrainer"
    tr_e, logs_e, lrs_e = _run_main(cfg_e, "emb", "ClassificationTrainer")
    print("aug  :", [l["neg_log_llhood"] for l in logs], [l["val_neg_log_llhood"] for l in logs], lrs)
    print("emb  :", [l["neg_log_llhood"] for l in logs_e], [l["val_neg_log_llhood"] for l in logs_e], lrs_e)
    assert logs == logs_e and lrs == lrs_e and len(logs) == 4
    sd, sd_e = tr.model.state_dict(), tr_e.model.state_dict()
    for k in sd:
        assert torch.equal(sd[k], sd_e[k]), k
    assert sorted(os.listdir(tr.save_dir)) == sorted(os.listdir(tr_e.save_dir))
    cp = torch.load(os.path.join(str(tr.save_dir), "checkpoint-epoch4.pth"), weights_only=True)
    cp_e = torch.load(os.path.join(str(tr_e.save_dir), "checkpoint-epoch4.pth"), weights_only=True)
    assert sorted(cp.keys()) == sorted(cp_e.keys()) and cp["arch"] == "MLPModel" and cp["monitor_best"] == cp_e["monitor_best"]
    assert cp["config"]["trainer"]["name"] == "AugClassificationTrainer"


def test_default_transform_refuses_faces_of_another_size(tmp_path):
    root = str(tmp_path)
    write_face_dataset(root, size=150, n_cls=2, per_cls_train=2, per_cls_val=1)
    cfg = aug_train_config(root, transforms="default", epochs=1, n_cls=2)
    with pytest.raises(ValueError, match="does not resize"):
        _run_main(cfg, "x", "AugClassificationTrainer")


def test_facenet_aug_training_is_reproducible_and_follows_the_specification(tmp_path, monkeypatch):
    from vn_celeb_face_recognition_amd.trainer import VNCelebDataset
    root = str(tmp_path)
    write_face_dataset(root)
    cfg = aug_train_config(root, transforms="facenet_aug", epochs=3)
    draws = []
    orig = A.draw_facenet_aug_params

    def spy(n, s, t):
        params, angles = orig(n, s, t)
        draws.append((params.copy(), angles.copy()))
        return params, angles
    monkeypatch.setattr(A, "draw_facenet_aug_params", spy)
    rec = []
    tr1, logs1, lrs1 = _run_main(cfg, "r1", "AugClassificationTrainer", record=rec)
    first_draws = list(draws)
    tr2, logs2, lrs2 = _run_main(cfg, "r2", "AugClassificationTrainer")
    print("run 1:", [l["neg_log_llhood"] for l in logs1], lrs1)
    print("run 2:", [l["neg_log_llhood"] for l in logs2], lrs2)
    assert logs1 == logs2 and lrs1 == lrs2 and len(logs1) == 3
    sd1, sd2 = tr1.model.state_dict(), tr2.model.state_dict()
    for k in sd1:
        assert torch.equal(sd1[k], sd2[k]), k
    assert len(draws) == 2 * len(first_draws) == 2 * 3 * 3
    assert all(np.array_equal(a[0], b[0]) for a, b in zip(first_draws, draws[len(first_draws):]))
    # the first batch: encoder(specification(face, its draws)) on the host-made images
    train_flag, idx, fed = rec[0]
    params, angles = first_draws[0]
    assert train_flag and len(idx) == 16 == len(params)
    assert len(set(params["flip"].tolist())) == 2 and float(np.abs(angles).max()) > 1.0     # the draws do vary
    ds = VNCelebDataset(**cfg["train_dataset"]["args"])
    imgs = np.stack([A.pillow_facenet_aug(ds.faces[int(k)], float(angles[r]), int(params["i"][r]), int(params["j"][r]),
                                          int(params["flip"][r]), 160) for r, k in enumerate(idx)])
    want = _encoder()(torch.from_numpy(A.normalise(imgs)).to(DEV))
    d = float((fed - want).abs().max())
    print("first batch: max |fed - encoder(specification)| = %g" % d)
    assert torch.equal(fed, want)
    # the augmented batch is not the plain one
    plain = _encoder()(torch.from_numpy(A.normalise(ds.faces[idx.numpy()])).to(DEV))
    assert float((fed - plain).abs().max()) > 1e-3


def test_train_py_cli_with_the_aug_config(tmp_path):
    from vn_celeb_face_recognition_amd.classifier import MLPModel, load_model_classify
    root = str(tmp_path)
    write_face_dataset(root)
    cfg = aug_train_config(root, transforms="facenet_aug", epochs=2)
    with open(os.path.join(root, "cfg.json"), "w") as f:
        json.dump(cfg, f)
    r = subprocess.run([sys.executable, os.path.join(REPO, "train.py"), "-c", os.path.join(root, "cfg.json"), "-d", "GPU"], cwd=root,
                       env=dict(os.environ, PYTHONPATH=REPO), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Train Epoch: 2" in r.stderr + r.stdout and "val_neg_log_llhood" in r.stderr + r.stdout
    runs = os.listdir(os.path.join(root, "saved", "models"))
    assert len(runs) == 1
    files = sorted(os.listdir(os.path.join(root, "saved", "models", runs[0])))
    assert files == ["checkpoint-epoch1.pth", "checkpoint-epoch2.pth", "model_best.pth"]
    m = MLPModel(512, 12)
    load_model_classify(os.path.join(root, "saved", "models", runs[0], "model_best.pth"), m)
    text = open(os.path.join(root, "saved", "logs", runs[0], "log_loss.txt")).read().splitlines()
    assert text[0] == "Epoch,Train_loss,Validation_loss" and len(text) == 3
