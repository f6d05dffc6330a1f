"""Host side of the facenet_aug training path: the NumPy specification of the augmentation against the
Pillow-made golden file and against live Pillow, the pinned draw order, VNCelebDataset's ordering and train.py's gating.
No GPU."""
import copy
import json
import math
import os

import numpy as np
import pytest
import torch

from aug_golden import aug_train_config, load_cases, write_face_dataset
from conftest import REPO
from vn_celeb_face_recognition_amd import augment as A


def test_specification_equals_the_pillow_golden_byte_for_byte():
    cases = load_cases()
    assert [(c[1], c[2]) for c in cases] == [(160, 160)] * 4 + [(112, 112)] * 2 + [(150, 160)] * 2
    assert any(c[3] == 0.0 for c in cases) and any(c[6] for c in cases)
    for face, s, t, angle, i, j, flip, want in cases:
        got = A.pillow_facenet_aug(face, angle, i, j, flip, t)
        assert got.dtype == np.uint8 and got.shape == (t, t, 3)
        assert int((got != want).sum()) == 0, (s, t, angle)


def test_specification_equals_live_pillow():
    Image = pytest.importorskip("PIL.Image")
    ImageOps = pytest.importorskip("PIL.ImageOps")
    rng = np.random.RandomState(5)
    face0 = load_cases()[0][0]
    for s, t in ((160, 160), (112, 112), (150, 160), (37, 50)):
        face = np.ascontiguousarray(face0[:s, :s])
        p = A.crop_padding(s, t)
        for angle in (-10.0, 10.0, 0.0, float(rng.uniform(-10, 10)), float(np.float32(rng.uniform(-10, 10)))):
            i, j = (int(v) for v in rng.randint(0, s + 2 * p - t + 1, 2))
            flip = int(rng.randint(0, 2))
            im = ImageOps.expand(Image.fromarray(face).rotate(angle, Image.BICUBIC), border=p, fill=0).crop((j, i, j + t, i + t))
            if flip:
                im = im.transpose(Image.FLIP_LEFT_RIGHT)
            got = A.pillow_facenet_aug(face, angle, i, j, flip, t)
            assert int((got != np.asarray(im)).sum()) == 0, (s, t, angle, i, j, flip)


def test_rotate_matrix_is_the_matrix_pillow_computes(monkeypatch):
    # written out from PIL/Image.py rotate (angle % 360, -radians, round(, 15), centre s/2)
    for s in (160, 112, 150):
        for angle in (-10.0, -3.25, 0.0, 7.5, 9.999):
            a = -math.radians(angle % 360.0)
            m = [round(math.cos(a), 15), round(math.sin(a), 15), 0.0, round(-math.sin(a), 15), round(math.cos(a), 15), 0.0]
            c = s / 2.0
            m[2] = m[0] * -c + m[1] * -c + m[2] + c
            m[5] = m[3] * -c + m[4] * -c + m[5] + c
            assert A.rotate_matrix(angle, s) == m
    # and captured from Pillow itself: Image.rotate hands its matrix to Image.transform
    Image = pytest.importorskip("PIL.Image")
    seen = []
    orig = Image.Image.transform

    def spy(self, size, method, data=None, *a, **k):
        seen.append(list(data))
        return orig(self, size, method, data, *a, **k)
    monkeypatch.setattr(Image.Image, "transform", spy)
    for s, angle in ((160, -7.3125), (112, 4.4), (150, 9.9)):
        Image.fromarray(np.zeros((s, s, 3), np.uint8)).rotate(angle, Image.BICUBIC)
        assert seen[-1] == A.rotate_matrix(angle, s)


def test_angle_zero_on_the_image_without_flip_is_the_identity():
    for face, s, t, *_ in load_cases():
        if s != t:
            continue
        p = A.crop_padding(s, t)
        assert p == 2
        assert np.array_equal(A.pillow_facenet_aug(face, 0.0, p, p, 0, t), face)
        prm = A.identity_params(3, s, t)
        assert list(prm["m"][0]) == [1.0, 0.0, 0.0, 0.0, 1.0, 0.0] and prm["i"][2] == prm["j"][2] == prm["pad"][2] == 2 and prm["flip"][1] == 0
    with pytest.raises(ValueError, match="does not resize"):
        A.identity_params(1, 150, 160)


def test_crop_padding_follows_pad_if_needed():
    assert A.crop_padding(160, 160) == 2 and A.crop_padding(112, 112) == 2 and A.crop_padding(200, 160) == 2
    assert A.crop_padding(150, 160) == 8 and A.crop_padding(156, 160) == 2 and A.crop_padding(155, 160) == 3


def test_draws_consume_the_generator_in_the_pinned_order():
    n, s, t = 5, 160, 160
    torch.manual_seed(77)
    params, angles = A.draw_facenet_aug_params(n, s, t)
    after = torch.rand(1)
    torch.manual_seed(77)
    for k in range(n):
        angle = float(torch.empty(1).uniform_(-10, 10).item())
        i = int(torch.randint(0, s + 4 - t + 1, (1,)).item())
        j = int(torch.randint(0, s + 4 - t + 1, (1,)).item())
        flip = bool(torch.rand(1) < 0.5)
        assert angles[k] == angle and -10.0 <= angle <= 10.0
        assert (params["i"][k], params["j"][k], params["flip"][k], params["pad"][k]) == (i, j, int(flip), 2)
        assert list(params["m"][k]) == A.rotate_matrix(angle, s)
    assert torch.equal(after, torch.rand(1))       # nothing else was drawn
    assert len(set(params["flip"].tolist())) == 2 or n < 4


def test_no_crop_draw_when_the_padded_size_equals_the_target():
    n, s, t = 4, 156, 160       # padding 2 per side: the padded image is exactly 160 x 160 (RandomCrop.get_params returns early)
    assert s + 2 * A.crop_padding(s, t) == t
    torch.manual_seed(3)
    params, angles = A.draw_facenet_aug_params(n, s, t)
    torch.manual_seed(3)
    for k in range(n):
        assert angles[k] == float(torch.empty(1).uniform_(-10, 10).item())
        assert params["i"][k] == 0 and params["j"][k] == 0
        assert params["flip"][k] == int(bool(torch.rand(1) < 0.5))


def test_check_params_refuses_a_crop_outside_the_padded_image():
    ok = A.make_params([1.0, -2.0], [0, 4], [4, 0], [0, 1], 160, 160)
    A.check_params(ok, 160, 160)
    for field, value in (("i", 5), ("j", -1), ("pad", -1)):
        bad = ok.copy()
        bad[field][1] = value
        with pytest.raises(ValueError, match="outside"):
            A.check_params(bad, 160, 160)


def test_transforms_dict_names():
    assert isinstance(A.get_transform("default"), A.DefaultTransform) and isinstance(A.get_transform("facenet_aug"), A.FacenetAug)
    with pytest.raises(NotImplementedError, match="imgaug"):
        A.get_transform("rank1_aug")
    with pytest.raises(KeyError):
        A.get_transform("emotion_inf")


def test_vnceleb_dataset_orders_like_the_reference(tmp_path):
    from PIL import Image
    from vn_celeb_face_recognition_amd.trainer import VNCelebDataset
    root = str(tmp_path)
    label = {"7": ["b.png", "a.png"], "2": ["z.png"], "11": ["m.png", "c.png", "k.png"]}     # dict order, not numeric order
    rng = np.random.RandomState(1)
    pix = {}
    for names in label.values():
        for nm in names:
            pix[nm] = rng.randint(0, 256, (20, 20, 3)).astype(np.uint8)
            Image.fromarray(pix[nm]).save(os.path.join(root, nm))
    with open(os.path.join(root, "l.json"), "w") as f:
        json.dump(label, f)
    ds = VNCelebDataset(root, os.path.join(root, "l.json"))
    # data_loader/vn_celeb_dataset.py:39-47: classes in dict order, each class's files sorted, label int(key)
    assert ds.img_names == ["a.png", "b.png", "z.png", "c.png", "k.png", "m.png"]
    assert ds.labels == [7, 7, 2, 11, 11, 11] and len(ds) == 6 and ds.n_classes == 3 and ds.size == 20
    assert ds.faces.shape == (6, 20, 20, 3) and all(np.array_equal(ds.faces[k], pix[nm]) for k, nm in enumerate(ds.img_names))
    assert ds[4] == (4, 11, os.path.join(root, "k.png"))
    loader = torch.utils.data.DataLoader(ds, batch_size=4, shuffle=False)
    idx, lab, paths = next(iter(loader))
    assert idx.tolist() == [0, 1, 2, 3] and lab.tolist() == [7, 7, 2, 11] and paths[2].endswith("z.png")
    # documented deviation: one size, square
    Image.fromarray(np.zeros((24, 24, 3), np.uint8)).save(os.path.join(root, "z.png"))
    with pytest.raises(ValueError, match="one size"):
        VNCelebDataset(root, os.path.join(root, "l.json"))
    Image.fromarray(np.zeros((20, 24, 3), np.uint8)).save(os.path.join(root, "a.png"))
    with pytest.raises(ValueError, match="square"):
        VNCelebDataset(root, os.path.join(root, "l.json"))


def test_train_py_gating(tmp_path, monkeypatch):
    import train
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    root = str(tmp_path)
    write_face_dataset(root, n_cls=2, per_cls_train=1, per_cls_val=1)
    cfg = aug_train_config(root)
    # the shipped file and the test's own config pass every check up to the one for a GPU
    shipped = json.load(open(os.path.join(REPO, "cfg", "train_cfg_aug_emb_classify.json")))
    assert shipped["trainer"]["chosen_idx_enc"] == 0 and shipped["trainer"]["encoders"][0]["name"] == "InceptionResnetV1"
    for c in (cfg, shipped, dict(copy.deepcopy(cfg), transforms={"name": "default", "resize": False})):
        assert train.aug_config(c) is True
        with pytest.raises(SystemExit, match="no GPU is visible"):
            train.main(copy.deepcopy(c))

    def refused(match, **edit):
        c = copy.deepcopy(cfg)
        for path, v in edit.items():
            d = c
            keys = path.split("__")
            for k in keys[:-1]:
                d = d[k]
            d[keys[-1]] = v
        with pytest.raises(SystemExit, match=match):
            train.main(c)
    refused("rank1_aug", transforms__name="rank1_aug")
    refused("resize", transforms__resize=True)
    refused("default or facenet_aug", transforms__name="emotion_inf")
    refused("AugClassificationTrainer", trainer__name="ClassificationTrainer")
    refused("AugClassificationTrainer", trainer__name="ImageClassificationTrainer")
    refused("AugClassificationTrainer", val_dataset__name="VNCelebEmbDataset")
    refused("MLPModel", model__name="InceptionResnetV1")
    refused("chosen_idx_enc", trainer__chosen_idx_enc=3)
    refused("Adam", optimizer__name="SGD")
    refused("trainer.device must be GPU", trainer__device="CPU")
    # the embedding configuration behaves as before
    emb = json.load(open(os.path.join(REPO, "cfg", "train_cfg_emb_classify.json")))
    assert train.aug_config(emb) is False
    bad = copy.deepcopy(emb)
    bad["model"]["name"] = "InceptionResnetV1"
    with pytest.raises(SystemExit, match="MLPModel on VNCelebEmbDataset only"):
        train.main(bad)
    bad = copy.deepcopy(emb)
    bad["trainer"]["name"] = "ImageClassificationTrainer"
    with pytest.raises(SystemExit, match="is not built"):
        train.main(bad)
    emb["train_dataset"]["args"]["label_file"] = os.path.join(root, "absent.json")
    with pytest.raises(FileNotFoundError):       # past every check, at the data set
        train.main(emb)
