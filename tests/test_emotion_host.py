"""CPU-only tests of the emotion feature: the golden fixture against a functional restatement of the network, the
NumPy restatement of Pillow's bilinear resize, the host transform, the tag table loader, the model wrapper's host
surface and find_emotion's ordering rules."""
import json
import os
import pickle

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_image, seeded_normal
from emotion_restatement import rn50_2b_forward

NC, NP = 690, 300


def _golden():
    return np.load(os.path.join(GOLDEN, "rn50_2b_seed0.npz"))


def test_restatement_reproduces_reference_golden():
    """fp32 CPU against fp32 CPU with a different summation order: 1e-5 relative per row."""
    from vn_celeb_face_recognition_amd.weights import generate_state_dict
    g = _golden()
    sd = generate_state_dict("rn50_2b", 0, as_torch=True, num_classes=NC, num_projections=NP)
    x = seeded_normal((2, 3, 224, 224), int(g["input_seed"]))
    cls, proj = rn50_2b_forward(sd, x)
    for got, want in ((cls.numpy(), g["x_cls"]), (proj.numpy(), g["x_proj"])):
        assert got.shape == want.shape
        rel = np.linalg.norm(got - want, axis=1) / np.linalg.norm(want, axis=1)
        print("restatement vs golden: rel L2 per row", rel)
        assert (rel <= 1e-5).all(), rel
    # the golden's own top-6 is what find_emotion's rule gives on its logits, and its gaps make index equality fair
    top7 = np.sort(g["x_cls"], axis=1)[:, ::-1][:, :7]
    assert ((top7[:, :-1] - top7[:, 1:]).min(axis=1) >= 1e-3 * np.abs(g["x_cls"]).max(axis=1)).all()
    assert (np.argsort(-g["x_cls"], axis=1, kind="stable")[:, :6] == g["top6_idx"]).all()


def test_spec_matches_generated_state_dict_and_heads():
    from vn_celeb_face_recognition_amd.weights import generate_state_dict, rn50_2b_spec
    spec = rn50_2b_spec(NC, NP)
    sd = generate_state_dict("rn50_2b", 0, num_classes=NC, num_projections=NP)
    assert [n for n, _, _ in spec] == list(sd) and sd["fc.weight"].shape == (NC, 2048) and sd["proj.weight"].shape == (NP, 2048)
    assert sum(1 for n in sd if n.endswith("conv1.weight") or n.endswith("conv2.weight") or n.endswith("conv3.weight")
               or n.endswith("downsample.0.weight")) == 1 + 16 * 3 + 4
    assert rn50_2b_spec()[-4][1] == (1000, 2048) and rn50_2b_spec()[-2][1] == (300, 2048)


@pytest.mark.parametrize("S", [96, 112, 150, 160, 224])
def test_numpy_resize_equals_pillow(S):
    from PIL import Image
    from vn_celeb_face_recognition_amd.emotion import pillow_bilinear_resize
    a = np.random.default_rng(S).integers(0, 256, (S, S, 3), dtype=np.uint8)
    want = np.asarray(Image.fromarray(a).resize((224, 224), Image.BILINEAR))
    got = pillow_bilinear_resize(a)
    assert got.dtype == np.uint8 and got.shape == (224, 224, 3)
    assert int((got != want).sum()) == 0


def test_numpy_resize_equals_pillow_on_golden_crop_and_downscale():
    from PIL import Image
    from vn_celeb_face_recognition_amd.emotion import pillow_bilinear_resize
    img = load_image("mrDam_HaHo_recog.jpg")
    for y0, x0, S in ((40, 60, 181), (10, 10, 150), (0, 0, 300)):   # 300: a downscale (support > 1, wider windows)
        a = np.ascontiguousarray(img[y0:y0 + S, x0:x0 + S])
        assert a.shape == (S, S, 3)
        want = np.asarray(Image.fromarray(a).resize((224, 224), Image.BILINEAR))
        assert int((pillow_bilinear_resize(a) != want).sum()) == 0


def test_trans_emotion_inf_is_resize_totensor_normalize():
    from PIL import Image
    from vn_celeb_face_recognition_amd.pipeline import trans_emotion_inf
    a = np.random.default_rng(5).integers(0, 256, (112, 112, 3), dtype=np.uint8)
    r = np.asarray(Image.fromarray(a).resize((224, 224), Image.BILINEAR)).astype(np.float64)
    want = (r / 255.0 - np.array([0.485, 0.456, 0.406])) / np.array([0.229, 0.224, 0.225])
    for arg in (a, Image.fromarray(a)):
        got = trans_emotion_inf(arg)
        assert got.device.type == "cpu" and got.dtype == torch.float32 and tuple(got.shape) == (3, 224, 224)
        assert np.abs(got.numpy().transpose(1, 2, 0) - want).max() <= 1e-6
    with pytest.raises(ValueError):
        trans_emotion_inf(np.zeros((100, 112, 3), np.uint8))


def test_load_etag2idx_pickle_json_and_refusal(tmp_path):
    from vn_celeb_face_recognition_amd.cli_utils import load_etag2idx
    names = json.load(open(os.path.join(GOLDEN, "etag2idx.json")))["idx2key"]
    assert len(names) == NC and len(set(names)) == NC
    tab = {"key2idx": {n: i for i, n in enumerate(names)}, "idx2key": {i: n for i, n in enumerate(names)}}
    pk = tmp_path / "etag2idx.pkl.keep"
    with open(pk, "wb") as f:
        pickle.dump(tab, f)
    js = tmp_path / "etag2idx.json"
    with open(js, "w") as f:
        json.dump({"key2idx": tab["key2idx"], "idx2key": {str(i): n for i, n in enumerate(names)}}, f)
    for p in (pk, js, os.path.join(GOLDEN, "etag2idx.json")):
        got = load_etag2idx(str(p))
        assert got == tab
    bad = tmp_path / "bad.pkl"
    with open(bad, "wb") as f:
        pickle.dump({"idx2key": {0: np.float64(1.0)}, "key2idx": {}}, f)   # names numpy globals
    with pytest.raises(pickle.UnpicklingError, match="global"):
        load_etag2idx(str(bad))
    evil = tmp_path / "evil.pkl"
    with open(evil, "wb") as f:
        f.write(b"cos\nsystem\n(S'true'\ntR.")
    with pytest.raises(pickle.UnpicklingError, match="global"):
        load_etag2idx(str(evil))


def test_model_host_surface(tmp_path):
    from vn_celeb_face_recognition_amd import models
    from vn_celeb_face_recognition_amd.cli_utils import read_json
    from vn_celeb_face_recognition_amd.weights import generate_state_dict
    from conftest import REPO
    kw = read_json(os.path.join(REPO, "cfg", "emotion", "resnet50_2_branch.json"))
    assert kw == {"pretrained": False, "num_classes": 690, "checkpoint_path": None}
    m = models.resnet_2branch_50(**kw).eval()
    assert m.num_classes == 690 and m.num_projections == 300 and m.to("cpu") is m
    with pytest.raises(RuntimeError, match="MI355X only"):
        m(torch.zeros(1, 3, 224, 224))
    sd = generate_state_dict("rn50_2b", 3, as_torch=True, num_classes=690, num_projections=300)
    assert not torch.equal(m.state_dict()["fc.weight"], sd["fc.weight"])
    ck = str(tmp_path / "emotion.pth")
    torch.save({"epoch": 1, "state_dict": {"module." + k: v for k, v in sd.items()}}, ck)
    m2 = models.resnet_2branch_50(pretrained=False, num_classes=690, checkpoint_path=ck)
    got = m2.state_dict()
    assert sorted(got) == sorted(sd) and all(torch.equal(torch.as_tensor(got[k]), sd[k]) for k in sd)
    with pytest.raises(RuntimeError):    # a checkpoint for other head sizes
        models.resnet_2branch_50(num_classes=7, checkpoint_path=ck)
    with pytest.raises(RuntimeError, match="Missing key"):
        m.load_state_dict({k: v for k, v in sd.items() if k != "proj.bias"})
    with pytest.raises(FileNotFoundError):
        models.resnet_2branch_50(pretrained=True)
    with pytest.raises(TypeError):
        models.resnet_2branch_50(bogus=1)


class _Stub:
    def __init__(self, logits):
        self.logits, self.evaled = logits, False

    def eval(self):
        self.evaled = True
        return self

    def __call__(self, x):
        return self.logits[: x.shape[0]], None


def test_find_emotion_order_and_tie_rule():
    from vn_celeb_face_recognition_amd.pipeline import find_emotion
    logits = torch.tensor([[0.5, 3.0, -1.0, 3.0, 2.0, 0.5, 7.0, 0.5],
                           [1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0]])
    stub = _Stub(logits)
    idx, prob = find_emotion(torch.zeros(2, 3, 4, 4), stub, topk=6)
    assert stub.evaled and idx.shape == (2, 6) and prob.shape == (2, 6)
    assert idx[0].tolist() == [6, 1, 3, 4, 0, 5]          # descending; exact ties lower index first
    assert idx[1].tolist() == [0, 1, 2, 3, 4, 5]
    sm = torch.softmax(logits, dim=1).numpy()
    assert np.allclose(prob, np.take_along_axis(sm, idx, axis=1), atol=1e-7) and (np.diff(prob, axis=1) <= 0).all()
    # a row without ties: what the reference's argsort / sort / flip gives
    r = torch.randn(3, 50, generator=torch.Generator().manual_seed(1))
    idx, prob = find_emotion(torch.zeros(3, 1), _Stub(r), topk=4)
    assert (idx == np.flip(np.argsort(r.numpy(), axis=1)[:, -4:], axis=1)).all()
    assert np.allclose(prob, np.flip(np.sort(torch.softmax(r, 1).numpy(), axis=1)[:, -4:], axis=1), atol=1e-7)
    with pytest.raises(ValueError):
        find_emotion(torch.zeros(2, 1), stub, topk=9)


def test_recognize_emotion_host_grouping_with_stub():
    """Per-frame grouping and the empty cases of demo_image.py:79-110, on a stub model and a caller's transform."""
    from vn_celeb_face_recognition_amd.pipeline import recognize_emotion
    logits = torch.arange(3 * 10, dtype=torch.float32).view(3, 10) % 7
    names = ["t%d" % i for i in range(10)]
    mp = np.vectorize(lambda i: names[i])
    faces = [np.full((8, 8, 3), v, np.uint8) for v in (1, 2, 3)]
    tf = lambda im: torch.from_numpy(np.asarray(im).astype(np.float32).transpose(2, 0, 1))   # noqa: E731
    tags, probs = recognize_emotion([[faces[0]], [], [faces[1], faces[2]]], "cpu", _Stub(logits), tf, mp, topk=3)
    assert [np.shape(t) for t in tags] == [(1, 3), (0,), (2, 3)] and [np.shape(p) for p in probs] == [(1, 3), (0, 3), (2, 3)]
    assert tags[0][0].tolist() == ["t6", "t5", "t4"] and tags[1] == []
    tags, probs = recognize_emotion([[], []], "cpu", _Stub(logits), tf, mp)
    assert tags == [[], []] and probs == [[], []]


def test_face_pipeline_with_emotion_keeps_one_lane_and_checks_face_size():
    """The emotion handle has one set of activation buffers: its calls must follow each other on one stream, so a
    pipeline with an emotion model runs one embedding lane (and embeds every submit at once), whatever was asked for."""
    from vn_celeb_face_recognition_amd import models
    from vn_celeb_face_recognition_amd.pipeline import FacePipeline
    emo = models.resnet_2branch_50(num_classes=7, num_projections=8)
    plain = FacePipeline(None, None, None, {}, 160, 0.0, embed_batch=64, embed_lanes=2)
    assert plain.embed_lanes == 2 and plain.embed_batch == 64 and plain.emotion is None
    withe = FacePipeline(None, None, None, {}, 160, 0.0, embed_batch=64, embed_lanes=2, emotion=emo, topk_emotions=3)
    assert withe.embed_lanes == 1 and withe.embed_batch == 0 and withe.topk_emotions == 3
    with pytest.raises(ValueError, match="224"):
        FacePipeline(None, None, None, {}, 256, 0.0, emotion=emo)
    with pytest.raises(NotImplementedError, match="one buffer set"):
        next(iter(emo.embed_stream([torch.zeros(1, 3, 224, 224)], lanes=2)))
    with pytest.raises(NotImplementedError):
        emo.set_contexts(2)
