"""CPU-only tests of the SE-IR ResNet-101 encoder (models.resnet101(use_se=True)): the reference's golden against the
functional restatement, the weight of the SE path in that result, the generator's keys, and the wrapper's host surface."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, REPO, seeded_normal
from seir_restatement import seir101_forward


@pytest.fixture(scope="module")
def case():
    """(golden, state dict, inputs, restatement output, restatement output with every gate forced to 1): computed once."""
    from vn_celeb_face_recognition_amd.weights import generate_state_dict
    g = np.load(os.path.join(GOLDEN, "seir101_seed0.npz"))
    sd = generate_state_dict("seir101", 0, as_torch=True)
    x = seeded_normal((2, 3, 112, 112), int(g["input_seed"]))
    return g, sd, x, seir101_forward(sd, x).numpy(), seir101_forward(sd, x, gates_one=True).numpy()


def test_restatement_reproduces_reference_golden(case):
    """fp32 CPU against fp32 CPU: 1e-5 relative per row, the bar of the emotion network's restatement."""
    g, _, _, got, _ = case
    want = g["features"]
    assert got.shape == want.shape == (2, 512)
    rel = np.linalg.norm(got - want, axis=1) / np.linalg.norm(want, axis=1)
    print("restatement vs golden: rel L2 per row", rel)
    assert (rel <= 1e-5).all(), rel
    assert np.allclose(np.linalg.norm(want, axis=1), 1.0, atol=1e-5)


def test_se_gates_carry_weight_in_the_embedding(case):
    """With every SE gate forced to 1 each embedding row moves by >= 1e-2 in L2: a hundred times the 1e-4 parity gate, so
    the parity tests do see the squeeze-and-excitation path."""
    _, _, _, y, y1 = case
    moved = np.linalg.norm(y - y1, axis=1)
    print("embedding shift with all gates = 1:", moved)
    assert (moved >= 1e-2).all(), moved


def test_generator_keys_equal_the_reference_modules(case):
    """Names, shapes and order of the generator's tensors are the reference module's state_dict, BatchNorm step counters
    aside (a plain dict loads strictly without them)."""
    from vn_celeb_face_recognition_amd.weights import seir_spec
    _, sd, _, _, _ = case
    ref = json.load(open(os.path.join(GOLDEN, "seir101_keys.json")))
    assert len(ref) == 796
    want = [(k, tuple(s)) for k, s in ref if not k.endswith("num_batches_tracked")]
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == want
    assert [n for n, _, _ in seir_spec()] == [k for k, _ in want]
    assert sum(int(np.prod(s)) for _, s in want) == 52244159
    b = sd["layer3.7.se.fc.2.bias"].numpy()
    assert b.std() > 0.5                                # the gates are spread: the bias is not a constant


def test_host_surface_and_refusals(tmp_path):
    from vn_celeb_face_recognition_amd import models
    from vn_celeb_face_recognition_amd.cli_utils import read_json
    from vn_celeb_face_recognition_amd.weights import generate_state_dict
    with pytest.raises(NotImplementedError, match="use_se=True"):
        models.resnet101()
    with pytest.raises(NotImplementedError, match="pretrained"):
        models.resnet101(use_se=True, pretrained=True)
    with pytest.raises(NotImplementedError, match="112"):
        models.resnet101(use_se=True, img_size=224)
    with pytest.raises(FileNotFoundError):
        models.resnet101(use_se=True, cp_path=str(tmp_path / "insight-face-v3.pt"))
    kw = read_json(os.path.join(REPO, "cfg", "embedding", "resnet101_se.json"))
    assert kw == {"use_se": True, "pretrained": False, "img_size": 112, "cp_path": None}
    m = models.resnet101(**kw).eval()
    assert m.input_size == 112 and m.head_classes is None and m.to("cpu") is m
    with pytest.raises(RuntimeError, match="MI355X only"):
        m(torch.zeros(1, 3, 112, 112))
    # a saved plain state_dict loads, strictly
    sd = generate_state_dict("seir101", 3, as_torch=True)
    assert not torch.equal(torch.as_tensor(m.state_dict()["fc.weight"]), sd["fc.weight"])
    ck = str(tmp_path / "seir.pt")
    torch.save(sd, ck)
    m2 = models.resnet101(use_se=True, cp_path=ck)
    got = m2.state_dict()
    assert list(got) == list(sd) and all(torch.equal(torch.as_tensor(got[k]), sd[k]) for k in sd)
    bad = str(tmp_path / "short.pt")
    torch.save({k: v for k, v in sd.items() if k != "layer3.22.se.fc.2.bias"}, bad)
    with pytest.raises(RuntimeError, match="layer3.22.se.fc.2.bias"):
        models.resnet101(use_se=True, cp_path=bad)
    # the shipped image-training config names the encoder behind its two pinned entries
    encs = read_json(os.path.join(REPO, "cfg", "train_cfg_aug_emb_classify.json"))["trainer"]["encoders"]
    assert [e["name"] for e in encs] == ["InceptionResnetV1", "iresnet100", "resnet101"] and encs[2]["args"]["use_se"] is True
