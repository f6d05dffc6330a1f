"""CPU: the gallery's host layer -- file format, refusals, registry, CLI dispatch, enroll.py's walk, and the float64 oracle
the GPU tests compare against."""
import argparse
import json
import os
import sys

import numpy as np
import pytest
import torch

from conftest import REPO

import gallery_oracle as go
from vn_celeb_face_recognition_amd import models
from vn_celeb_face_recognition_amd.gallery import GalleryModel


def _unit(n, dim, seed):
    x = np.random.default_rng(seed).standard_normal((n, dim))
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def test_npz_round_trip_all_mode(tmp_path):
    emb, lab = _unit(5, 32, 0), np.array([3, 3, 0, 7, 1], np.int64)
    p = str(tmp_path / "g.npz")
    np.savez(p, embeddings=emb, labels=lab, mode=np.array("all"), num_classes=np.array(8, np.int64))
    g = GalleryModel.load(p)
    assert (g.mode, g.input_dim, g.size, g.num_classes) == ("all", 32, 5, 8)
    p2 = str(tmp_path / "g2.npz")
    g.save(p2)
    with np.load(p2, allow_pickle=False) as z:
        assert sorted(z.files) == ["embeddings", "labels", "mode", "num_classes"]
        assert z["embeddings"].dtype == np.float32 and np.array_equal(z["embeddings"], emb)
        assert z["labels"].dtype == np.int64 and np.array_equal(z["labels"], lab)
        assert str(z["mode"]) == "all" and int(z["num_classes"]) == 8
    assert GalleryModel.load(p2).size == 5


def test_npz_round_trip_centroid_mode(tmp_path):
    emb, lab = _unit(3, 16, 1), np.array([1, 4, 9], np.int64)
    sums, counts = (emb * np.float32(2.5)).astype(np.float32), np.array([3, 1, 2], np.int64)
    p = str(tmp_path / "c.npz")
    np.savez(p, embeddings=emb, labels=lab, mode=np.array("centroid"), num_classes=np.array(10, np.int64), sums=sums, counts=counts)
    g = GalleryModel.load(p)
    assert g.mode == "centroid" and g.num_classes == 10 and g.size == 3
    p2 = str(tmp_path / "c2.npz")
    g.save(p2)
    with np.load(p2, allow_pickle=False) as z:
        assert sorted(z.files) == ["counts", "embeddings", "labels", "mode", "num_classes", "sums"]
        assert np.array_equal(z["sums"], sums) and z["sums"].dtype == np.float32
        assert np.array_equal(z["counts"], counts) and z["counts"].dtype == np.int64
        assert np.array_equal(z["embeddings"], emb) and np.array_equal(z["labels"], lab)
    # a centroid file without its sums cannot be appended to: refused
    np.savez(p, embeddings=emb, labels=lab, mode=np.array("centroid"), num_classes=np.array(10, np.int64))
    with pytest.raises(ValueError):
        GalleryModel.load(p)
    # rows out of label order: refused
    np.savez(p, embeddings=emb, labels=lab[::-1].copy(), mode=np.array("centroid"), num_classes=np.array(10, np.int64), sums=sums,
             counts=counts)
    with pytest.raises(ValueError):
        GalleryModel.load(p)


def test_pickled_and_foreign_files_are_refused(tmp_path):
    p = str(tmp_path / "p.npz")
    np.savez(p, embeddings=np.array([{"a": 1}], dtype=object), labels=np.zeros(1, np.int64), mode=np.array("all"),
             num_classes=np.array(1))
    with pytest.raises(ValueError):
        GalleryModel.load(p)
    np.savez(p, arr_0=np.zeros((512,), np.float32))     # an embedding file is not a gallery
    with pytest.raises(ValueError, match="not a gallery file"):
        GalleryModel.load(p)
    np.savez(p, embeddings=np.full((1, 16), np.nan, np.float32), labels=np.zeros(1, np.int64), mode=np.array("all"),
             num_classes=np.array(1))
    with pytest.raises(ValueError):
        GalleryModel.load(p)


def test_add_refuses_bad_rows_and_labels_on_the_host():
    g = GalleryModel(16)          # on the CPU: the ValueError comes before any device is looked for
    ok = np.ones((2, 16), np.float32)
    for bad in (np.nan, np.inf, -np.inf):
        x = ok.copy()
        x[1, 3] = bad
        with pytest.raises(ValueError, match="non-finite"):
            g.add(x, [0, 1])
    with pytest.raises(ValueError, match="non-finite"):
        g.add(torch.from_numpy(np.full((1, 16), np.nan, np.float32)), [0])
    for labels in ([0, -1], [0, 2 ** 31], np.array([0.0, 1.0])):
        with pytest.raises(ValueError, match="labels"):
            g.add(ok, labels)
    with pytest.raises(ValueError):
        g.add(ok, [0])                                   # one label for two rows
    with pytest.raises(ValueError):
        g.add(np.ones((2, 32), np.float32), [0, 1])      # wrong width
    for dim in (0, 8, 24, 528):
        with pytest.raises(ValueError):
            GalleryModel(dim)
    with pytest.raises(ValueError):
        GalleryModel(512, mode="mean")


def test_registry_and_cpu_refusals(tmp_path):
    assert models.GalleryModel is GalleryModel
    g = GalleryModel(16, num_classes=4).eval()
    assert g.to("cpu") is g and g.size == 0 and g.num_classes == 4
    x = torch.ones((2, 16))
    with pytest.raises(RuntimeError, match="MI355X only"):
        g.add(np.ones((2, 16), np.float32), [0, 1])
    for call in (lambda: g.search(x), lambda: g.classify(x), lambda: g.classify(x, want_logp=False)):
        with pytest.raises(RuntimeError, match="MI355X only"):
            call()
    with pytest.raises(NotImplementedError, match="no probability model"):
        g.classify(x, want_logp=True)
    with pytest.raises(NotImplementedError, match="no probability model"):
        g(x)


def test_build_models_dispatches_on_npz(monkeypatch, tmp_path):
    sys.path.insert(0, REPO)
    import demo_image
    calls = []

    class FakeGallery:
        input_dim, num_classes = 512, 77

        @classmethod
        def load(cls, path):
            calls.append(("gallery.load", path))
            return cls()

        def to(self, device):
            calls.append(("gallery.to", device))
            return self

    class FakeMLP:
        def __init__(self, input_dim, num_classes):
            calls.append(("mlp", input_dim, num_classes))

        def to(self, device):
            calls.append(("mlp.to", device))
            return self

    class FakeDet:
        def __init__(self, **kw):
            pass

        def eval(self):
            return self

        def to(self, device):
            return self

    monkeypatch.setattr(demo_image.model_md, "GalleryModel", FakeGallery)
    monkeypatch.setattr(demo_image.model_md, "MLPModel", FakeMLP)
    monkeypatch.setattr(demo_image.model_md, "MTCNN", FakeDet)
    monkeypatch.setattr(demo_image.model_md, "InceptionResnetV1", FakeDet)
    monkeypatch.setattr(demo_image, "load_model_classify", lambda path, m: calls.append(("load_model_classify", path)) or m)
    l2n = tmp_path / "l2n.csv"
    l2n.write_text("label,name\n0,a\n")
    common = ["-l2n", str(l2n), "-dargs", os.path.join(REPO, "cfg/detection/mtcnn.json"), "-eargs",
              os.path.join(REPO, "cfg/embedding/inception_resnet_v1.json")]
    parser = demo_image.build_parser("t")
    args = parser.parse_args(["-m", "some/gallery.npz"] + common)
    clf = demo_image.build_models(args, "cuda:0")[3]
    assert isinstance(clf, FakeGallery) and calls == [("gallery.load", "some/gallery.npz"), ("gallery.to", "cuda:0")]
    assert args.num_classes == 77
    with pytest.raises(SystemExit, match="does not match"):
        demo_image.build_models(parser.parse_args(["-m", "g.npz", "-id", "128"] + common), "cuda:0")
    del calls[:]
    clf = demo_image.build_models(parser.parse_args(["-m", "model_best.pth", "-nc", "9"] + common), "cuda:0")[3]
    assert isinstance(clf, FakeMLP) and calls == [("mlp", 512, 9), ("load_model_classify", "model_best.pth"), ("mlp.to", "cuda:0")]


def test_enroll_walk(tmp_path):
    sys.path.insert(0, REPO)
    import enroll
    d = tmp_path / "emb"
    d.mkdir()
    for i, stem in enumerate(["b", "a", "c", "z"]):
        np.savez_compressed(str(d / (stem + ".npz")), np.full((16,), i, np.float32))
    lj = tmp_path / "l.json"
    lj.write_text(json.dumps({"5": ["b.png", "a.png"], "2": ["z.jpg", "c.png"]}))
    paths, labels = enroll.list_samples(str(d), str(lj))
    assert [p.name for p in paths] == ["a.npz", "b.npz", "c.npz", "z.npz"] and labels == [5, 5, 2, 2]   # sorted per label
    emb, lab = enroll.load_samples(str(d), str(lj))
    assert emb.shape == (4, 16) and emb.dtype == np.float32 and emb[:, 0].tolist() == [1, 0, 2, 3] and lab.tolist() == [5, 5, 2, 2]
    lj.write_text(json.dumps({"5": ["b.png", "nope.png"]}))
    with pytest.raises(FileNotFoundError, match="nope.png"):
        enroll.list_samples(str(d), str(lj))


def test_oracle_tie_order_and_padding():
    g = np.array([[1, 0], [0, 1], [1, 0], [2, 0], [-1, 0]], np.float64)
    idx, lab, sc = go.search(np.array([[3.0, 0.0]]), g, [10, 11, 12, 13, 14], 7)
    assert idx.tolist() == [[0, 2, 3, 1, 4, -1, -1]]                 # ties by ascending index, k > G padded
    assert lab.tolist() == [[10, 12, 13, 11, 14, -1, -1]]
    assert sc[0, :5].tolist() == [1, 1, 1, 0, -1] and np.isneginf(sc[0, 5:]).all()
    idx, _, sc = go.search(np.zeros((1, 2)), g, np.arange(5), 3)     # a zero query: every score 0, rows in order
    assert idx.tolist() == [[0, 1, 2]] and (sc == 0).all()
    idx, _, sc = go.topk(np.array([[0.5, np.nan, -0.25, np.nan]]), np.arange(4), 4)
    assert idx.tolist() == [[0, 2, 1, 3]] and np.isnan(sc[0, 2:]).all()   # NaN below every number, then by index
    s = go.scores(np.array([[np.nan, 1.0]]), g)
    assert np.isnan(s).all()
    assert abs(go.tol(512) - 6.2e-5) < 1e-6
    worst = go.check_ranks(np.array([[0, 2, 3]]), np.array([[1.0, 1.0, 1.0]]), go.scores(np.array([[3.0, 0.0]]), g), 3, go.tol(2))
    assert worst == 0.0
    with pytest.raises(AssertionError):
        go.check_ranks(np.array([[1, 2, 3]]), np.array([[1.0, 1.0, 1.0]]), go.scores(np.array([[3.0, 0.0]]), g), 3, go.tol(2))


@pytest.mark.parametrize("chunk_rows", [0, 32])
@pytest.mark.parametrize("G", [0, 1, 3, 4, 5, 70, 100000])
def test_cluster_and_tracks_workspaces_keep_their_layout(G, chunk_rows):
    """The two carved workspaces (csrc/gallery_cluster.hip, gallery_tracks.hip, both on gallery_core.h's carver) have the
    totals of the layouts they were first written with: (nchunks, G) 8-byte keys then seven arrays of G 32-bit entries, and
    five such arrays, each section rounded up to 16 bytes, an array to a multiple of 4 entries; 16 bytes for an empty one."""
    from vn_celeb_face_recognition_amd import _lib
    lib = _lib.load()

    def align16(n):
        return (n + 15) // 16 * 16

    cr = chunk_rows
    if cr == 0:                                                  # the library's default: about 2048 waves, 64 rows at least
        target = max(2048 // max((G + 15) // 16, 1), 1)
        cr = max((-(-G // target) + 31) // 32 * 32, 64)
    nchunks, padded = -(-G // cr), (G + 3) // 4 * 4
    assert lib.vnf_gallery_cluster_workspace_bytes(G, chunk_rows) == max(align16(nchunks * G * 8) + 7 * align16(padded * 4), 16)
    assert lib.vnf_gallery_tracks_workspace_bytes(G) == max(5 * align16(padded * 4), 16)
