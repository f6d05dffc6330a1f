"""GPU: cluster.py end to end on the small case of tests/gallery_cluster_data.py -- unlabelled embedding files are grouped
as the float64 oracle groups them, enroll.py reads the result as its label file, and a gallery with three swapped labels
gets exactly those three rows named."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO

import gallery_cluster_data as data
import gallery_cluster_oracle as gco
import gallery_oracle as go

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MS = 3


def _run(args, cwd):
    r = subprocess.run([sys.executable] + args, cwd=cwd, env=dict(os.environ, PYTHONPATH=REPO), capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def test_a_directory_is_grouped_as_the_oracle_groups_it_and_enrols(tmp_path):
    x, s64 = data.case("small")
    o = data.oracle("small", MS)                       # asserts both margins on the CPU
    d = tmp_path / "faces_emb"
    d.mkdir()
    names = ["face_%03d.npz" % i for i in range(x.shape[0])]
    for name, row in zip(names, x):
        np.savez_compressed(str(d / name), row)
    cj, nf, rj = str(tmp_path / "clusters.json"), str(tmp_path / "noise.txt"), str(tmp_path / "detail.json")
    so = _run([os.path.join(REPO, "cluster.py"), "-d", str(d), "--threshold", repr(data.T), "--min_samples", str(MS), "-o", cj,
               "--noise_file", nf, "-r", rj], str(tmp_path))
    want = {str(k): [names[i] for i in np.flatnonzero(o.cluster == k)] for k in range(o.n_clusters)}
    noise = [names[i] for i in np.flatnonzero(o.cluster < 0)]
    assert json.load(open(cj)) == want and open(nf).read().split() == noise
    assert "%d files: %d clusters, %d border files, %d noise files" % (len(names), o.n_clusters, o.border.sum(), len(noise)) in so
    biggest = max(want, key=lambda k: len(want[k]))
    assert "cluster %s: %d files" % (biggest, len(want[biggest])) in so
    detail = json.load(open(rj))
    assert [r["file"] for r in detail["rows"]] == names and [r["cluster"] for r in detail["rows"]] == o.cluster.tolist()
    assert [r["degree"] for r in detail["rows"]] == o.degree.tolist()
    assert np.abs(np.array([r["nn_score"] for r in detail["rows"]]) - o.nn_score).max() <= go.tol(512)
    # clusters.json is enroll.py's label file: the clustered rows, cluster id for label
    gal = str(tmp_path / "gallery.npz")
    so = _run([os.path.join(REPO, "enroll.py"), "-d", str(d), "-l", cj, "-o", gal], str(tmp_path))
    rows = np.concatenate([np.flatnonzero(o.cluster == k) for k in range(o.n_clusters)])
    assert "Enrolled %d rows of %d labels (all mode)" % (rows.size, o.n_clusters) in so
    with np.load(gal, allow_pickle=False) as z:
        assert np.array_equal(z["labels"], o.cluster[rows])
        unit = go.normalize(x[rows])
        assert (np.abs(z["embeddings"].astype(np.float64) - unit) <= 70 * 2.0 ** -24 * np.abs(unit) + 1e-45).all()


def test_swapped_labels_are_named(tmp_path):
    from vn_celeb_face_recognition_amd.gallery import GalleryModel
    x, s64 = data.case("small")
    sub = np.flatnonzero(data.oracle("small", MS).cluster >= 0)
    o = gco.cluster_scores(s64[np.ix_(sub, sub)], data.T, MS)
    assert o.margin_t > 4 * go.tol(512) and o.margin_border > 4 * go.tol(512) and (o.cluster >= 0).all()
    sizes = np.bincount(o.cluster)
    assert (np.sort(sizes)[-2:] >= 5).all()
    a, b = np.argsort(sizes)[-2:]
    labels = o.cluster.copy()
    swapped = sorted([int(np.flatnonzero(o.cluster == a)[1]), int(np.flatnonzero(o.cluster == a)[3]), int(np.flatnonzero(o.cluster == b)[2])])
    for i in swapped:
        labels[i] = b if o.cluster[i] == a else a
    gal, rj = str(tmp_path / "g.npz"), str(tmp_path / "report.json")
    GalleryModel(512).to(DEV).add(x[sub], labels).save(gal)
    so = _run([os.path.join(REPO, "cluster.py"), "-g", gal, "--threshold", repr(data.T), "--min_samples", str(MS), "-r", rj], str(tmp_path))
    r = json.load(open(rj))
    assert [s["row"] for s in r["suspect_rows"]] == swapped
    assert all(s["majority"] == int(o.cluster[s["row"]]) and s["label"] == int(labels[s["row"]]) for s in r["suspect_rows"])
    assert r["mixed_clusters"] == sorted([int(a), int(b)]) and r["n_clusters"] == o.n_clusters and r["noise_rows"] == []
    assert r["degree"] == o.degree.tolist()
    assert "3 rows whose label is not their cluster's majority, 2 clusters with several labels" in so
