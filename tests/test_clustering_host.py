"""CPU: the clustering oracle on hand-made cases with known answers, vn_celeb_face_recognition_amd/clustering.py, the
generator the GPU tests share, cluster.py's refusals and the ABI's declaration.  No GPU."""
import ctypes
import json
import os
import re
import sys

import numpy as np
import pytest

from conftest import REPO

import gallery_cluster_data as data
import gallery_cluster_oracle as gco
import gallery_oracle as go
from vn_celeb_face_recognition_amd import _lib, clustering


def _scores(n, edges, base=0.1):
    """A symmetric (n,n) score matrix: 1 on the diagonal, `base` elsewhere, edges {(i, j): score}."""
    s = np.full((n, n), base)
    np.fill_diagonal(s, 1.0)
    for (i, j), v in edges.items():
        s[i, j] = s[j, i] = v
    return s


def test_a_chain_of_three_at_min_samples_1_3_and_4():
    s = _scores(6, {(1, 2): 0.7, (2, 3): 0.8})            # a - b - c among three loners
    o = gco.cluster_scores(s, 0.5, 3)                      # b has two neighbours: core; a and c are its borders
    assert o.degree.tolist() == [0, 1, 2, 1, 0, 0] and o.core.tolist() == [False, False, True, False, False, False]
    assert o.cluster.tolist() == [-1, 0, 0, 0, -1, -1] and o.n_clusters == 1 and o.border.tolist() == [False, True, False, True, False, False]
    assert o.nn_idx.tolist()[1:4] == [2, 3, 2] and o.nn_score[1] == 0.7 and abs(o.margin_t - 0.2) < 1e-12 and o.margin_border == np.inf
    o = gco.cluster_scores(s, 0.5, 1)                      # everybody is core: connected components, numbered by smallest row
    assert o.cluster.tolist() == [0, 1, 1, 1, 2, 3] and o.n_clusters == 4 and not o.border.any()
    o = gco.cluster_scores(s, 0.5, 2)
    assert o.cluster.tolist() == [-1, 0, 0, 0, -1, -1] and o.core.sum() == 3
    o = gco.cluster_scores(s, 0.5, 4)                      # nobody has three neighbours
    assert (o.cluster == -1).all() and o.n_clusters == 0 and not o.border.any()


def _two_clusters(to_a, to_b):
    """Rows 0..2 and 3..5 are two triangles, row 6 a neighbour of rows 1 and 4 with these scores."""
    e = {(i, j): 0.9 for i in range(3) for j in range(i + 1, 3)}
    e.update({(i, j): 0.9 for i in range(3, 6) for j in range(i + 1, 6)})
    e.update({(1, 6): to_a, (4, 6): to_b})
    return _scores(8, e)


def test_a_border_between_two_clusters_goes_to_the_higher_score():
    o = gco.cluster_scores(_two_clusters(0.6, 0.7), 0.5, 4)      # rows 1 and 4 have three neighbours, row 6 two
    assert o.core.tolist() == [False, True, False, False, True, False, False, False]
    assert o.cluster.tolist() == [0, 0, 0, 1, 1, 1, 1, -1] and o.border.sum() == 5 and abs(o.margin_border - 0.1) < 1e-12
    o = gco.cluster_scores(_two_clusters(0.7, 0.6), 0.5, 4)
    assert o.cluster.tolist() == [0, 0, 0, 1, 1, 1, 0, -1]
    o = gco.cluster_scores(_two_clusters(0.7, 0.6), 0.5, 3)      # row 6 is core now: one cluster
    assert o.cluster.tolist() == [0] * 7 + [-1] and o.n_clusters == 1


def test_an_exact_tie_goes_to_the_smaller_index():
    o = gco.cluster_scores(_two_clusters(0.65, 0.65), 0.5, 4)
    assert o.cluster[6] == 0 and o.margin_border == 0.0
    s = _scores(4, {(0, 1): 0.8, (0, 2): 0.8, (0, 3): 0.6})
    assert gco.cluster_scores(s, 0.5, 2).nn_idx.tolist() == [1, 0, 0, 0]


def test_a_nan_row_is_nobodys_neighbour():
    s = _scores(5, {(0, 1): 0.9, (1, 2): 0.9})
    s[3, :] = s[:, 3] = np.nan
    o = gco.cluster_scores(s, 0.5, 2)
    assert o.degree.tolist() == [1, 2, 1, 0, 0] and o.cluster.tolist() == [0, 0, 0, -1, -1]
    assert o.nn_idx[3] == 0 and np.isnan(o.nn_score[3]) and o.nn_idx[4] == 0 and o.nn_score[4] == 0.1    # NaN below every number
    assert gco.cluster_scores(s, 0.5, 1).cluster.tolist() == [0, 0, 0, 1, 2]
    one = gco.cluster_scores(np.ones((1, 1)), 0.5, 1)
    assert one.nn_idx.tolist() == [-1] and one.nn_score[0] == -np.inf and one.cluster.tolist() == [0]


def test_the_shared_cases_keep_their_margins():
    """What the GPU tests assert before they compare: both margins above 4 tol(512), at every min_samples they use."""
    for name, want in (("small", {1: (24, 0, 0), 3: (3, 5, 23), 4: (3, 6, 66)}), ("large", {1: (157, 0, 0), 3: (6, 13, 153), 4: (8, 17, 331)})):
        x, _ = data.case(name)
        assert x.shape == ({"small": 112, "large": 977}[name], 512)
        for ms, counts in want.items():
            o = data.oracle(name, ms)
            assert (o.n_clusters, int(o.border.sum()), int((o.cluster < 0).sum())) == counts, (name, ms)
            assert min(o.margin_t, o.margin_border) > 4 * go.tol(512)


def test_groups():
    g, noise = clustering.groups(np.array([1, -1, 0, 1, 2, -1]), ["a.png", "b.png", "c.png", "d.png", "e.png", "f.png"])
    assert g == {"0": ["c.png"], "1": ["a.png", "d.png"], "2": ["e.png"]} and list(g) == ["0", "1", "2"] and noise == ["b.png", "f.png"]
    assert clustering.groups(np.zeros(0, np.int32), []) == ({}, [])
    with pytest.raises(ValueError, match="names"):
        clustering.groups(np.array([0, 1]), ["a"])
    with pytest.raises(ValueError):
        clustering.groups(np.array([0.5, 1.0]), ["a", "b"])
    with pytest.raises(ValueError):
        clustering.groups(np.array([0, -2]), ["a", "b"])


def test_purity_report(tmp_path):
    #                    cluster 0: labels 7 7 7 9 | cluster 1: 9 9 | cluster 2: 4 5 (a tie: the smaller) | noise: 7 3
    cluster = np.array([0, 0, 0, 0, 1, 1, 2, 2, -1, -1])
    labels = np.array([7, 7, 7, 9, 9, 9, 5, 4, 7, 3])
    r = clustering.purity_report(cluster, labels)
    assert r["rows"] == 10 and r["n_clusters"] == 3 and r["noise_rows"] == [8, 9]
    assert r["clusters"]["0"] == {"size": 4, "labels": {"7": 3, "9": 1}, "majority": 7}
    assert r["clusters"]["1"] == {"size": 2, "labels": {"9": 2}, "majority": 9}
    assert r["clusters"]["2"]["majority"] == 4
    assert r["labels"]["9"] == {"rows": 3, "clusters": [0, 1], "noise": 0}              # a label spread over two clusters
    assert r["labels"]["7"] == {"rows": 4, "clusters": [0], "noise": 1} and r["labels"]["3"] == {"rows": 1, "clusters": [], "noise": 1}
    assert r["mixed_clusters"] == [0, 2]                                                 # clusters with two labels
    assert r["suspect_rows"] == [{"row": 3, "label": 9, "cluster": 0, "majority": 7}, {"row": 6, "label": 5, "cluster": 2, "majority": 4}]
    p = str(tmp_path / "r.json")
    clustering.write_report(p, r)
    assert json.load(open(p)) == r
    with pytest.raises(ValueError, match="labels"):
        clustering.purity_report(cluster, labels[:5])


def test_writers_feed_enroll(tmp_path):
    sys.path.insert(0, REPO)
    import enroll
    g, noise = clustering.groups(np.array([1, 0, -1, 1]), ["b.npz", "a.npz", "n.npz", "c.npz"])
    cj, nf = str(tmp_path / "clusters.json"), str(tmp_path / "noise.txt")
    clustering.write_groups(cj, g)
    clustering.write_noise(nf, noise)
    assert open(nf).read() == "n.npz\n"
    for stem in "abcn":
        np.savez_compressed(str(tmp_path / (stem + ".npz")), np.full((16,), ord(stem), np.float32))
    emb, labels = enroll.load_samples(str(tmp_path), cj)
    assert labels.tolist() == [0, 1, 1] and emb[:, 0].tolist() == [ord("a"), ord("b"), ord("c")]


def test_cli_refusals(tmp_path):
    sys.path.insert(0, REPO)
    import cluster
    d = tmp_path / "emb"
    d.mkdir()
    out = ["-o", str(tmp_path / "c.json")]
    for argv in (["-d", str(d)] + out,                                   # --threshold has no default
                 ["--threshold", "0.5"] + out,                           # neither -d nor -g
                 ["-d", str(d), "-g", "g.npz", "--threshold", "0.5"]):   # both
        with pytest.raises(SystemExit) as ex:
            cluster.main(argv)
        assert ex.value.code == 2
    with pytest.raises(SystemExit, match="MI355X only"):
        cluster.main(["-d", str(d), "--threshold", "0.5", "-dv", "CPU"] + out)
    for t in ("nan", "inf"):
        with pytest.raises(SystemExit, match="threshold"):
            cluster.main(["-d", str(d), "--threshold", t] + out)
    with pytest.raises(SystemExit, match="min_samples"):
        cluster.main(["-d", str(d), "--threshold", "0.5", "--min_samples", "0"] + out)
    with pytest.raises(SystemExit, match="no .npz files"):
        cluster.main(["-d", str(d), "--threshold", "0.5"] + out)
    # non-finite embeddings are refused on the host, before any device is looked for
    np.savez_compressed(str(d / "x.npz"), np.full((16,), np.nan, np.float32))
    with pytest.raises(SystemExit, match="non-finite"):
        cluster.main(["-d", str(d), "--threshold", "0.5"] + out)
    np.savez_compressed(str(d / "y.npz"), np.ones((32,), np.float32))
    with pytest.raises(SystemExit, match="values"):
        cluster.main(["-d", str(d), "--threshold", "0.5"] + out)
    assert not os.path.exists(out[1])


def test_cluster_refuses_a_cpu_gallery():
    from vn_celeb_face_recognition_amd.gallery import GalleryModel
    with pytest.raises(RuntimeError, match="MI355X only"):
        GalleryModel(16).cluster(0.5)


def test_the_abi_is_declared_and_bound():
    header = open(os.path.join(REPO, "include", "vnface.h")).read()
    for name, nargs in (("vnf_gallery_cluster_workspace_bytes", 2), ("vnf_gallery_cluster", 12)):
        m = re.search(r"\b%s\(([^;]*)\);" % name, header)
        assert m and len(m.group(1).split(",")) == nargs, name
        assert len(_lib.SIGNATURES[name][1]) == nargs
    assert _lib.SIGNATURES["vnf_gallery_cluster_workspace_bytes"][0] is ctypes.c_int64
    assert _lib.SIGNATURES["vnf_gallery_cluster"][0] is ctypes.c_int and _lib.SIGNATURES["vnf_gallery_cluster"][1][1] is ctypes.c_float
