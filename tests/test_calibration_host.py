"""CPU: gallery calibration's host layer -- the threshold / FAR / DIR / per-class statistics on hand-made scores (beside the
plain-loop oracle gallery_calibration_oracle.py), the thresholds.json round trip into identify_names, calibrate.py's
refusals, and the new ABI's declarations."""
import ctypes
import json
import os
import re
import sys

import numpy as np
import pytest

from conftest import REPO

import gallery_calibration_oracle as gco
from vn_celeb_face_recognition_amd import _lib, calibration as cal, statistics
from vn_celeb_face_recognition_amd.pipeline import identify_names


def _scores(m, n, n_label, probe_label, m_idx=None, n_idx=None):
    """Scores from per-probe mate / non-mate scores; None: absent.  Row indices default to distinct made-up ones."""
    f = len(m)
    idx = np.full((f, 2), -1, np.int64)
    lab = np.full((f, 2), -1, np.int64)
    sc = np.full((f, 2), -np.inf, np.float32)
    for p in range(f):
        if m[p] is not None:
            idx[p, 0], lab[p, 0], sc[p, 0] = (2 * p if m_idx is None else m_idx[p]), probe_label[p], m[p]
        if n[p] is not None:
            idx[p, 1], lab[p, 1], sc[p, 1] = (2 * p + 1 if n_idx is None else n_idx[p]), n_label[p], n[p]
    return cal.Scores(idx, lab, sc, probe_label)


def _same_as_oracle(sc, far, nc):
    local, rep = cal.calibrate(sc, far, nc)
    want = gco.calibrate(sc.idx, sc.label, sc.score, sc.probe_labels, far, nc)
    assert (rep["thr"], rep["Fm"], rep["Fn"], rep["achieved_far"], rep["dir"], rep["rank1"]) == \
        (want["thr"], want["Fm"], want["Fn"], want["far"], want["dir"], want["rank1"])
    assert local == want["local"] and list(local) == [str(c) for c in range(nc)]
    return local, rep


def test_ties_at_the_cut_stay_out():
    sc = _scores([0.95] * 4, [0.9, 0.8, 0.8, 0.5], [1, 1, 1, 1], [0, 0, 0, 0])
    above = float(np.nextafter(np.float32(0.8), np.float32(1)))
    for far, a in ((0.25, 1), (0.5, 2)):      # the 2nd and the 3rd largest are both 0.8: neither 0.8 may pass
        local, rep = _same_as_oracle(sc, far, 2)
        assert cal.accepted_impostors(4, far) == a
        assert rep["thr"] == above and rep["achieved_far"] == 0.25 and rep["achieved_far"] * 4 <= a
    _, rep = _same_as_oracle(sc, 0.75, 2)      # a = 3: the 4th largest is 0.5, and the three above it pass
    assert rep["thr"] == float(np.nextafter(np.float32(0.5), np.float32(1))) and rep["achieved_far"] == 0.75


def test_far_zero_lets_no_impostor_pass():
    sc = _scores([0.7, 0.99, 0.6], [0.6, 0.3, 0.6], [1, 0, 1], [0, 1, 0])
    local, rep = _same_as_oracle(sc, 0.0, 2)
    assert rep["thr"] == float(np.nextafter(np.float32(0.6), np.float32(1))) and rep["achieved_far"] == 0.0
    assert rep["operating_points"] == []                       # 0.1 * 3 < 1: no impostor may pass at any listed FAR
    # class 1 attracted the two 0.6 strangers, class 0 the 0.3 one: both end at the global threshold (the maximum)
    assert local == {"0": rep["thr"], "1": rep["thr"]}
    assert rep["rank1"] == 1.0 and rep["dir"] == 2 / 3         # the third probe's mate (0.6) is below the threshold


def test_far_times_fn_on_an_integer():
    assert 0.29 * 100 < 29                                     # in doubles; the rule's 1e-9 puts it back on 29
    n = [np.float32(i) / np.float32(100) for i in range(100)]
    sc = _scores([1.0] * 100, n, [1] * 100, [0] * 100)
    assert cal.accepted_impostors(100, 0.29) == 29
    _, rep = _same_as_oracle(sc, 0.29, 2)
    assert rep["thr"] == float(np.nextafter(np.float32(70) / np.float32(100), np.float32(1))) and rep["achieved_far"] == 0.29
    pts = {p["far"]: p for p in rep["operating_points"]}
    assert sorted(pts) == [0.01, 0.1] and pts[0.1]["achieved_far"] == 0.1 and pts[0.01]["achieved_far"] == 0.01
    assert all(p["dir"] == 1.0 for p in pts.values())


def test_no_non_mates_gives_minus_one_and_says_so():
    sc = _scores([0.9, 0.8], [None, None], [0, 0], [0, 0])
    local, rep = _same_as_oracle(sc, 0.01, 3)
    assert rep["thr"] == -1.0 and rep["Fn"] == 0 and rep["Fm"] == 2 and rep["achieved_far"] == 0.0
    assert local == {"0": -1.0, "1": -1.0, "2": -1.0}
    assert any("non-mate" in note for note in rep["notes"])
    assert rep["dir"] == 1.0 and rep["rank1"] == 1.0           # an absent non-mate is outranked


def test_probes_without_mates_and_a_class_that_attracted_nobody():
    #          mate   non-mate  its label  probe label
    rows = [(0.90, 0.40, 1, 0),
            (None, 0.70, 1, 5),      # a stranger (label 5 is not enrolled): no mate
            (0.50, 0.60, 0, 1),      # misidentified: the non-mate outranks the mate
            (0.65, 0.65, 1, 0),      # an exact tie, mate at the smaller index: the mate outranks
            (None, 0.20, 0, 5)]
    m, n, nl, pl = zip(*rows)
    sc = _scores(m, n, nl, pl, m_idx=[0, -1, 7, 2, -1], n_idx=[9, 9, 1, 9, 1])
    local, rep = _same_as_oracle(sc, 0.2, 3)                   # a = 1: thr above the 2nd largest non-mate, 0.65
    up = lambda v: float(np.nextafter(np.float32(v), np.float32(1)))
    assert (rep["Fm"], rep["Fn"], rep["F"]) == (3, 5, 5) and rep["thr"] == up(0.65) and rep["achieved_far"] == 0.2
    assert rep["rank1"] == 2 / 3
    # class 1 attracted 0.40, 0.70, 0.65 (a = 0): above 0.70; class 0 attracted 0.60, 0.20 (a = 0): above 0.60, raised to
    # thr; class 2 attracted nobody: thr
    assert local == {"0": up(0.65), "1": up(0.70), "2": up(0.65)}
    assert rep["dir"] == 1 / 3                                 # probe 0 alone: probe 3's 0.65 is below its class's threshold
    sc2 = _scores(m, n, nl, pl, m_idx=[0, -1, 7, 9, -1], n_idx=[9, 9, 1, 2, 1])   # the tie the other way round
    assert cal.calibrate(sc2, 0.2, 3)[1]["rank1"] == 1 / 3 == gco.calibrate(sc2.idx, sc2.label, sc2.score, sc2.probe_labels, 0.2, 3)["rank1"]


def test_random_scores_equal_the_oracle():
    rng = np.random.default_rng(3)
    f, nc = 400, 9
    pl = rng.integers(0, nc + 2, f)
    m = [None if (l >= nc or rng.random() < 0.1) else np.float32(rng.uniform(0.2, 1.0)) for l in pl]
    n = [np.float32(np.round(rng.uniform(-0.2, 0.8), 2)) for _ in pl]          # two decimals: plenty of exact ties
    nl = [int((l + 1 + rng.integers(0, nc - 2)) % (nc - 1)) for l in pl]       # class nc - 1 attracts nobody
    sc = _scores(m, n, nl, pl)
    for far in (0.0, 0.001, 0.01, 0.1, 0.5):
        local, rep = _same_as_oracle(sc, far, nc)
        assert rep["achieved_far"] <= far and local[str(nc - 1)] == rep["thr"] and min(local.values()) == rep["thr"]
    assert [p["far"] for p in rep["operating_points"]] == [0.1, 0.01]          # 0.001 * 400 < 1


def test_thresholds_json_round_trip_is_exact(tmp_path):
    s = np.float32(0.1) * np.float32(7.3)                      # no short decimal form
    sc = _scores([0.9, 0.9, 0.9], [s, 0.2, 0.3], [1, 0, 0], [0, 1, 1])
    local, rep = cal.calibrate(sc, 0.0, 3)
    p = str(tmp_path / "thresholds.json")
    cal.write_thresholds(p, local)
    back = statistics.build_thresholds(p, 3, 0.7)
    assert back == local == json.load(open(p)) and all(type(v) is float for v in back.values())
    thr1 = np.float32(back["1"])
    assert float(thr1) == back["1"] and thr1 == np.nextafter(s, np.float32(1))      # the float32 survives the text
    df = {"label": [0, 1, 2], "name": ["a", "b", "c"]}
    at, below = thr1, np.nextafter(thr1, np.float32(-1))
    assert below == s
    names = identify_names(np.array([1, 1], np.int32), np.array([at, below], np.float32), 3, df, back)
    assert names == ["b", "Unknown"]                           # exactly at the threshold: accepted; one ulp below: refused
    assert identify_names(np.array([1], np.int32), np.array([at], np.float32), 3, df, rep["thr"]) == ["b"]


def _gallery_file(path, mode):
    x = np.random.default_rng(0).standard_normal((3, 16))
    emb = (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
    d = dict(embeddings=emb, labels=np.array([1, 4, 9], np.int64), mode=np.array(mode), num_classes=np.array(10, np.int64))
    if mode == "centroid":
        d.update(sums=emb.copy(), counts=np.ones(3, np.int64))
    np.savez(path, **d)


def test_cli_refusals(tmp_path):
    sys.path.insert(0, REPO)
    import calibrate
    cg, ag = str(tmp_path / "c.npz"), str(tmp_path / "a.npz")
    _gallery_file(cg, "centroid")
    _gallery_file(ag, "all")
    out = ["-o", str(tmp_path / "t.json"), "-r", str(tmp_path / "r.json")]
    with pytest.raises(SystemExit, match="centroid"):
        calibrate.main(["-g", cg, "--self"] + out)
    with pytest.raises(SystemExit, match="MI355X only"):
        calibrate.main(["-g", ag, "--self", "-dv", "CPU"] + out)
    for far in ("1", "1.5", "-0.01", "nan"):
        with pytest.raises(SystemExit, match="far"):
            calibrate.main(["-g", ag, "--self", "--far", far] + out)
    # non-finite probes are refused on the host, before any device is looked for
    d = tmp_path / "emb"
    d.mkdir()
    np.savez_compressed(str(d / "x.npz"), np.full((16,), np.nan, np.float32))
    lj = tmp_path / "l.json"
    lj.write_text(json.dumps({"1": ["x.png"]}))
    with pytest.raises(SystemExit, match="non-finite"):
        calibrate.main(["-g", ag, "-d", str(d), "-l", str(lj)] + out)
    assert not os.path.exists(out[1]) and not os.path.exists(out[3])
    with pytest.raises(ValueError):
        cal.check_far(1.0)


def test_mated_search_refusals_on_the_host():
    import torch
    from vn_celeb_face_recognition_amd.gallery import GalleryModel
    g = GalleryModel(16)
    with pytest.raises(RuntimeError, match="MI355X only"):
        g.mated_search(torch.ones((2, 16)), [0, 1])


def test_the_abi_is_declared_and_bound():
    header = open(os.path.join(REPO, "include", "vnface.h")).read()
    for name, nargs in (("vnf_gallery_mated_search_workspace_bytes", 3), ("vnf_gallery_mated_search", 12)):
        m = re.search(r"\b%s\(([^;]*)\);" % name, header)
        assert m and len(m.group(1).split(",")) == nargs, name
        res, args = _lib.SIGNATURES[name]
        assert len(args) == nargs
    assert _lib.SIGNATURES["vnf_gallery_mated_search_workspace_bytes"][0] is ctypes.c_int64
    assert _lib.SIGNATURES["vnf_gallery_mated_search"][0] is ctypes.c_int
