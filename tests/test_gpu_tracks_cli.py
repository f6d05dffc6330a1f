"""GPU: celeb_statistic.py --track_faces end to end (generator weights, as test_gpu_cli.py), with an MLP checkpoint and
with -m gallery.npz.  The stream: three identical frames of mrDam_HaHo_recog.jpg, a black frame, the picture twice more,
then another picture.  Identical frames give identical embeddings, so the faces of a run of them are each other's best
candidates at cosine 1 whatever the weights are; what is linked across the change of picture is not assumed but taken from
tracking.link_tracks on the embeddings the test computes itself."""
import ast
import csv
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, REPO, load_image
from test_gpu_cli import _classifier_files

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PIC, OTHER = "mrDam_HaHo_recog.jpg", "hoai_linh_4_recog.jpg"
ENC_ARGS = os.path.join(REPO, "cfg/embedding/inception_resnet_v1.json")
DET_ARGS = os.path.join(REPO, "cfg/detection/mtcnn.json")
NUMBERS = [1, 2, 3, 4, 5, 6, 7]
SCRIPT = os.path.join(REPO, "celeb_statistic.py")


def _cli(args, cwd):
    return subprocess.run([sys.executable, SCRIPT] + args, cwd=cwd, env=dict(os.environ, PYTHONPATH=REPO), capture_output=True, text=True,
                          timeout=600)


def _run(args, cwd):
    r = _cli(args, cwd)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """The stream as a .npy file, its faces embedded the way the CLI embeds them, and the two kinds of classifier."""
    from vn_celeb_face_recognition_amd import models
    from vn_celeb_face_recognition_amd.cli_utils import read_json, read_label2name
    from vn_celeb_face_recognition_amd.classifier import load_model_classify
    from vn_celeb_face_recognition_amd.pipeline import FacePipeline
    tmp = tmp_path_factory.mktemp("tracks_cli")
    other = load_image(OTHER)
    a = np.zeros_like(other)
    pic = load_image(PIC)
    a[:pic.shape[0], :pic.shape[1]] = pic
    frames = np.stack([a, a, a, np.zeros_like(a), a, a, other])
    npy = str(tmp / "stream.npy")
    np.save(npy, frames)
    det_args = read_json(DET_ARGS)
    det_args["device"] = DEV
    det = models.MTCNN(**det_args).eval()
    enc = models.InceptionResnetV1(**read_json(ENC_ARGS)).to(DEV)
    counts, boxes, emb = FacePipeline(det, enc, None, None, 160).embed_frames(torch.from_numpy(frames).to(DEV))
    emb, counts = emb.cpu().numpy(), [int(c) for c in counts]
    assert counts[0] >= 2 and counts[:6] == [counts[0]] * 3 + [0] + [counts[0]] * 2 and counts[6] >= 1
    ck, l2n = _classifier_files(tmp)
    mlp = load_model_classify(ck, models.MLPModel(512, 1001)).to(DEV)
    gal_path = str(tmp / "gallery.npz")
    labels = np.arange(counts[0]) + 10
    models.GalleryModel(512).to(DEV).add(emb[:counts[0]], labels).save(gal_path)
    gl2n = tmp / "gallery_l2n.csv"
    gl2n.write_text("label,name\n" + "".join("%d,person_%d\n" % (l, l) for l in labels))
    gallery = models.GalleryModel.load(gal_path).to(DEV)
    common = ["-i", npy, "-fps", "4", "-fidx", "0", "1", "2", "3", "-enc", "InceptionResnetV1", "-eargs", ENC_ARGS, "-tg_fs", "160",
              "--inference_method", "par_fd_vs_aln", "-dargs", DET_ARGS, "--track_bbox", "-tap", "1", "-nvi", "2", "--n_frames", "2"]
    kinds = {"mlp": dict(flags=["-m", ck, "-l2n", l2n, "--recog_threshold", "0.0"], clf=mlp, l2n=read_label2name(l2n),
                         thr={str(i): 0.0 for i in range(1001)}),
             "gallery": dict(flags=["-m", gal_path, "-l2n", str(gl2n), "--recog_threshold", "0.9"], clf=gallery, l2n=read_label2name(str(gl2n)),
                             thr={str(i): 0.9 for i in range(gallery.num_classes)})}
    frame_of = np.repeat(np.arange(7), counts)
    return dict(tmp=tmp, common=common, kinds=kinds, counts=counts, emb=emb, boxes=np.asarray(boxes, np.float32), frame_of=frame_of,
                shape=a.shape, runs={})


def _tracker(world, kind, tag, extra):
    """one run of the CLI -> (csv rows as dicts, the json text, stdout); a run another test has made already is not repeated"""
    if (kind, tag) not in world["runs"]:
        world["runs"][(kind, tag)] = _tracker_run(world, kind, tag, extra)
    return world["runs"][(kind, tag)]


def _tracker_run(world, kind, tag, extra):
    tmp = world["tmp"]
    trk, js = str(tmp / ("%s_%s.csv" % (kind, tag))), str(tmp / ("%s_%s.json" % (kind, tag)))
    out = _run(world["common"] + world["kinds"][kind]["flags"] + ["-o", str(tmp / "of"), "-ot", trk, "-jst", js] + extra, str(tmp))
    assert "Create tracker file" in out
    rows = list(csv.DictReader(open(trk)))
    assert [int(r["Frame_idx"]) for r in rows] == NUMBERS
    return rows, open(js).read(), out


def _expected(world, kind, gap, threshold=0.5):
    """tracks and track names of the test's own embeddings through tracking.py"""
    from vn_celeb_face_recognition_amd import tracking
    k = world["kinds"][kind]
    res = tracking.link_tracks(world["emb"], world["frame_of"], world["boxes"], threshold=threshold, max_gap=gap, device=DEV)
    names = tracking.name_tracks(tracking.pool_tracks(world["emb"], res), k["clf"], k["l2n"], k["thr"])
    return res, names


def _check_tracked(world, kind, rows, gap):
    c = world["counts"][0]
    tracks = [ast.literal_eval(r["Track"]) for r in rows]
    names = [ast.literal_eval(r["Names"]) for r in rows]
    assert [len(t) for t in tracks] == world["counts"] == [len(n) for n in names]
    # a run of identical frames: one track id per face, the same list in every row of the run
    assert tracks[0] == tracks[1] == tracks[2] == list(range(c)) and tracks[3] == [] and tracks[4] == tracks[5] and len(set(tracks[4])) == c
    if gap == 1:
        assert not set(tracks[4]) & set(tracks[0])                       # the black frame breaks the tracks
    else:
        assert tracks[4] == tracks[0]                                    # and --track_gap 2 joins them
    by_track = {}
    for t, n in zip(sum(tracks, []), sum(names, [])):
        by_track.setdefault(t, set()).add(n)
    assert all(len(v) == 1 for v in by_track.values())                   # one name per track
    res, want = _expected(world, kind, gap)
    assert sorted(by_track) == list(range(res.n_tracks))
    # the CLI's faces against the test's: the same frame, the nearest box
    h, w = world["shape"][:2]
    for r, (row, t_row, n_row) in enumerate(zip(rows, tracks, names)):
        mine = np.flatnonzero(world["frame_of"] == r)
        for box, t, n in zip(ast.literal_eval(row["Bboxes"]), t_row, n_row):
            d = np.abs(world["boxes"][mine] - np.array(box, np.float32) * np.array([w, h, w, h], np.float32)).sum(axis=1)
            i = int(mine[np.argmin(d)])
            assert d.min() < 2.0 and res.track[i] == t and want[res.track[i]] == n, (r, box, t, n)
    return by_track


@pytest.mark.parametrize("kind", ["mlp", "gallery"])
def test_tracks_follow_the_runs_of_identical_frames(world, kind):
    rows1, _, out = _tracker(world, kind, "gap1", ["--track_faces", "--track_threshold", "0.5", "--track_gap", "1"])
    assert list(rows1[0]) == ["Time", "Names", "Frame_idx", "Bboxes", "Track"] and "Linked %d faces into" % sum(world["counts"]) in out
    _check_tracked(world, kind, rows1, 1)
    rows2, _, _ = _tracker(world, kind, "gap2", ["--track_faces", "--track_threshold", "0.5", "--track_gap", "2"])
    named = _check_tracked(world, kind, rows2, 2)
    if kind == "gallery":                                                # the enrolled faces come back under their own names
        assert [named[t] for t in range(world["counts"][0])] == [{"person_%d" % (10 + i)} for i in range(world["counts"][0])]


@pytest.mark.parametrize("kind", ["mlp", "gallery"])
def test_a_threshold_nobody_meets_changes_nothing_but_the_column(world, kind):
    plain, plain_js, _ = _tracker(world, kind, "plain", [])
    assert list(plain[0]) == ["Time", "Names", "Frame_idx", "Bboxes"]
    rows, js, _ = _tracker(world, kind, "alone", ["--track_faces", "--track_threshold", "2.0"])
    for col in ("Time", "Names", "Frame_idx", "Bboxes"):
        assert [r[col] for r in rows] == [r[col] for r in plain], col
    assert sum((ast.literal_eval(r["Track"]) for r in rows), []) == list(range(sum(world["counts"])))    # every face its own track
    assert json.loads(js) == json.loads(plain_js)


def test_reuse_refusals_and_the_parser(world):
    tmp = world["tmp"]
    rows, js, _ = _tracker(world, "mlp", "gap1", ["--track_faces", "--track_threshold", "0.5", "--track_gap", "1"])
    trk, jp = str(tmp / "mlp_gap1.csv"), str(tmp / "mlp_gap1.json")
    os.remove(jp)
    base = world["common"] + world["kinds"]["mlp"]["flags"] + ["-o", str(tmp / "of"), "-jst", jp]
    out = _run(base + ["-ot", trk], str(tmp))                            # the re-use branch reads the file with its Track column
    assert "Re-use tracker file" in out and open(jp).read() == js
    fresh = ["-ot", str(tmp / "never.csv")]
    for flags in (["-ov", str(tmp / "v.avi")], ["-sfr"]):
        r = _cli(base + fresh + ["--track_faces", "--track_threshold", "0.5"] + flags, str(tmp))
        assert r.returncode != 0 and "--track_faces" in r.stderr and "-ov" in r.stderr and "-sfr" in r.stderr
    r = _cli(base + fresh + ["--track_faces"], str(tmp))
    assert r.returncode == 2 and "--track_threshold" in r.stderr         # argparse's error
    assert not os.path.exists(tmp / "never.csv")
