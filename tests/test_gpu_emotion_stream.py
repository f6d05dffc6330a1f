"""GPU: emotions on the frame stream.  vnf_overlay_draw_text against its specification (tests/text_overlay_restatement.py,
itself checked against Pillow on the CPU) with zero differing bytes, VideoEncoder.write_batch(emotions=...) against
Pillow's encode of the host drawing, video.run_stream(emotions=6) against recognize_emotion, and celeb_statistic.py
--recog_emotion --track_bbox -ov end to end."""
import ast
import csv
import json
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

import jpeg_encode_restatement as E
import text_overlay_restatement as T
from conftest import GOLDEN, REPO, load_image

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NC, NP = 690, 300
K = 6


def _tags():
    return json.load(open(os.path.join(GOLDEN, "etag2idx.json")))["idx2key"]


def _noise(seed=21):
    return np.random.default_rng(seed).integers(0, 256, (3, 48, 80, 3), dtype=np.uint8)


def device_text(frames, runs, chars, ends, b=None):
    """(b,H,W,3) u8 numpy + a run table -> the painted batch through the C ABI; the bytes around the batch stay untouched"""
    from vn_celeb_face_recognition_amd import jpeg_encode
    n = frames.size
    buf = torch.full((n + 8192,), 0x5A, dtype=torch.uint8, device=DEV)
    dev = buf[4096:4096 + n].view(frames.shape)
    dev.copy_(torch.from_numpy(np.ascontiguousarray(frames)))
    runs_dev = torch.from_numpy(runs.view(np.uint8).copy()).to(DEV)
    jpeg_encode.overlay_draw_text(dev, runs_dev, torch.from_numpy(chars.copy()).to(DEV), ends)
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert (host[:4096] == 0x5A).all() and (host[4096 + n:] == 0x5A).all()
    return host[4096:4096 + n].reshape(frames.shape)


def _lines():
    tags = _tags()
    longest = next(t for t in tags if len(t) == 16) + " - 100.00%"
    assert len(longest) == 26
    return [
        (0, -9, -4, "joy - 12.34%"), (0, 60, 10, "sadness - 7.00%"), (0, 5, 42, "fear - 0.50%"), (0, 30, -3, "calm - 99.99%"),   # every edge
        (1, 500, 500, "outside - 1.00%"), (1, -300, -50, "outside - 2.00%"), (1, 2, 48, "below - 3.00%"),                    # wholly outside
        (1, 1, 20, longest),                                                                                                # the longest line
        (2, 10, 10, "affection - 50.00%"), (2, 14, 13, "fifty fluffy - 8.25%"), (2, 12, 16, "off - 100.00%"),               # on top of each other
        (3, 5, 5, "nobody - 1.00%"), (-1, 5, 5, "nobody - 2.00%"),                                                          # frames outside the batch
    ]


def test_draw_text_equals_the_restatement():
    from vn_celeb_face_recognition_amd import jpeg_encode
    frames, lines = _noise(), _lines()
    want = T.draw_runs(frames, lines)
    assert all((want[i] != frames[i]).any() for i in range(3))
    runs, chars, ends, ops, _ = jpeg_encode.text_runs(lines)
    assert ops.shape[0] == 0 and runs.shape[0] == len(lines) and len(ends) == 3      # three runs on top of each other
    got = device_text(frames, runs, chars, ends)
    assert int((got != want).sum()) == 0
    # entries the call cannot check on the host, in the first launch: an empty run, one longer than the kernel takes,
    # characters outside the buffer, a negative start, a character outside the atlas (no ink, the pen stays)
    junk = np.zeros((5,), jpeg_encode.RUN_DTYPE)
    junk[0] = (0, 5, 5, 0xFFFFFF, 0, 0)
    junk[1] = (0, 5, 5, 0xFFFFFF, 0, jpeg_encode.TEXT_RUN_MAX + 1)
    junk[2] = (0, 5, 5, 0xFFFFFF, chars.size - 3, 8)
    junk[3] = (0, 5, 5, 0xFFFFFF, -2, 4)
    junk[4] = (0, 5, 5, 0xFFFFFF, chars.size, 2)
    got = device_text(frames, np.concatenate([junk, runs]), np.concatenate([chars, np.array([7, 200], np.uint8)]), ends + 5)
    assert int((got != want).sum()) == 0
    # one run alone, default launch table; and the colour is the run's
    one = np.array([(1, 3, 7, 0x2010F0, 0, 5)], jpeg_encode.RUN_DTYPE)
    got = device_text(frames, one, np.frombuffer(b"Aj%.f", np.uint8), None)
    assert int((got != T.draw_runs(frames, [(1, 3, 7, "Aj%.f")], colour=(0xF0, 0x10, 0x20))).sum()) == 0


def test_draw_text_statuses_and_no_runs():
    from vn_celeb_face_recognition_amd import _lib, jpeg_encode
    frames = _noise()
    dev = torch.from_numpy(frames).to(DEV)
    atlas = jpeg_encode.text_atlas_device(DEV)
    runs = torch.zeros((24,), dtype=torch.uint8, device=DEV)
    lib, st = _lib.load(), _lib.current_stream_ptr()
    ends = np.array([1], np.int32)
    call = lambda fr, b, h, n, e, ne, at, ab: lib.vnf_overlay_draw_text(fr, b, h, 80, runs.data_ptr(), n, e, ne, None, 0, at, ab, st)   # noqa: E731
    assert call(dev.data_ptr(), 3, 48, 0, None, 0, atlas.data_ptr(), atlas.numel()) == 0            # n_runs = 0: no-op
    assert call(None, 0, 48, 1, None, 0, None, 0) == 0                                            # b = 0: no-op
    assert call(dev.data_ptr(), 3, 48, 1, None, 0, atlas.data_ptr(), atlas.numel()) == 0            # a zero run paints nothing
    assert call(dev.data_ptr(), 3, 48, 1, ends.ctypes.data, 1, atlas.data_ptr(), atlas.numel()) == 0
    assert call(dev.data_ptr(), 3, 48, -1, None, 0, atlas.data_ptr(), atlas.numel()) == -1
    assert call(None, 3, 48, 1, None, 0, atlas.data_ptr(), atlas.numel()) == -1
    assert call(dev.data_ptr(), 3, 0, 1, None, 0, atlas.data_ptr(), atlas.numel()) == -1
    assert call(dev.data_ptr(), 3, 48, 1, None, 0, None, 0) == -1                                  # no atlas
    assert call(dev.data_ptr(), 3, 48, 1, None, 0, atlas.data_ptr(), 4) == -1                      # not even its header
    assert call(dev.data_ptr(), 3, 48, 1, None, 0, atlas.data_ptr() + 1, atlas.numel() - 1) == -1  # misaligned
    assert call(dev.data_ptr(), 3, 48, 2, ends.ctypes.data, 1, atlas.data_ptr(), atlas.numel()) == -1   # launches end at 1 of 2 runs
    bad = np.array([1, 1], np.int32)
    assert call(dev.data_ptr(), 3, 48, 1, bad.ctypes.data, 2, atlas.data_ptr(), atlas.numel()) == -1    # an empty launch
    torch.cuda.synchronize()
    assert np.array_equal(dev.cpu().numpy(), frames)
    jpeg_encode.draw_emotions_device(dev, [[], [], []], [[], [], []], [[], [], []])
    torch.cuda.synchronize()
    assert np.array_equal(dev.cpu().numpy(), frames)


def _faces(seed=4):
    """boxes, names, tag indices and probabilities for a batch of three 48x80 frames: two faces that overlap on frame
    0, none on frame 1, one at the edge on frame 2"""
    rng = np.random.default_rng(seed)
    boxes = [[np.array([3.4, 2.6, 50.2, 44.9], np.float32), np.array([20.5, 10.1, 78.8, 46.0], np.float32)], [],
             [np.array([-6.5, 20.3, 40.0, 60.7], np.float32)]]
    names = [["celeb_1", "Unknown"], [], ["celeb_22"]]
    idx = [rng.integers(0, NC, (len(b), 3)) for b in boxes]
    prob = [np.sort(rng.random((len(b), 3)).astype(np.float32), axis=1)[:, ::-1].copy() for b in boxes]
    return boxes, names, idx, prob


def _host_drawing(frames, boxes, names, idx, prob):
    from vn_celeb_face_recognition_amd.cli_utils import draw_boxes_on_image, draw_emotions
    tags = _tags()
    out = []
    for f, fr in enumerate(frames):
        img = draw_boxes_on_image(fr, boxes[f], names[f]) if names[f] else fr
        if names[f]:
            img = draw_emotions(img, boxes[f], [[tags[int(i)] for i in face] for face in idx[f]], prob[f])
        out.append(img)
    return np.stack(out)


def test_text_after_boxes_equals_draw_boxes_then_draw_emotions():
    from vn_celeb_face_recognition_amd import jpeg_encode
    frames = _noise(8)
    boxes, names, idx, prob = _faces()
    tags = _tags()
    want = _host_drawing(frames, boxes, names, idx, prob)
    dev = torch.from_numpy(frames).to(DEV)
    jpeg_encode.draw_annotations_device(dev, boxes, names, [[[tags[int(i)] for i in face] for face in fr] for fr in idx], prob)
    torch.cuda.synchronize()
    assert int((dev.cpu().numpy() != want).sum()) == 0 and (want[0] != frames[0]).any() and np.array_equal(want[1], frames[1])
    # a frame with a tag outside the atlas goes through the LABEL path; the batch is Pillow's all the same
    odd = [[["buồn", "sầu", "sad"], [")a", "surprise", "c"]], [], [["x", "y", "z"]]]   # 's', ')' start left of the pen
    from vn_celeb_face_recognition_amd.cli_utils import draw_boxes_on_image, draw_emotions
    want = np.stack([draw_emotions(draw_boxes_on_image(frames[f], boxes[f], names[f]), boxes[f], odd[f], prob[f]) if names[f] else frames[f]
                     for f in range(3)])
    dev = torch.from_numpy(frames).to(DEV)
    jpeg_encode.draw_annotations_device(dev, boxes, names, odd, prob)
    torch.cuda.synchronize()
    assert int((dev.cpu().numpy() != want).sum()) == 0


def test_write_batch_with_emotions_writes_pillows_files(tmp_path):
    from vn_celeb_face_recognition_amd.jpeg_encode import VideoEncoder
    from vn_celeb_face_recognition_amd.mjpeg_avi import read_mjpeg_avi
    frames = _noise(9)
    boxes, names, idx, prob = _faces()
    want = _host_drawing(frames, boxes, names, idx, prob)
    path = str(tmp_path / "out.avi")
    enc = VideoEncoder(path, 2.0, DEV, 92, "4:2:0", idx2tag=dict(enumerate(_tags())))
    enc.write_batch(torch.from_numpy(frames).to(DEV), [1, 3, 5], boxes, names, emotions=list(zip(idx, prob)))
    enc.close()
    fps, got, n = read_mjpeg_avi(path)
    assert n == 3 and fps == 2.0
    for i in range(3):
        assert got.compressed(i) == E.pillow_jpeg(want[i], 92, E.S420), i


# ------------------------------------------------------------------------------------------------ the stream
def _stream_frames():
    """six 360 x 640 frames: the picture scaled to the frame's height on a grey canvas, its mirror image, one blank"""
    from PIL import Image
    pic = Image.fromarray(load_image("mrDam_HaHo_recog.jpg"))
    w = pic.width * 360 // pic.height
    a = np.full((360, 640, 3), 96, np.uint8)
    a[:, 40:40 + w] = np.asarray(pic.resize((w, 360), Image.BILINEAR))
    flip = np.ascontiguousarray(a[:, ::-1])
    return [a, flip, np.zeros_like(a), flip, a, flip]


def test_run_stream_carries_the_pipelines_emotions(tmp_path):
    from test_gpu_emotion import _model
    from vn_celeb_face_recognition_amd import models
    from vn_celeb_face_recognition_amd.cli_utils import open_frame_source
    from vn_celeb_face_recognition_amd.mjpeg_avi import read_mjpeg_avi, write_mjpeg_avi
    from vn_celeb_face_recognition_amd.pipeline import (FacePipeline, center_point_dict, parallel_detect_and_align,
                                                        recognize_emotion, trans_emotion_inf)
    from vn_celeb_face_recognition_amd.video import run_stream, tracker_row
    vin = str(tmp_path / "in.avi")
    write_mjpeg_avi(vin, _stream_frames(), 25.0, quality=97)
    _, decoded, n = read_mjpeg_avi(vin)
    assert n == 6
    det = models.MTCNN(keep_all=True, min_face_size=40, device=DEV, max_batch=2, max_height=360, max_width=640)
    enc = models.InceptionResnetV1(pretrained=None, max_batch=16).to(DEV).eval()
    clf = models.MLPModel(512, 1001).to(DEV).eval()
    l2n = {"label": list(range(1001)), "name": ["c%d" % i for i in range(1001)]}
    emo = _model("f16x2", max_batch=1)                           # below a batch's faces: the handle works in chunks
    # the reference, once: the stream's two distinct pictures (frames 1 and 2; 4, 5, 6 repeat them, 3 is blank)
    pics = [np.asarray(decoded[0]), np.asarray(decoded[1])]
    faces, _ = parallel_detect_and_align(pics, det, center_point_dict["(160, 160)"], (160, 160))
    tags, probs = recognize_emotion(faces, DEV, emo, trans_emotion_inf, np.vectorize(lambda i: int(i)), topk=K)
    which = {1: 0, 2: 1, 4: 1, 5: 0, 6: 1}
    assert all(len(f) >= 1 for f in faces), [len(f) for f in faces]

    def run(decode):
        seen = {}

        def row(tm, num, names, boxes, shape, emotions=None):
            seen[num] = emotions
            return tracker_row(tm, num, names, boxes, shape)
        pipe = FacePipeline(det, enc, clf, l2n, 160, 0.0, emotion=emo, topk_emotions=K)
        rows, processed = run_stream(open_frame_source(vin), pipe, 2, 0, 1, device=DEV, decode=decode, emotions=K, row=row)
        assert processed == 6 and sorted(rows) == sorted(seen) == [1, 2, 3, 4, 5, 6]
        return rows, seen
    rows, seen = run("device")
    for num in range(1, 7):
        idx, prob = seen[num]
        if num == 3:
            assert idx.shape == (0, K) and prob.shape == (0, K) and rows[3].endswith(',"[]",3,"[]"\n')
            continue
        w = which[num]
        err = float(np.abs(prob - np.asarray(probs[w])).max())
        print("frame %d: emotion indices %s, max probability error %.3e" % (num, idx.tolist(), err))
        assert idx.dtype == np.int64 and np.array_equal(idx, np.asarray(tags[w]))
        assert err <= 1e-6
    rows_h, seen_h = run("host")
    assert rows_h == rows
    for num in range(1, 7):
        assert np.array_equal(seen_h[num][0], seen[num][0]) and np.array_equal(seen_h[num][1], seen[num][1])
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ the CLI
def _emotion_files(tmp_path):
    from test_gpu_cli import _classifier_files
    from vn_celeb_face_recognition_amd.weights import generate_state_dict
    ck, l2n = _classifier_files(tmp_path)
    sd = generate_state_dict("rn50_2b", 0, as_torch=True, num_classes=NC, num_projections=NP)
    eck = str(tmp_path / "emotion.pth")
    torch.save({"epoch": 9, "state_dict": {"module." + k: v for k, v in sd.items()}}, eck)
    eargs = str(tmp_path / "emotion.json")
    with open(eargs, "w") as f:
        json.dump({"pretrained": False, "num_classes": NC, "checkpoint_path": eck, "max_batch": 8}, f)
    names = _tags()
    t2i = str(tmp_path / "etag2idx.pkl.keep")
    with open(t2i, "wb") as f:
        pickle.dump({"key2idx": {n: i for i, n in enumerate(names)}, "idx2key": dict(enumerate(names))}, f)
    return ck, l2n, eargs, t2i


def test_celeb_statistic_cli_with_emotions_and_device_video(tmp_path):
    """celeb_statistic.py --recog_emotion --track_bbox -ov out.avi on a 6-frame Motion-JPEG AVI at 4 fps, -fidx 1 3:
    frames 1, 3 (blank) and 5 are sampled -- the others are never decoded --, the tracker gains the Emotion column, the
    JSON the 'emotions', the re-use branch needs no GPU, and the video holds the three sampled frames at 2 per second."""
    from vn_celeb_face_recognition_amd.mjpeg_avi import read_mjpeg_avi, write_mjpeg_avi
    ck, l2n, eargs, t2i = _emotion_files(tmp_path)
    a = load_image("mrDam_HaHo_recog.jpg")
    flip, blank, other = np.ascontiguousarray(a[:, ::-1]), np.zeros_like(a), np.ascontiguousarray(255 - a[::-1])
    vin = str(tmp_path / "in.avi")
    write_mjpeg_avi(vin, [a, other, blank, other, flip, other], 4.0, quality=97)
    vout, trk, jst = str(tmp_path / "out.avi"), str(tmp_path / "tracker.csv"), str(tmp_path / "t.json")
    common = ["-i", vin, "-fidx", "1", "3", "-m", ck, "-l2n", l2n, "-enc", "InceptionResnetV1", "-eargs",
              os.path.join(REPO, "cfg/embedding/inception_resnet_v1.json"), "-tg_fs", "160", "--inference_method", "par_fd_vs_aln",
              "-dargs", os.path.join(REPO, "cfg/detection/mtcnn.json"), "--track_bbox", "--recog_threshold", "0.0", "-tap", "1", "-ign", "nobody",
              "-nvi", "1", "--n_frames", "2", "-o", str(tmp_path / "of"), "-ot", trk, "-jst", jst,
              "--recog_emotion", "-emtargs", eargs, "-t2i", t2i, "--topk_emotions", str(K), "-ov", vout]
    env = dict(os.environ, PYTHONPATH=REPO)
    r = subprocess.run([sys.executable, os.path.join(REPO, "celeb_statistic.py")] + common, cwd=str(tmp_path), env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Create tracker file" in r.stdout and "Loaded emotion model from checkpoint path" in r.stdout
    assert "Save exported video in" in r.stdout
    rows = list(csv.reader(open(trk)))
    assert rows[0] == ["Time", "Names", "Frame_idx", "Bboxes", "Emotion"]
    assert [int(x[2]) for x in rows[1:]] == [1, 3, 5] and [x[0] for x in rows[1:]] == ["0.25", "0.75", "1.25"]
    tags = set(_tags())
    for x in rows[1:]:
        names, boxes, emotions = ast.literal_eval(x[1]), ast.literal_eval(x[3]), ast.literal_eval(x[4])
        assert "np." not in x[4] and len(names) == len(boxes) == len(emotions) == (0 if x[2] == "3" else 2)
        assert all(type(face) is list and len(face) == K and all(type(t) is str and t in tags for t in face) for face in emotions)
    assert rows[2][4] == "[]"
    stat = json.load(open(jst))
    carried = [b["emotions"] for v in stat["1"]["celebrities"].values() for b in v]
    assert len(carried) == 4 and all(len(e) == K and set(e) <= tags for e in carried)
    assert sorted(map(tuple, carried)) == sorted(tuple(e) for x in rows[1:] for e in ast.literal_eval(x[4]))
    # the video: the sampled frames alone, as many per second as -fidx keeps; the blank one went through untouched
    fps, got, n = read_mjpeg_avi(vout)
    _, src, _ = read_mjpeg_avi(vin)
    assert n == 3 and fps == 2.0
    assert got.compressed(1) == E.pillow_jpeg(np.asarray(src[2]), 92, E.S420)
    import io
    from PIL import Image
    for i, k in ((0, 0), (2, 4)):
        # the encoder is Pillow's byte for byte, so against Pillow's encode of the plain source frame only the 16 x 16
        # blocks the drawing touches can differ: some do (it is annotated), most do not (it is that frame: another
        # frame of the stream differs everywhere)
        plain = E.pillow_jpeg(np.asarray(src[k]), 92, E.S420)
        assert got.compressed(i) != plain
        differs = (np.asarray(got[i]) != np.asarray(Image.open(io.BytesIO(plain)).convert("RGB"))).any(axis=2)
        assert 0.0 < differs.mean() < 0.5, differs.mean()
    assert os.listdir(tmp_path / "of") == [] and not [f for f in os.listdir(tmp_path) if f.endswith(".part")]
    # the re-use branch (celeb_statistic.py:393-399) reproduces the JSON without a GPU
    first = open(jst).read()
    os.remove(jst)
    r2 = subprocess.run([sys.executable, os.path.join(REPO, "celeb_statistic.py")] + common, cwd=str(tmp_path),
                        env=dict(env, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES=""), capture_output=True, text=True, timeout=600)
    assert r2.returncode == 0, r2.stdout + r2.stderr
    assert "Re-use tracker file" in r2.stdout and open(jst).read() == first
