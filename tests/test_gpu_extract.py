"""GPU: vnf_extract_faces and the host API on top of it (MTCNN.forward / extract, extract_face, crop_face.py) against the CPU
restatement (crop_rects + interpolate(mode="area").byte()) and the reference-made golden file, byte for byte."""
import ctypes
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

import extract_golden as eg
from conftest import GOLDEN, REPO

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _frames(shape, seed):
    return np.random.RandomState(seed).randint(0, 256, size=shape, dtype=np.uint8)


def _run(frames, rects, s, **kw):
    from vn_celeb_face_recognition_amd.detector import extract_faces_device
    fd = frames if isinstance(frames, torch.Tensor) else torch.from_numpy(frames).to(DEV)
    x, u8 = extract_faces_device(fd, np.asarray(rects, np.int32), s, want_u8=True, **kw)
    torch.cuda.synchronize()
    return x.cpu(), u8.cpu().numpy()


def _check(frames, rects, s):
    ref = eg.restate_rects(frames, rects, s)
    x, u8 = _run(frames, rects, s)
    print("S=%d %s: %d of %d bytes differ" % (s, frames.shape, int((u8 != ref).sum()), ref.size))
    assert int((u8 != ref).sum()) == 0
    f = torch.from_numpy(ref).permute(0, 3, 1, 2).float()
    assert x.dtype == torch.float32 and torch.equal(x, (f - 127.5) / 128.0)
    return ref, f


# (frame, x1, y1, x2, y2): a 7x9 crop (up-sampling), the whole frame (of the last frame too: the final bytes of the buffer),
# 23x31 at an odd x1, a 16x16 identity, a rectangle on frame 1
def _rects16(h, w):
    return [(0, 5, 3, 12, 12), (0, 0, 0, w, h), (1, 0, 0, w, h), (0, 11, 2, 34, 33), (0, 20, 10, 36, 26), (1, 13, 5, 60, 30)]


@pytest.mark.parametrize("shape", [(2, 37, 83, 3), (2, 40, 80, 3)], ids=["pitch249", "pitch240"])
def test_synthetic_frames_equal_the_restatement_in_every_output_form(shape):
    frames = _frames(shape, 11)
    rects = _rects16(shape[1], shape[2])
    ref, f = _check(frames, rects, 16)
    assert np.array_equal(ref[4], frames[0, 10:26, 20:36])                      # the identity
    std = (f - 127.5) / 128.0
    for dt in (torch.bfloat16, torch.float16):
        x, _ = _run(frames, rects, 16, dtype=dt)
        assert x.dtype == dt and torch.equal(x, std.to(dt))                    # the fp32 value, rounded to nearest-even
        x, _ = _run(frames, rects, 16, dtype=dt, standardize=False)
        assert torch.equal(x, f.to(dt))
    x, _ = _run(frames, rects, 16, standardize=False)
    assert torch.equal(x, f)
    _check(frames, [(1, 31, 4, 61, 34)], 160)                                  # 30x30 -> 160


def test_frames_at_an_odd_address_and_only_one_output():
    from vn_celeb_face_recognition_amd.detector import extract_faces_device
    frames = _frames((2, 37, 83, 3), 12)
    buf = torch.zeros(frames.size + 1, dtype=torch.uint8, device=DEV)
    buf[1:] = torch.from_numpy(frames).to(DEV).reshape(-1)
    fd = buf[1:].view(frames.shape)
    assert fd.data_ptr() % 2 == 1
    rects = _rects16(37, 83)
    ref = eg.restate_rects(frames, rects, 16)
    _, u8 = _run(fd, rects, 16)
    assert int((u8 != ref).sum()) == 0
    x, none = extract_faces_device(fd, np.asarray(rects, np.int32), 16, want_u8=False)
    assert none is None and torch.equal(x.cpu(), (torch.from_numpy(ref).permute(0, 3, 1, 2).float() - 127.5) / 128.0)


@pytest.mark.parametrize("shape,s", [((1, 8, 1500, 3), 16),      # wider than one strip of column sums: x-tiles
                                     ((1, 8, 1500, 3), 2),       # one bin wider than a strip: per-pixel sums
                                     ((1, 600, 8, 3), 2),        # bins deeper than 256 rows: the 16-bit partial sums roll over
                                     ((1, 9, 700, 3), 7)],       # an odd output side, two x-tiles
                         ids=["xtiles", "widebin", "deepbin", "odd-s"])
def test_every_code_path_by_crop_size(shape, s):
    frames = _frames(shape, 13)
    _check(frames, [(0, 0, 0, shape[2], shape[1]), (0, 1, 1, shape[2] - 2, shape[1] - 1)], s)


def test_constant_frames_keep_their_value():
    """The test a reciprocal multiply fails: sum * (1 / (kh kw)) truncates a constant bin to v - 1."""
    vals = [1, 85, 127, 254, 255]
    frames = np.empty((5, 101, 101, 3), np.uint8)
    for k, v in enumerate(vals):
        frames[k] = v
    rects = [(k, x1, y1, x1 + cw, y1 + ch) for k in range(5) for (x1, y1, cw, ch) in ((3, 2, 23, 29), (7, 5, 37, 41), (6, 0, 95, 101))]
    x, u8 = _run(frames, rects, 16, standardize=False)
    for i, r in enumerate(rects):
        assert (u8[i] == vals[r[0]]).all() and (x[i] == float(vals[r[0]])).all(), (r, np.unique(u8[i]))


def _abi(frames, b, h, w, rects, n, s, std, x, dt, u8):
    from vn_celeb_face_recognition_amd import _lib
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None      # noqa: E731
    return _lib.load().vnf_extract_faces(p(frames), b, h, w, p(rects), n, s, std, p(x), dt, p(u8), _lib.current_stream_ptr())


def test_abi_noop_invalid_arguments_and_unseen_rows():
    from vn_celeb_face_recognition_amd import _lib
    frames_h = _frames((2, 20, 30, 3), 14)
    frames = torch.from_numpy(frames_h).to(DEV)
    rects_h = np.array([[0, 2, 2, 18, 18], [2, 2, 2, 18, 18], [-1, 2, 2, 18, 18], [1, 5, 5, 5, 9], [1, 5, 9, 9, 5],
                        [0, -1, 2, 18, 18], [0, 2, 2, 31, 18], [1, 2, 2, 18, 21], [1, 0, 0, 30, 20]], np.int32)
    rects = torch.from_numpy(rects_h).to(DEV)
    n, s = len(rects_h), 8
    x = torch.full((n, 3, s, s), 7.0, device=DEV)
    u8 = torch.full((n, s, s, 3), 7, dtype=torch.uint8, device=DEV)
    assert _abi(None, 0, 0, 0, None, 0, s, 1, None, 0, None) == 0               # n == 0: no-op
    assert _abi(frames, 2, 20, 30, rects, 0, s, 1, x, _lib.VNF_F32, u8) == 0
    torch.cuda.synchronize()
    assert (x == 7.0).all() and (u8 == 7).all()
    for args in ((frames, 2, 20, 30, rects, n, 0, 1, x, _lib.VNF_F32, u8), (frames, 2, 20, 30, rects, n, 1025, 1, x, _lib.VNF_F32, u8),
                 (None, 2, 20, 30, rects, n, s, 1, x, _lib.VNF_F32, u8), (frames, 2, 20, 30, None, n, s, 1, x, _lib.VNF_F32, u8),
                 (frames, 2, 20, 30, rects, n, s, 1, x, _lib.VNF_I64, u8), (frames, 2, 20, 30, rects, n, s, 1, x, 9, None),
                 (frames, 2, 20, 30, rects, n, s, 1, None, _lib.VNF_F32, None)):
        assert _abi(*args) == -1 and b"vnf_extract_faces" in _lib.load().vnf_last_error()
    torch.cuda.synchronize()
    assert (x == 7.0).all() and (u8 == 7).all()
    # rows the call cannot see: a frame index or rectangle out of range (or empty) is written as zeros; good rows are served
    assert _abi(frames, 2, 20, 30, rects, n, s, 1, x, _lib.VNF_F32, u8) == 0
    torch.cuda.synchronize()
    good = [0, n - 1]
    ref = eg.restate_rects(frames_h, rects_h[good], s)
    assert np.array_equal(u8.cpu().numpy()[good], ref)
    assert (u8[1:n - 1] == 0).all() and (x[1:n - 1] == 0).all()
    # the host layer refuses such rows before anything is uploaded
    from vn_celeb_face_recognition_amd.detector import extract_faces_device
    with pytest.raises(ValueError, match="rectangle 1 "):
        extract_faces_device(frames, rects_h, s)
    with pytest.raises(_lib.VnfError, match="VNF_E_INVALID"):
        extract_faces_device(torch.zeros((1, 400, 400, 3), dtype=torch.uint8, device=DEV), [[0, 0, 0, 400, 400]], 2)


@pytest.fixture(scope="module")
def picture_forms():
    img = eg.picture()
    return {"ndarray": img, "tensor": torch.from_numpy(img.copy()), "pil": Image.fromarray(img)}


def _mtcnn(**kw):
    from vn_celeb_face_recognition_amd.models import MTCNN
    h, w = eg.picture().shape[:2]
    return MTCNN(min_face_size=int(eg.golden()["min_face_size"]), device=DEV, max_batch=2, max_height=h, max_width=w, **kw)


def _bytes(face):
    return (face.float().cpu() * 128.0 + 127.5).numpy()


def test_extract_with_the_golden_boxes_equals_the_golden_faces(picture_forms):
    from vn_celeb_face_recognition_amd.detector import extract_face
    for keep_all, margin, size, boxes, _, _, faces in eg.forward_cases():
        det = _mtcnn(image_size=size, margin=margin, keep_all=keep_all)
        for form, img in picture_forms.items():
            got = det.extract(img, boxes, None)
            assert got.is_cuda and got.dtype == torch.float32
            assert tuple(got.shape) == ((len(boxes), 3, size, size) if keep_all else (3, size, size))
            assert np.array_equal(_bytes(got).reshape(faces.shape), faces), (keep_all, margin, size, form)
        raw = _mtcnn(image_size=size, margin=margin, keep_all=keep_all, post_process=False).extract(picture_forms["ndarray"], boxes, None)
        assert np.array_equal(raw.cpu().numpy().reshape(faces.shape), faces)
        half = det.extract(picture_forms["ndarray"], boxes, None, dtype=torch.bfloat16)
        assert half.dtype == torch.bfloat16 and torch.equal(half.cpu(), det.extract(picture_forms["ndarray"], boxes, None).cpu().to(torch.bfloat16))
    for box, margin, size, face in eg.extract_face_cases():
        for form, img in picture_forms.items():
            got = extract_face(img, box, size, margin)
            assert got.is_cuda and np.array_equal(got.cpu().numpy(), face), (box, form)
    # batch form: a list per image, None where an image has no boxes; one buffer behind all of them
    _, _, _, boxes, _, _, faces = eg.forward_cases()[0]
    det = _mtcnn(keep_all=True)
    img = picture_forms["ndarray"]
    out = det.extract([img, img, img], [boxes, None, boxes[[1]]], None)
    assert out[1] is None and np.array_equal(_bytes(out[0]), faces) and np.array_equal(_bytes(out[2]), faces[[1]])
    assert out[2].untyped_storage().data_ptr() == out[0].untyped_storage().data_ptr()
    with pytest.raises(ValueError, match="box 0 "):
        det.extract(img, np.array([[900.0, 10.0, 950.0, 60.0]], np.float32), None)


def test_forward_end_to_end(picture_forms):
    img = picture_forms["ndarray"]
    _, _, _, gboxes, gprobs, _, _ = eg.forward_cases()[0]
    det = _mtcnn(keep_all=True)
    faces, boxes, probs = det(img, return_prob=True)
    boxes = np.asarray(boxes)
    assert np.abs(boxes - gboxes).max() <= 1e-3 and np.abs(np.asarray(probs) - gprobs).max() <= 1e-5   # tests/test_gpu_mtcnn.py's bounds
    assert faces.is_cuda and faces.dtype == torch.float32 and tuple(faces.shape) == (2, 3, 160, 160)
    assert torch.equal(faces, det.extract(img, boxes, None))
    assert np.array_equal(_bytes(faces), eg.restate_boxes(img, boxes, 160, 0))
    two = det.forward(img)
    assert len(two) == 2 and torch.equal(two[0], faces) and np.array_equal(np.asarray(two[1]), boxes)
    none, b2 = det(img, extract_face=False)
    assert none is None and np.array_equal(np.asarray(b2), boxes)
    # without keep_all: the selected box alone, unwrapped; an image without a face gives None / None / [None]
    one = _mtcnn(keep_all=False, margin=14, image_size=64)
    face, box, prob = one(picture_forms["pil"], return_prob=True)
    _, _, _, sboxes, sprobs, _, sfaces = eg.forward_cases()[2]
    assert tuple(face.shape) == (3, 64, 64) and box.shape == (1, 4) and np.ndim(prob) == 0
    assert np.abs(box - sboxes).max() <= 1e-3 and abs(float(prob) - float(sprobs[0])) <= 1e-5
    assert np.array_equal(_bytes(face)[None], eg.restate_boxes(img, box, 64, 14))
    grey = np.full_like(img, 128)
    faces, boxes, probs = one([img, grey], return_prob=True)
    assert isinstance(faces, list) and faces[1] is None and boxes[1] is None and probs[1] == [None]
    assert torch.equal(faces[0], face) and np.array_equal(boxes[0], box)
    faces, boxes = det([grey, img])
    assert faces[0] is None and len(boxes[0]) == 0 and tuple(faces[1].shape) == (2, 3, 160, 160)
    face, box, prob = one(grey, return_prob=True)
    assert face is None and box is None and prob is None


def test_save_path_writes_the_unstandardised_faces(picture_forms, tmp_path):
    _, _, _, boxes, _, _, faces = eg.forward_cases()[0]
    det = _mtcnn(keep_all=True)
    path = str(tmp_path / "out" / "face.png")
    got = det.extract(picture_forms["ndarray"], boxes, path)
    assert np.array_equal(_bytes(got), faces)
    assert sorted(os.listdir(tmp_path / "out")) == ["face.png", "face_2.png"]
    assert np.array_equal(np.asarray(Image.open(path)), faces[0].transpose(1, 2, 0))
    assert np.array_equal(np.asarray(Image.open(str(tmp_path / "out" / "face_2.png"))), faces[1].transpose(1, 2, 0))
    # a list with one entry per image; an image without a path saves nothing
    p2 = str(tmp_path / "b" / "second.png")
    det.extract([picture_forms["ndarray"]] * 2, [boxes, boxes[[1]]], [None, p2])
    assert os.listdir(tmp_path / "b") == ["second.png"]
    assert np.array_equal(np.asarray(Image.open(p2)), faces[1].transpose(1, 2, 0))
    with pytest.raises(ValueError, match="one entry per image"):
        det.extract([picture_forms["ndarray"]] * 2, [boxes, boxes], path)


def test_encoder_takes_the_faces_directly(picture_forms):
    from vn_celeb_face_recognition_amd import models
    enc = models.InceptionResnetV1(pretrained=None, max_batch=8).to(DEV).eval()
    faces = _mtcnn(keep_all=True)(picture_forms["tensor"])[0]
    emb = enc(faces)
    assert tuple(emb.shape) == (2, 512) and bool(torch.isfinite(emb.float()).all())


def test_crop_face_cli(tmp_path):
    name = str(eg.golden()["picture"])
    src = tmp_path / "in"; src.mkdir()
    shutil.copy(os.path.join(GOLDEN, "images", name), src / name)
    Image.fromarray(np.full((120, 160, 3), 128, np.uint8)).save(src / "grey.png")
    cfg = tmp_path / "mtcnn.json"
    cfg.write_text(json.dumps({"image_size": 160, "keep_all": True, "min_face_size": int(eg.golden()["min_face_size"])}))
    args = [sys.executable, os.path.join(REPO, "crop_face.py"), "-id", str(src), "-od", str(tmp_path / "out"),
            "-nf", str(tmp_path / "unknown.txt"), "-mf", str(tmp_path / "many.txt"), "-dargs", str(cfg)]
    env = dict(os.environ, PYTHONPATH=REPO)
    r = subprocess.run(args, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Total images: 2." in r.stdout and "No face images: 1." in r.stdout and "Many face images: 1." in r.stdout
    assert os.listdir(tmp_path / "out") == [name]
    assert (tmp_path / "unknown.txt").read_text() == str(src / "grey.png") + "\n"
    assert (tmp_path / "many.txt").read_text() == str(src / name) + "\n"
    img = eg.picture()
    b = eg.forward_cases()[0][3][0]              # box 0; the device's differs by under 1e-3 px, far from a pixel edge here
    assert min(abs(v - round(v)) for v in b.tolist()) > 2e-3
    want = img[max(int(b[1]), 0):min(int(b[3] + 1), img.shape[0]), max(int(b[0]), 0):min(int(b[2] + 1), img.shape[1])]
    assert np.array_equal(np.asarray(Image.open(tmp_path / "out" / name).convert("RGB")), want)
    # a second run skips what exists: nothing is processed again, the picture is not listed again
    before = os.path.getmtime(tmp_path / "out" / name)
    r = subprocess.run(args, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Processing " + str(src / name) not in r.stdout and os.path.getmtime(tmp_path / "out" / name) == before
    assert (tmp_path / "many.txt").read_text() == ""
