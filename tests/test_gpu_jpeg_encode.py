"""GPU: frames JPEG-encoded on the device (csrc/jpeg_encode.hip in front of csrc/jpeg_huff_encode.cpp, jpeg_encode.py, the
encoder path of video.run_stream behind demo_video.py -ov).  Expected numbers: Pillow's -- the quantised coefficients
and the bytes of the files it writes for the same pixels; every comparison is exact."""
import ast
import csv
import io
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import jpeg_encode_restatement as E
from conftest import REPO, load_image

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = [(1, 1), (8, 8), (17, 9), (8, 24), (33, 47), (64, 48), (130, 70)]          # (W, H)
GUARD = 4096       # int16 elements on either side of the coefficient buffer


def _mods():
    from vn_celeb_face_recognition_amd import _lib, jpeg, jpeg_encode
    return _lib, jpeg, jpeg_encode


def device_encode(frames, sampling, quality):
    """(B,H,W,3) u8 numpy -> (B, coef_count) int16 numpy through the C ABI on the current stream; the words around the
    coefficient buffer must come back untouched"""
    _lib, jpeg, jenc = _mods()
    b, h, w = frames.shape[:3]
    info = jenc.encode_info(w, h, sampling, quality)
    cc = int(info.coef_count)
    ws = _lib.load().vnf_jpeg_encode_workspace_bytes(b, w, h, sampling)
    assert ws == b * cc
    buf = torch.full((b * cc + 2 * GUARD,), 0x5A5A, dtype=torch.int16, device=DEV)
    coefs = buf[GUARD:GUARD + b * cc]
    quant = torch.from_numpy(jenc.quant_tables(quality)).to(DEV)
    jenc.encode_frames(torch.from_numpy(np.ascontiguousarray(frames)).to(DEV), quant, coefs,
                       torch.empty((ws,), dtype=torch.uint8, device=DEV), sampling)
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert (host[:GUARD] == 0x5A5A).all() and (host[GUARD + b * cc:] == 0x5A5A).all()
    return host[GUARD:GUARD + b * cc].reshape(b, cc), info


def pillow_coefs(rgb, sampling, quality):
    _, jpeg, _ = _mods()
    data = E.pillow_jpeg(rgb, quality, sampling)
    rc, info = jpeg.probe(data)
    assert rc == 0
    coefs = np.zeros(info.coef_count, np.int16)
    assert jpeg.entropy_decode(data, info, coefs) == 0
    return coefs, data


@pytest.mark.parametrize("sampling", [E.S444, E.S422, E.S420], ids=["444", "422", "420"])
@pytest.mark.parametrize("size", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_coefficients_equal_pillow(size, sampling):
    w, h = size
    for quality in (30, 92):
        for content in ("noise", "ramp"):
            frames = np.stack([E.make_frame(w, h, content, seed=i) for i in range(3)])   # 3 different frames, one geometry
            got, _ = device_encode(frames, sampling, quality)
            for i in range(3):
                want, _ = pillow_coefs(frames[i], sampling, quality)
                diff = int((got[i] != want).sum())
                print(size, sampling, quality, content, i, "differing coefficients:", diff)
                assert diff == 0


@pytest.fixture(scope="module")
def frame_1080p():
    from vn_celeb_face_recognition_amd.synth import make_frames
    frames, _ = make_frames(1, 8, seed=5)
    return np.ascontiguousarray(frames[0])


def test_1080p_frame_equals_pillow_and_is_deterministic(frame_1080p):
    assert frame_1080p.shape == (1080, 1920, 3)
    got, info = device_encode(frame_1080p[None], E.S420, 92)
    assert info.blocks_h[0] * 8 == 1088                           # the last MCU row is partial: a row of dummy blocks
    want, _ = pillow_coefs(frame_1080p, E.S420, 92)
    diff = int((got[0] != want).sum())
    print("1080p differing coefficients:", diff)
    assert diff == 0
    assert np.array_equal(got, device_encode(frame_1080p[None], E.S420, 92)[0])


@pytest.mark.parametrize("sampling", [E.S444, E.S422, E.S420], ids=["444", "422", "420"])
def test_round_trip_on_the_device_equals_pillow_decode_of_pillow_file(sampling):
    _lib, jpeg, jenc = _mods()
    for (w, h) in ((33, 47), (8, 24), (130, 70)):
        frames = np.stack([E.make_frame(w, h, c, seed=4) for c in ("noise", "ramp")])
        info = jenc.encode_info(w, h, sampling, 92)
        cc = int(info.coef_count)
        ws = torch.empty((2 * cc,), dtype=torch.uint8, device=DEV)
        coefs = torch.empty((2 * cc,), dtype=torch.int16, device=DEV)
        q2 = jenc.quant_tables(92)
        jenc.encode_frames(torch.from_numpy(frames).to(DEV), torch.from_numpy(q2).to(DEV), coefs, ws, sampling)
        q3 = torch.from_numpy(np.stack([q2[0], q2[1], q2[1]])[None].repeat(2, axis=0).copy()).to(DEV)
        out = torch.zeros((2, h, w, 3), dtype=torch.uint8, device=DEV)
        jpeg.decode_frames(coefs, q3, 2, w, h, sampling, out, ws)      # the same coefficient format, both ways
        torch.cuda.synchronize()
        for i in range(2):
            want = jpeg.decode_host(E.pillow_jpeg(frames[i], 92, sampling))
            assert int((out[i].cpu().numpy() != want).sum()) == 0


def test_encode_batch_device_writes_pillows_files(frame_1080p):
    _, jpeg, jenc = _mods()
    from vn_celeb_face_recognition_amd.upload import FrameUploader
    frames = np.stack([E.make_frame(130, 70, "noise", seed=i) for i in range(5)])
    dev = torch.from_numpy(frames).to(DEV)
    for quality, sampling, code in ((92, "4:2:0", E.S420), (75, "4:2:2", E.S422), (100, "4:4:4", E.S444)):
        files = jenc.encode_batch_device(dev, quality, sampling)
        assert files == [E.pillow_jpeg(f, quality, code) for f in frames]
    up = FrameUploader(DEV, depth=2)
    try:
        assert jenc.encode_batch_device(dev[:1], 92, "4:2:0", up) == [E.pillow_jpeg(frames[0], 92, E.S420)]
    finally:
        up.close()
    big = jenc.encode_batch_device(torch.from_numpy(frame_1080p[None]).to(DEV), 92, "4:2:0")
    assert big == [E.pillow_jpeg(frame_1080p, 92, E.S420)]
    assert np.array_equal(dev.cpu().numpy(), frames)               # encoding does not touch the frames


def test_documented_statuses():
    _lib, jpeg, jenc = _mods()
    lib = _lib.load()
    st = _lib.current_stream_ptr()
    assert lib.vnf_jpeg_encode_frames(None, 0, 16, 16, E.S420, None, None, None, 0, st) == 0          # n == 0: no-op
    fr = torch.full((16, 16, 3), 128, dtype=torch.uint8, device=DEV)
    q = torch.ones((128,), dtype=torch.uint8, device=DEV)
    co = torch.full((384 + 8,), 77, dtype=torch.int16, device=DEV)
    ws = torch.zeros((384,), dtype=torch.uint8, device=DEV)
    args = lambda samp, nbytes, cp=co.data_ptr(): (fr.data_ptr(), 1, 16, 16, samp, q.data_ptr(), cp, ws.data_ptr(), nbytes, st)
    assert lib.vnf_jpeg_encode_workspace_bytes(1, 16, 16, E.S420) == 384
    assert lib.vnf_jpeg_encode_workspace_bytes(1, 16, 16, E.GRAY) == -1 and lib.vnf_jpeg_encode_workspace_bytes(1, 0, 16, E.S420) == -1
    assert lib.vnf_jpeg_encode_frames(*args(E.S420, 383)) == -4                                       # VNF_E_CAPACITY
    assert lib.vnf_jpeg_encode_frames(*args(E.GRAY, 384)) == -1 and lib.vnf_jpeg_encode_frames(*args(7, 384)) == -1
    assert lib.vnf_jpeg_encode_frames(*args(E.S420, 384, co.data_ptr() + 2)) == -1                    # misaligned coefs_out
    assert lib.vnf_jpeg_encode_frames(*args(E.S420, 384)) == 0
    torch.cuda.synchronize()
    got = co.cpu().numpy()
    assert (got[:384] == 0).all() and (got[384:] == 77).all()      # mid grey: every coefficient zero


def _run(args, cwd):
    env = dict(os.environ, PYTHONPATH=REPO)
    r = subprocess.run([sys.executable] + args, cwd=cwd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def test_demo_video_writes_the_annotated_video_without_pngs(tmp_path):
    """demo_video.py -ov out.avi without -sfr: every frame of the output is Pillow's decode of Pillow's encode (q92,
    4:2:0) of draw_boxes_on_image(frame, boxes, names) with the tracker's boxes and names; no PNG is written; the
    tracker file is the one of a run without -ov."""
    from test_gpu_cli import _classifier_files
    from vn_celeb_face_recognition_amd.cli_utils import draw_boxes_on_image
    from vn_celeb_face_recognition_amd.mjpeg_avi import read_mjpeg_avi, write_mjpeg_avi
    ck, l2n = _classifier_files(tmp_path)
    a = load_image("mrDam_HaHo_recog.jpg")
    h, w = a.shape[:2]
    vin = str(tmp_path / "in.avi")
    write_mjpeg_avi(vin, [a if i != 3 else np.zeros_like(a) for i in range(5)], 25.0, quality=97)
    common = ["-m", ck, "-l2n", l2n, "-enc", "InceptionResnetV1", "-eargs", os.path.join(REPO, "cfg/embedding/inception_resnet_v1.json"),
              "-dargs", os.path.join(REPO, "cfg/detection/mtcnn.json"), "-tg_fs", "160", "--inference_method", "par_fd_vs_aln"]
    trk, trk0, vout = str(tmp_path / "tracker.csv"), str(tmp_path / "tracker0.csv"), str(tmp_path / "out.avi")
    so = _run([os.path.join(REPO, "demo_video.py"), "-i", vin, "-o", str(tmp_path / "of"), "-ot", trk, "--n_frames", "2",
               "-ov", vout, "-fps", "25"] + common, str(tmp_path))
    assert "Save exported video in" in so and "Saved tracker file in" in so
    _run([os.path.join(REPO, "demo_video.py"), "-i", vin, "-o", str(tmp_path / "of0"), "-ot", trk0, "--n_frames", "2"] + common,
         str(tmp_path))
    assert open(trk).read() == open(trk0).read()
    assert os.listdir(tmp_path / "of") == []                       # no PNG, no spool file left
    assert sorted(os.listdir(tmp_path)).count("out.avi") == 1 and not [n for n in os.listdir(tmp_path) if n.endswith(".part")]
    fps, got, n = read_mjpeg_avi(vout)
    _, src, n_in = read_mjpeg_avi(vin)
    assert n == n_in == 5 and fps == 25.0
    rows = list(csv.reader(open(trk)))[1:]
    assert [int(r[2]) for r in rows] == [1, 2, 3, 4, 5]
    drawn = 0
    for i, r in enumerate(rows):
        names = ast.literal_eval(r[1])
        boxes = [np.float32(np.array(b) * np.array([w, h, w, h])) for b in ast.literal_eval(r[3])]    # demo_video.py:160-166 undone
        assert len(names) == len(boxes)
        frame = src[i]
        want = draw_boxes_on_image(frame, boxes, names) if names else frame
        drawn += int((want != frame).any())
        want_file = E.pillow_jpeg(want, 92, E.S420)
        assert got.compressed(i) == want_file, i
        assert np.array_equal(got[i], np.asarray(__import__("PIL.Image").Image.open(io.BytesIO(want_file)).convert("RGB")))
    assert drawn == 4 and not ast.literal_eval(rows[3][1])        # faces on every frame but the blank one
    # a name the container cannot carry is refused before any model is loaded
    r = subprocess.run([sys.executable, os.path.join(REPO, "demo_video.py"), "-i", vin, "-ov", str(tmp_path / "out.mp4")] + common,
                       cwd=str(tmp_path), env=dict(os.environ, PYTHONPATH=REPO), capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and ".avi" in r.stderr and not os.path.exists(tmp_path / "out.mp4")
