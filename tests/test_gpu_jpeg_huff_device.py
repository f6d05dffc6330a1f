"""GPU: the Huffman pass of the JPEG frame encoder on the device (csrc/jpeg_huff_device.hip behind csrc/jpeg_encode.hip,
jpeg_encode.py entropy="device", --ov_entropy device).  Expected bytes: the host coder's (jpeg_encode.entropy_encode,
itself pinned to Pillow) at the coefficient level, Pillow's own files at the pixel level.  Every comparison is exact."""
import ast
import csv
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import jpeg_encode_restatement as E
import jpeg_huff_device_restatement as H
from conftest import REPO, load_image

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 4096       # bytes on either side of every buffer the call writes (a multiple of 16: the alignments hold)


def _mods():
    from vn_celeb_face_recognition_amd import _lib, jpeg_encode
    return _lib, jpeg_encode


def _guarded(nbytes):
    """a cuda u8 buffer of nbytes between two guard regions -> (whole, the part between the guards)"""
    whole = torch.full((nbytes + 2 * GUARD,), 0x5A, dtype=torch.uint8, device=DEV)
    return whole, whole[GUARD:GUARD + nbytes]


def _intact(whole, nbytes):
    host = whole.cpu().numpy()
    return bool((host[:GUARD] == 0x5A).all() and (host[GUARD + nbytes:] == 0x5A).all())


def device_huff(coefs, info, capacity, stream=None):
    """(n, coef_count) int16 numpy through vnf_jpeg_huff_encode_frames on `stream` (default: the current one) ->
    (status (n) int32, lengths (n) int64, out (n, capacity) u8), all numpy; out, lengths, status and the workspace sit
    between guard regions that must come back untouched"""
    _lib, jenc = _mods()
    n = coefs.shape[0]
    ws_bytes = jenc.huff_workspace_bytes(n, info, capacity)
    header = torch.from_numpy(jenc.huff_header(info)).to(DEV)
    dev = torch.from_numpy(np.ascontiguousarray(coefs)).to(DEV).reshape(-1)
    bufs = [_guarded(n * capacity), _guarded(8 * n), _guarded(4 * n), _guarded(ws_bytes)]
    (_, out), (_, lengths), (_, status), (_, ws) = bufs
    torch.cuda.synchronize()
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
        jenc.huff_encode_frames(dev, n, info, header, out, capacity, lengths.view(torch.int64), status.view(torch.int32), ws)
    torch.cuda.synchronize()
    for (whole, _), nbytes in zip(bufs, (n * capacity, 8 * n, 4 * n, ws_bytes)):
        assert _intact(whole, nbytes)
    return (status.view(torch.int32).cpu().numpy(), lengths.view(torch.int64).cpu().numpy(),
            out.cpu().numpy().reshape(n, capacity))


def family_batch(info, seed=0):
    return np.stack([H.family(name, info.coef_count, seed) for name in H.FAMILIES])


def check_family_batch(w, h, sampling):
    _, jenc = _mods()
    info = jenc.encode_info(w, h, sampling, 75)
    coefs = family_batch(info, seed=w + h)
    capacity = H.enough_capacity(info.coef_count // 64)
    status, lengths, out = device_huff(coefs, info, capacity)
    assert list(status) == [0] * len(H.FAMILIES)
    for i, name in enumerate(H.FAMILIES):
        want = jenc.entropy_encode(coefs[i], info)
        assert lengths[i] == len(want), (name, lengths[i], len(want))
        assert out[i, :lengths[i]].tobytes() == want, name


@pytest.mark.parametrize("sampling", H.SAMPLINGS, ids=["444", "422", "420"])
@pytest.mark.parametrize("size", H.SIZES, ids=["%dx%d" % s for s in H.SIZES])
def test_files_equal_the_host_coder(size, sampling):
    check_family_batch(size[0], size[1], sampling)


def test_1080p_files_equal_the_host_coder():
    check_family_batch(1920, 1080, E.S420)


@pytest.fixture(scope="module")
def frame_1080p():
    from vn_celeb_face_recognition_amd.synth import make_frames
    frames, _ = make_frames(1, 8, seed=5)
    return np.ascontiguousarray(frames[0])


def test_encode_batch_device_writes_pillows_files(frame_1080p):
    _, jenc = _mods()
    frames = np.stack([E.make_frame(130, 70, "noise", seed=i) for i in range(5)])
    dev = torch.from_numpy(frames).to(DEV)
    for quality, sampling, code in ((92, "4:2:0", E.S420), (75, "4:2:2", E.S422), (100, "4:4:4", E.S444)):
        files = jenc.encode_batch_device(dev, quality, sampling, entropy="device")
        assert files == [E.pillow_jpeg(f, quality, code) for f in frames]
    assert np.array_equal(dev.cpu().numpy(), frames)               # encoding does not touch the frames
    two = np.stack([E.make_frame(130, 70, "ramp", seed=1), np.full((70, 130, 3), 128, np.uint8)])   # mid grey: 6 / 4 bits a unit
    for code, sampling in ((E.S420, "4:2:0"), (E.S444, "4:4:4")):
        assert jenc.encode_batch_device(torch.from_numpy(two).to(DEV), 92, sampling, entropy="device") == \
            [E.pillow_jpeg(f, 92, code) for f in two]
    big = jenc.encode_batch_device(torch.from_numpy(frame_1080p[None]).to(DEV), 92, "4:2:0", entropy="device")
    assert big == [E.pillow_jpeg(frame_1080p, 92, E.S420)]
    assert big == jenc.encode_batch_device(torch.from_numpy(frame_1080p[None]).to(DEV), 92, "4:2:0")      # the host back end


def test_capacity_is_reported_per_frame_and_never_crossed():
    _, jenc = _mods()
    info = jenc.encode_info(130, 70, E.S420, 75)
    capacity = 1024 + int(info.coef_count)
    coefs = family_batch(info, seed=3)
    dense = H.FAMILIES.index("dense")
    for order in (list(range(5)), [0, 2, 3, 4, dense]):            # the frame that overflows inside the batch, and last:
        status, lengths, out = device_huff(coefs[order], info, capacity)     # its capacity ends at the guard
        for k, i in enumerate(order):
            want = jenc.entropy_encode(coefs[i], info)
            assert lengths[k] == len(want), (H.FAMILIES[i], lengths[k], len(want))
            if i == dense:
                assert len(want) > capacity and status[k] == H.CAPACITY
            else:
                assert status[k] == 0 and out[k, :lengths[k]].tobytes() == want, H.FAMILIES[i]


def test_batch_encoder_retries_at_the_reported_size():
    _, jenc = _mods()
    frames = np.stack([E.make_frame(130, 70, "noise", seed=i) for i in range(3)] + [E.make_frame(130, 70, "ramp")])
    want = [E.pillow_jpeg(f, 100, E.S444) for f in frames]
    info = jenc.encode_info(130, 70, E.S444, 100)
    assert max(len(f) for f in want) > 1024 + info.coef_count > len(want[3])       # three overflow the first guess, one fits
    enc = jenc.BatchEncoder(DEV, 100, "4:4:4", entropy="device")
    assert enc.encode(torch.from_numpy(frames).to(DEV)) == want
    assert enc._host is None and enc.d2h_bytes == sum(len(f) for f in want) + 2 * 16 * 4      # files and two tables cross
    assert enc.encode(torch.from_numpy(frames[3:]).to(DEV)) == want[3:]


def test_invalid_coefficients_mark_their_frame_only():
    _lib, jenc = _mods()
    info = jenc.encode_info(33, 47, E.S420, 75)
    coefs = np.stack([H.family("sparse_big", info.coef_count, seed=i) for i in range(5)])
    coefs[1, 64 * 7 + 5] = 1024                                   # an AC of category 11
    coefs[3, 64 * 4], coefs[3, 64 * 5] = 1500, -1500              # luma plane, neighbours in the scan: a DC step of 3000
    status, lengths, out = device_huff(coefs, info, H.enough_capacity(info.coef_count // 64))
    assert list(status) == [0, H.INVALID, 0, H.INVALID, 0]
    for i in (0, 2, 4):
        want = jenc.entropy_encode(coefs[i], info)
        assert lengths[i] == len(want) and out[i, :lengths[i]].tobytes() == want
    for i in (1, 3):
        with pytest.raises(_lib.VnfError):
            jenc.entropy_encode(coefs[i], info)
    # through BatchEncoder: the coefficients of a batch replaced behind the encode kernels
    enc = jenc.BatchEncoder(DEV, 75, "4:2:0", entropy="device")
    frames = torch.from_numpy(np.stack([E.make_frame(33, 47, "noise", seed=i) for i in range(5)])).to(DEV)
    job = enc.enqueue(frames)
    torch.cuda.synchronize()
    enc._coefs[:coefs.size].copy_(torch.from_numpy(coefs.reshape(-1)))
    with torch.cuda.stream(job["stream"]):
        enc._huff_enqueue(job, job["capacity"], job["stream"])
    with pytest.raises(_lib.VnfError):
        enc.finish(job)


def test_same_bytes_twice_and_on_a_side_stream():
    _, jenc = _mods()
    info = jenc.encode_info(264, 136, E.S422, 75)
    coefs = family_batch(info, seed=9)
    capacity = H.enough_capacity(info.coef_count // 64)
    s1, l1, o1 = device_huff(coefs, info, capacity)
    s2, l2, o2 = device_huff(coefs, info, capacity, stream=torch.cuda.Stream(DEV))
    assert list(s1) == list(s2) == [0] * 5 and list(l1) == list(l2)
    for i in range(5):
        assert np.array_equal(o1[i, :l1[i]], o2[i, :l2[i]])


def test_documented_statuses():
    _lib, jenc = _mods()
    lib = _lib.load()
    st = _lib.current_stream_ptr()
    info = jenc.encode_info(16, 16, E.S420, 75)
    assert lib.vnf_jpeg_huff_encode_frames(None, 0, ctypes.byref(info), None, 623, None, 0, None, None, None, 0, st) == 0   # n == 0
    cc, cap = int(info.coef_count), 2048
    ws_bytes = jenc.huff_workspace_bytes(1, info, cap)
    coefs = torch.zeros((cc + 8,), dtype=torch.int16, device=DEV)
    header = torch.from_numpy(jenc.huff_header(info)).to(DEV)
    out = torch.full((cap + 64,), 77, dtype=torch.uint8, device=DEV)
    lengths = torch.zeros((1,), dtype=torch.int64, device=DEV)
    status = torch.full((1,), 9, dtype=torch.int32, device=DEV)
    ws = torch.zeros((ws_bytes,), dtype=torch.uint8, device=DEV)

    def call(inf=info, header_len=623, cp=None, nbytes=ws_bytes):
        return lib.vnf_jpeg_huff_encode_frames(cp if cp is not None else coefs.data_ptr(), 1, ctypes.byref(inf), header.data_ptr(),
                                               header_len, out.data_ptr(), cap, lengths.data_ptr(), status.data_ptr(),
                                               ws.data_ptr(), nbytes, st)

    def changed(**fields):
        bad = _lib.JpegInfo.from_buffer_copy(bytes(info))
        for k, v in fields.items():
            setattr(bad, k, v)
        return bad

    assert call(changed(sampling=E.S444)) == -1 and call(changed(sampling=E.GRAY)) == -1 and call(changed(sampling=7)) == -1
    assert call(changed(restart_interval=1)) == -1
    assert call(header_len=622) == -1
    assert call(cp=coefs.data_ptr() + 2) == -1                    # misaligned coefs_dev
    assert call(nbytes=ws_bytes - 1) == -4                        # VNF_E_CAPACITY
    assert lib.vnf_jpeg_huff_workspace_bytes(1, ctypes.byref(changed(restart_interval=1)), cap) == -1
    torch.cuda.synchronize()
    assert int(status.item()) == 9 and (out.cpu().numpy() == 77).all()        # a refused call enqueues nothing
    assert call() == 0
    torch.cuda.synchronize()
    want = jenc.entropy_encode(np.zeros(cc, np.int16), info)
    got = out.cpu().numpy()
    assert int(status.item()) == 0 and int(lengths.item()) == len(want)
    assert got[:len(want)].tobytes() == want and (got[cap:] == 77).all()


def test_video_encoder_writes_the_same_avi_with_either_back_end(tmp_path):
    from vn_celeb_face_recognition_amd.jpeg_encode import VideoEncoder
    frames = np.stack([E.make_frame(130, 70, "noise", seed=i) for i in range(6)])
    boxes = [[(20.3, 15.7, 50.9, 45.2)], [], [(10.0, 10.0, 50.0, 50.0), (60.5, 5.5, 120.5, 45.5)]]
    names = [["celeb_12"], [], ["celeb_1", "Unknown"]]
    paths = {}
    for entropy in ("host", "device"):
        paths[entropy] = str(tmp_path / (entropy + ".avi"))
        enc = VideoEncoder(paths[entropy], 25.0, DEV, 92, "4:2:0", entropy=entropy)
        for b in range(2):
            enc.write_batch(torch.from_numpy(frames[3 * b:3 * b + 3]).to(DEV), [3 * b + 1, 3 * b + 2, 3 * b + 3], boxes, names)
        enc.close()
        assert enc.frames == 6
    assert open(paths["host"], "rb").read() == open(paths["device"], "rb").read()


def test_demo_video_ov_entropy_device(tmp_path):
    """demo_video.py -ov out.avi --ov_entropy device: every compressed frame is Pillow's encode (q92, 4:2:0) of
    draw_boxes_on_image(frame, boxes, names) with the tracker's boxes and names; the tracker file is the one of a run
    without -ov."""
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
    env = dict(os.environ, PYTHONPATH=REPO)

    def run(args):
        r = subprocess.run([sys.executable, os.path.join(REPO, "demo_video.py")] + args + common, cwd=str(tmp_path), env=env,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        return r.stdout

    so = run(["-i", vin, "-o", str(tmp_path / "of"), "-ot", trk, "--n_frames", "2", "-ov", vout, "-fps", "25", "--ov_entropy", "device"])
    assert "Save exported video in" in so and "Saved tracker file in" in so
    run(["-i", vin, "-o", str(tmp_path / "of0"), "-ot", trk0, "--n_frames", "2"])
    assert open(trk).read() == open(trk0).read()
    fps, got, n = read_mjpeg_avi(vout)
    _, src, n_in = read_mjpeg_avi(vin)
    assert n == n_in == 5 and fps == 25.0
    rows = list(csv.reader(open(trk)))[1:]
    assert [int(r[2]) for r in rows] == [1, 2, 3, 4, 5]
    drawn = 0
    for i, r in enumerate(rows):
        names = ast.literal_eval(r[1])
        boxes = [np.float32(np.array(b) * np.array([w, h, w, h])) for b in ast.literal_eval(r[3])]
        frame = src[i]
        want = draw_boxes_on_image(frame, boxes, names) if names else frame
        drawn += int((want != frame).any())
        assert got.compressed(i) == E.pillow_jpeg(want, 92, E.S420), i
    assert drawn == 4
