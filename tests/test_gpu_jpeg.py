"""GPU: JPEG frames decoded on the device (csrc/jpeg_decode.hip behind csrc/jpeg_entropy.cpp, jpeg.py, the device-decode
path of video.run_stream).  Expected bytes: Pillow's, from tests/golden/jpeg_cases.npz or decoded here; every comparison
is exact."""
import ctypes
import io

import numpy as np
import pytest
import torch

import jpeg_restatement as R
from conftest import load_image

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OK_CASES = [c for c in R.load_cases()[0] if c["expect"] == "ok"]


def _jpeg():
    from vn_celeb_face_recognition_amd import jpeg
    return jpeg


def device_decode(frames):
    """list of JPEG bytes of one geometry -> (B,H,W,3) u8 numpy, through the C ABI on the current stream"""
    jpeg = _jpeg()
    from vn_celeb_face_recognition_amd import _lib
    infos = []
    for d in frames:
        rc, info = jpeg.probe(d)
        assert rc == 0
        infos.append(info)
    i0, B = infos[0], len(frames)
    coefs = np.zeros((B, i0.coef_count), np.int16)
    quant = np.zeros((B, 3, 64), np.uint8)
    for i, d in enumerate(frames):
        assert (infos[i].width, infos[i].height, infos[i].sampling) == (i0.width, i0.height, i0.sampling)
        assert jpeg.entropy_decode(d, infos[i], coefs[i]) == 0
        quant[i] = jpeg.quant_table(infos[i])
    ws = _lib.load().vnf_jpeg_workspace_bytes(B, i0.width, i0.height, i0.sampling)
    assert ws == B * i0.coef_count
    out = torch.full((B, i0.height, i0.width, 3), 0xAB, dtype=torch.uint8, device=DEV)
    jpeg.decode_frames(torch.from_numpy(coefs).to(DEV), torch.from_numpy(quant).to(DEV), B, i0.width, i0.height, i0.sampling,
                       out, torch.empty((ws,), dtype=torch.uint8, device=DEV))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _encode(rgb, **kw):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(rgb).save(buf, format="JPEG", **kw)
    return buf.getvalue()


@pytest.mark.parametrize("case", OK_CASES, ids=[c["name"] for c in OK_CASES])
def test_every_golden_case_equals_pillow_bytes(case):
    got = device_decode([case["jpg"]])[0]
    assert got.shape == case["rgb"].shape
    assert int((got != case["rgb"]).sum()) == 0


def test_batch_with_per_frame_tables_equals_single_decodes():
    pick = ["33x47_420_q75", "33x47_420_q30", "33x47_420_q100"]       # two pictures, three quantisation tables
    cs = [next(c for c in OK_CASES if c["name"] == n) for n in pick]
    tabs = [_jpeg().quant_table(_jpeg().probe(c["jpg"])[1]).tobytes() for c in cs]
    assert len(set(tabs)) == 3
    got = device_decode([c["jpg"] for c in cs])
    for i, c in enumerate(cs):
        assert np.array_equal(got[i], device_decode([c["jpg"]])[0]) and np.array_equal(got[i], c["rgb"])


@pytest.fixture(scope="module")
def frame_1080p():
    from vn_celeb_face_recognition_amd.synth import make_frames
    frames, _ = make_frames(1, 8, seed=5)
    data = _encode(frames[0], quality=92, subsampling=2)
    return data, _jpeg().decode_host(data)


def test_1080p_frame_equals_pillow_and_is_deterministic(frame_1080p):
    data, want = frame_1080p
    rc, info = _jpeg().probe(data)
    assert rc == 0 and (info.width, info.height, info.sampling) == (1920, 1080, R.S420)
    assert info.blocks_h[0] * 8 == 1088                           # the last MCU row is partial
    a = device_decode([data])[0]
    assert int((a != want).sum()) == 0
    assert np.array_equal(a, device_decode([data])[0])


def test_documented_statuses():
    from vn_celeb_face_recognition_amd import _lib
    lib = _lib.load()
    st = _lib.current_stream_ptr()
    assert lib.vnf_jpeg_decode_frames(None, None, 0, 16, 16, R.S420, None, None, 0, st) == 0          # n == 0: no-op
    co = torch.zeros((384,), dtype=torch.int16, device=DEV)
    q = torch.ones((192,), dtype=torch.uint8, device=DEV)
    out = torch.zeros((16, 16, 3), dtype=torch.uint8, device=DEV)
    ws = torch.zeros((384,), dtype=torch.uint8, device=DEV)
    args = lambda samp, nbytes: (co.data_ptr(), q.data_ptr(), 1, 16, 16, samp, out.data_ptr(), ws.data_ptr(), nbytes, st)
    assert lib.vnf_jpeg_workspace_bytes(1, 16, 16, R.S420) == 384
    assert lib.vnf_jpeg_decode_frames(*args(R.S420, 383)) == -4                                       # VNF_E_CAPACITY
    assert lib.vnf_jpeg_decode_frames(*args(7, 384)) == -1 and lib.vnf_jpeg_workspace_bytes(1, 16, 16, 7) == -1
    assert lib.vnf_jpeg_decode_frames(*args(R.S420, 384)) == 0
    torch.cuda.synchronize()
    assert bool((out == 128).all())                               # zero coefficients: mid grey


def test_untaken_batch_falls_back_to_the_host_decoder():
    from vn_celeb_face_recognition_amd.upload import FrameUploader
    jpeg = _jpeg()
    prog = next(c["jpg"] for c in R.load_cases()[0] if c["name"] == "33x47_progressive")
    base = next(c for c in OK_CASES if c["name"] == "33x47_420_q75")
    up = FrameUploader(DEV, depth=3)
    try:
        assert jpeg.decode_batch_device([prog], DEV, up) is None
        assert jpeg.decode_batch_device([base["jpg"], prog], DEV, up) is None                         # one is enough
        other = next(c["jpg"] for c in OK_CASES if c["name"] == "17x13_420_q75")
        assert jpeg.decode_batch_device([base["jpg"], other], DEV, up) is None                        # mixed geometry
        assert jpeg.decode_batch_device([base["jpg"], base["jpg"][:200]], DEV, up) is None            # truncated stream
        dev, ev, slot, host = jpeg.decode_batch([prog], DEV, up)
        ev.synchronize()
        assert np.array_equal(dev.cpu().numpy()[0], jpeg.decode_host(prog)) and np.array_equal(host[0], jpeg.decode_host(prog))
        got = jpeg.decode_batch_device([base["jpg"]] * 2, DEV, up)
        got[1].synchronize()
        assert got[2] >= 0 and np.array_equal(got[0].cpu().numpy()[1], base["rgb"])
        up.release(got[2], None)
    finally:
        up.close()


def test_run_stream_device_decode_equals_host_decode(tmp_path, monkeypatch):
    """A 6-frame Motion-JPEG AVI through video.run_stream: the device-decode path and decode="host" write the same
    tracker rows, and the device batches are the host frames byte for byte."""
    from vn_celeb_face_recognition_amd import jpeg, models
    from vn_celeb_face_recognition_amd.cli_utils import open_frame_source
    from vn_celeb_face_recognition_amd.mjpeg_avi import write_mjpeg_avi
    from vn_celeb_face_recognition_amd.pipeline import FacePipeline
    from vn_celeb_face_recognition_amd.video import run_stream
    a = load_image("mrDam_HaHo_recog.jpg")
    m = np.ascontiguousarray(a[:, ::-1])
    avi = str(tmp_path / "clip.avi")
    assert write_mjpeg_avi(avi, [a, m, a, m, a, m], 25.0) == 6
    det = models.MTCNN(keep_all=True, min_face_size=50, device=DEV, max_batch=2, max_height=a.shape[0], max_width=a.shape[1])
    enc = models.InceptionResnetV1(pretrained=None, compute_dtype="f32", max_batch=16).to(DEV).eval()
    clf = models.MLPModel(512, 1001).to(DEV).eval()
    pipe = FacePipeline(det, enc, clf, {"label": list(range(1001)), "name": ["c%d" % i for i in range(1001)]}, 160, 0.0)
    batches = []
    real = jpeg.decode_batch_device

    def spy(frames, device, uploader, timing=None):
        r = real(frames, device, uploader, timing)
        assert r is not None
        r[1].synchronize()
        batches.append(r[0].cpu().numpy())
        return r

    monkeypatch.setattr(jpeg, "decode_batch_device", spy)
    seen = {}
    rows_dev, n_dev = run_stream(open_frame_source(avi), pipe, 2, device=DEV,
                                 on_frame=lambda f, num, names, boxes: seen.__setitem__(num, np.asarray(f)))
    assert len(batches) == 3 and n_dev == 6
    rows_host, n_host = run_stream(open_frame_source(avi), pipe, 2, device=DEV, decode="host")
    assert len(batches) == 3 and n_host == 6                      # decode="host" never asked the device decoder
    assert rows_dev == rows_host and sorted(rows_dev) == [1, 2, 3, 4, 5, 6]
    assert sum("c" in rows_dev[k].split(",")[1] for k in rows_dev) == 6       # faces were found and named on every frame
    src = open_frame_source(avi)
    for i in range(6):
        want = src._get(i)
        assert np.array_equal(batches[i // 2][i % 2], want) and np.array_equal(seen[i + 1], want)
    torch.cuda.synchronize()
