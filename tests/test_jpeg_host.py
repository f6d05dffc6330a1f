"""CPU: the host half of the JPEG frame decoder (csrc/jpeg_entropy.cpp through ctypes) and the compressed-frame access of
the video sources.  The pixel arithmetic behind the entropy decode is tests/jpeg_restatement.py (NumPy); the expected
bytes are Pillow's, recorded in tests/golden/jpeg_cases.npz (tools/make_jpeg_golden.py)."""
import ctypes
import os

import numpy as np
import pytest

import jpeg_restatement as R
from conftest import GOLDEN, load_image

OK_CASES = [c for c in R.load_cases()[0] if c["expect"] == "ok"]
NOT_TAKEN_CASES = [c for c in R.load_cases()[0] if c["expect"] != "ok"]
PICTURES = ["dam_vinh_hung_2_recog.jpg", "mrDam_HaHo_recog.jpg"]
CANARY = 4096   # int16 guard elements on either side of the coefficient buffer


@pytest.fixture(scope="module")
def jpeg():
    import __graft_entry__ as ge
    ge.build()
    from vn_celeb_face_recognition_amd import jpeg as j
    return j


def _decode(jpeg, data):
    rc, info = jpeg.probe(data)
    assert rc == 0, rc
    coefs = np.zeros(info.coef_count, np.int16)
    assert jpeg.entropy_decode(data, info, coefs) == 0
    rgb = R.coefs_to_rgb(coefs, jpeg.quant_table(info), info.width, info.height, info.sampling, list(info.blocks_w),
                         list(info.blocks_h))
    return info, rgb


def test_goldens_record_their_versions():
    _, ver = R.load_cases()
    assert ver["pillow"] and ver["libjpeg_turbo"]
    assert len(OK_CASES) >= 40 and len(NOT_TAKEN_CASES) >= 1


@pytest.mark.parametrize("case", OK_CASES, ids=[c["name"] for c in OK_CASES])
def test_entropy_decode_and_restatement_equal_pillow_bytes(jpeg, case):
    info, rgb = _decode(jpeg, case["jpg"])
    assert rgb.shape == case["rgb"].shape
    assert int((rgb != case["rgb"]).sum()) == 0


@pytest.mark.parametrize("name", PICTURES)
def test_reference_pictures_equal_pillow_bytes(jpeg, name):
    with open(os.path.join(GOLDEN, "images", name), "rb") as f:
        data = f.read()
    info, rgb = _decode(jpeg, data)
    want = load_image(name)
    assert info.sampling == R.S420 and rgb.shape == want.shape
    assert int((rgb != want).sum()) == 0


@pytest.mark.parametrize("case", OK_CASES, ids=[c["name"] for c in OK_CASES])
def test_probe_reports_what_was_written(jpeg, case):
    rc, info = jpeg.probe(case["jpg"])
    assert rc == 0
    hdr = R.read_header(case["jpg"])
    assert hdr["sof"] == 0xC0 and (info.width, info.height) == (case["width"], case["height"]) == (hdr["width"], hdr["height"])
    gray = case["mode"] == "L"
    assert info.components == (1 if gray else 3) == len(hdr["comps"])
    sub = case["params"].get("subsampling")
    assert info.sampling == (R.GRAY if gray else {0: R.S444, 1: R.S422, 2: R.S420}[sub])
    hv = (1, 1) if gray else {0: (1, 1), 1: (2, 1), 2: (2, 2)}[sub]
    assert (info.h[0], info.v[0]) == hv and all((info.h[c], info.v[c]) == (1, 1) for c in range(1, info.components))
    mx, my = -(-case["width"] // (8 * hv[0])), -(-case["height"] // (8 * hv[1]))
    for c in range(info.components):
        assert (info.blocks_w[c], info.blocks_h[c]) == ((mx * hv[0], my * hv[1]) if c == 0 else (mx, my))
        assert np.array_equal(jpeg.quant_table(info)[c], hdr["quant"][hdr["comps"][c][3]])
    assert info.coef_count == 64 * sum(info.blocks_w[c] * info.blocks_h[c] for c in range(info.components))
    want_dri = 0
    if "restart_marker_blocks" in case["params"]:
        want_dri = case["params"]["restart_marker_blocks"]
    elif "restart_marker_rows" in case["params"]:
        want_dri = case["params"]["restart_marker_rows"] * mx
    assert info.restart_interval == want_dri == hdr["dri"]


@pytest.mark.parametrize("case", NOT_TAKEN_CASES, ids=[c["name"] for c in NOT_TAKEN_CASES])
def test_progressive_and_cmyk_are_not_taken(jpeg, case):
    rc, _ = jpeg.probe(case["jpg"])
    assert rc == jpeg.NOT_TAKEN == 1


def test_probe_tells_corrupt_from_not_taken(jpeg):
    data = OK_CASES[0]["jpg"]
    assert jpeg.probe(b"")[0] < 0 and jpeg.probe(b"\x89PNG\r\n\x1a\n" + bytes(64))[0] < 0
    assert jpeg.probe(data[:40])[0] < 0                       # cut inside the header
    hdr = R.read_header(data)
    assert jpeg.probe(data[:hdr["scan"]])[0] == 0             # the header alone probes; the scan is the decode's business


def _guarded_decode(jpeg, data, info):
    """entropy-decode into a buffer of exactly coef_count elements between two canaries -> (status, canaries intact)"""
    from vn_celeb_face_recognition_amd import _lib
    n = int(info.coef_count)
    buf = np.full(n + 2 * CANARY, 0x5A5A, np.int16)
    rc = _lib.load().vnf_jpeg_entropy_decode(data, len(data), ctypes.byref(info), buf.ctypes.data + 2 * CANARY, n)
    return rc, bool((buf[:CANARY] == 0x5A5A).all() and (buf[n + CANARY:] == 0x5A5A).all())


STRESS = ["33x47_420_rstb3", "64x48_420_noise_q95", "33x47_444_opt"]


@pytest.mark.parametrize("name", STRESS)
def test_truncated_streams_are_errors_and_stay_inside_the_buffer(jpeg, name):
    data = next(c["jpg"] for c in OK_CASES if c["name"] == name)
    rc, info = jpeg.probe(data)
    assert rc == 0
    scan = R.read_header(data)["scan"]
    for k in range(1, 17):
        cut = data[:len(data) * k // 17]
        rc_p, info_p = jpeg.probe(cut)
        assert rc_p <= 0 if len(cut) < scan else rc_p == 0
        rc, intact = _guarded_decode(jpeg, cut, info)
        assert intact, (name, k)
        assert rc < 0, (name, k, rc)            # every one of these cuts loses entropy-coded data: never a success
    assert _guarded_decode(jpeg, data, info) == (0, True)
    assert _guarded_decode(jpeg, data[:-2], info) == (0, True)   # only the EOI marker missing: every MCU is there
    from vn_celeb_face_recognition_amd import _lib
    small = np.zeros(64, np.int16)
    assert _lib.load().vnf_jpeg_entropy_decode(data, len(data), ctypes.byref(info), small.ctypes.data, 63) == -4


@pytest.mark.parametrize("name", STRESS)
def test_flipped_bytes_succeed_or_fail_inside_the_buffer(jpeg, name):
    data = next(c["jpg"] for c in OK_CASES if c["name"] == name)
    rc, info = jpeg.probe(data)
    scan = R.read_header(data)["scan"]
    rng = np.random.default_rng(1234)
    seen = set()
    for _ in range(32):
        b = bytearray(data)
        at = int(rng.integers(scan, len(data) - 2))
        b[at] ^= 1 << int(rng.integers(0, 8))
        rc, intact = _guarded_decode(jpeg, bytes(b), info)
        assert intact and rc <= 0, (name, at, rc)
        seen.add(rc)
    assert seen <= {0, -1}


def _jpeg_dir(tmp_path, names):
    from PIL import Image
    a = load_image("mrDam_HaHo_recog.jpg")[:96, :120]
    d = tmp_path / "frames"
    d.mkdir()
    for i, n in enumerate(names):
        img = Image.fromarray(np.ascontiguousarray(np.roll(a, 7 * i, axis=1)))
        img.save(d / n, **({"quality": 90} if not n.endswith(".png") else {}))
    return str(d), a


def test_frame_sources_hand_out_compressed_batches(jpeg, tmp_path):
    from vn_celeb_face_recognition_amd.cli_utils import open_frame_source
    from vn_celeb_face_recognition_amd.mjpeg_avi import read_mjpeg_avi, write_mjpeg_avi
    d, a = _jpeg_dir(tmp_path, ["f0.jpg", "f1.jpeg", "f2.JPG", "f3.jpg", "f4.jpg"])
    avi = str(tmp_path / "clip.avi")
    write_mjpeg_avi(avi, [np.ascontiguousarray(np.roll(a, 5 * i, axis=0)) for i in range(5)], 25.0)
    _, frames, n = read_mjpeg_avi(avi)
    assert n == 5 and np.array_equal(jpeg.decode_host(frames.compressed(3)), frames[3])
    assert frames.compressed(3)[:2] == b"\xff\xd8"
    for path in (d, avi):
        src = open_frame_source(path)
        plain = list(open_frame_source(path).rank_batches(2))
        got = list(src.rank_batches(2, compressed=True))
        assert [g[0] for g in got] == [0, 1, 2] and [g[2] for g in got] == [p[2] for p in plain]
        for (b, q, inf), (_, want, _) in zip(got, plain):
            assert isinstance(q, jpeg.CompressedBatch) and all(isinstance(x, bytes) for x in q)
            for x, w, (_, num) in zip(q, want, inf):
                assert np.array_equal(jpeg.decode_host(x), w) and np.array_equal(w, src._get(num - 1))
                hf = jpeg.HostFrame(x, w.shape)
                assert hf.shape == w.shape and np.array_equal(np.asarray(hf), w)
        # a rank reads only its own batches, compressed or not
        src2 = open_frame_source(path)
        assert [g[0] for g in src2.rank_batches(2, rank=1, world=2, compressed=True)] == [1] and src2.reads == 2


def test_mixed_directory_reports_no_compressed_batch(jpeg, tmp_path):
    from vn_celeb_face_recognition_amd.cli_utils import open_frame_source
    from vn_celeb_face_recognition_amd.video import FrameSource
    d, _ = _jpeg_dir(tmp_path, ["f0.jpg", "f1.png", "f2.jpg", "f3.png"])
    src = open_frame_source(d)
    got = list(src.rank_batches(2, compressed=True))
    assert len(got) == 2 and not any(isinstance(q, jpeg.CompressedBatch) for _, q, _ in got)
    assert all(isinstance(f, np.ndarray) and f.shape == (96, 120, 3) for _, q, _ in got for f in q)
    # a source without compressed access (arrays, decoders) yields what it always did
    arr = FrameSource(np.zeros((3, 4, 4, 3), np.uint8), 30.0)
    assert arr.compressed is None and not isinstance(next(arr.rank_batches(2, compressed=True))[1], jpeg.CompressedBatch)
