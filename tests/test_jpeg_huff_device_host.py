"""CPU: the host side of the device Huffman coder (csrc/jpeg_huff_device.hip): its three entry points are declared and
exported, vnf_jpeg_huff_header is the header vnf_jpeg_entropy_encode writes, the decomposition into per-unit passes
(tests/jpeg_huff_device_restatement.py, the OR-pack in a shuffled order) gives the host coder's bytes, the stand-alone
checker of the per-lane bodies passes, and the Python layer and the command lines take `entropy` / --ov_entropy.  Every
comparison is exact."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import jpeg_encode_restatement as E
import jpeg_huff_device_restatement as H
from conftest import REPO

NEW = ("vnf_jpeg_huff_header", "vnf_jpeg_huff_workspace_bytes", "vnf_jpeg_huff_encode_frames")
CANARY = 64


@pytest.fixture(scope="module")
def jenc():
    import __graft_entry__ as ge
    ge.build()
    from vn_celeb_face_recognition_amd import jpeg_encode
    return jpeg_encode


def test_the_three_entry_points_are_declared_exported_and_bound(jenc):
    from vn_celeb_face_recognition_amd import _lib
    lib = _lib.load()
    hdr = open(os.path.join(REPO, "include", "vnface.h")).read()
    declared = set(re.findall(r"\b(vnf_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared and hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert _lib.SIGNATURES["vnf_jpeg_huff_workspace_bytes"][0] is ctypes.c_int64
    assert len(_lib.SIGNATURES["vnf_jpeg_huff_encode_frames"][1]) == 12


@pytest.mark.parametrize("sampling", H.SAMPLINGS, ids=["444", "422", "420"])
def test_header_is_the_host_coders(jenc, sampling):
    from vn_celeb_face_recognition_amd import _lib
    lib = _lib.load()
    for quality in (30, 92, 100):
        for (w, h) in ((1, 1), (17, 9), (130, 70)):
            info = jenc.encode_info(w, h, sampling, quality)
            want = jenc.entropy_encode(H.family("sparse_big", info.coef_count), info)[:H.HEADER_LEN]
            got = jenc.huff_header(info)
            assert got.size == H.HEADER_LEN and got.tobytes() == want
            assert want[-14:-12] == b"\xff\xda"                                  # ends with the SOS segment
            buf = np.full(H.HEADER_LEN - 1 + CANARY, 0x5A, np.uint8)
            n = ctypes.c_int64(-1)
            rc = lib.vnf_jpeg_huff_header(ctypes.byref(info), buf.ctypes.data, H.HEADER_LEN - 1, ctypes.byref(n))
            assert (rc, n.value) == (H.CAPACITY, H.HEADER_LEN)
            assert buf[:H.HEADER_LEN - 1].tobytes() == want[:-1] and (buf[H.HEADER_LEN - 1:] == 0x5A).all()
    bad = _lib.JpegInfo.from_buffer_copy(bytes(jenc.encode_info(16, 16, sampling, 75)))
    bad.restart_interval = 1
    assert lib.vnf_jpeg_huff_header(ctypes.byref(bad), buf.ctypes.data, 1024, ctypes.byref(n)) == H.INVALID


@pytest.mark.parametrize("sampling", H.SAMPLINGS, ids=["444", "422", "420"])
@pytest.mark.parametrize("size", H.SIZES, ids=["%dx%d" % s for s in H.SIZES])
def test_restated_passes_equal_the_host_coder(jenc, size, sampling):
    w, h = size
    info = jenc.encode_info(w, h, sampling, 75)
    header = jenc.huff_header(info).tobytes()
    for i, name in enumerate(H.FAMILIES):
        coefs = H.family(name, info.coef_count, seed=w + h)
        want = jenc.entropy_encode(coefs, info)
        status, length, got = H.encode(coefs, w, h, sampling, header, seed=i)
        assert (status, length) == (H.OK, len(want)) and got == want, name
        assert len(want) <= H.enough_capacity(info.coef_count // 64)
    # cut short: the length is still the one that fits
    coefs = H.family("dense", info.coef_count, seed=w + h)
    want = jenc.entropy_encode(coefs, info)
    assert H.encode(coefs, w, h, sampling, header, capacity=len(want) - 1) == (H.CAPACITY, len(want), want[:-1])


def test_restated_passes_equal_pillow_on_pillows_coefficients(jenc):
    from vn_celeb_face_recognition_amd import jpeg
    for (w, h, sampling, quality) in ((33, 47, E.S420, 92), (17, 9, E.S422, 30), (64, 48, E.S444, 100), (130, 70, E.S420, 75)):
        for content in ("noise", "ramp"):
            data = E.pillow_jpeg(E.make_frame(w, h, content, seed=2), quality, sampling)
            rc, info = jpeg.probe(data)
            coefs = np.zeros(info.coef_count, np.int16)
            assert rc == 0 and jpeg.entropy_decode(data, info, coefs) == 0
            mine = jenc.encode_info(w, h, sampling, quality)
            status, length, got = H.encode(coefs, w, h, sampling, jenc.huff_header(mine).tobytes(), seed=5)
            assert status == H.OK and got == jenc.entropy_encode(coefs, mine)
            a, b = data.index(b"\xff\xda"), got.index(b"\xff\xda")
            assert got[b:] == data[a:]                                           # Pillow's scan, byte for byte


def test_restatement_refuses_what_the_host_coder_refuses(jenc):
    info = jenc.encode_info(33, 47, E.S420, 75)
    header = jenc.huff_header(info).tobytes()
    from vn_celeb_face_recognition_amd import _lib
    for at, v in ((5, 1024), (64 * 9, 2048)):
        coefs = np.zeros(info.coef_count, np.int16)
        coefs[at] = v
        assert H.encode(coefs, 33, 47, E.S420, header)[0] == H.INVALID
        with pytest.raises(_lib.VnfError):
            jenc.entropy_encode(coefs, info)


def test_standalone_checker_of_the_per_lane_bodies_passes(tmp_path):
    exe = str(tmp_path / "jpeg_huff_device_check")
    r = subprocess.run(["c++", "-std=c++17", "-O1", os.path.join(REPO, "tools", "jpeg_huff_device_check.cpp"),
                        os.path.join(REPO, "vn_celeb_face_recognition_amd", "csrc", "jpeg_huff_encode.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "every file equal" in r.stdout, r.stdout + r.stderr


def test_unknown_entropy_is_refused_and_device_entropy_has_no_cpu_path(jenc, tmp_path):
    import torch
    frames = torch.zeros((1, 8, 8, 3), dtype=torch.uint8)
    with pytest.raises(ValueError, match="entropy"):
        jenc.BatchEncoder("cpu", 92, "4:2:0", entropy="gpu")
    with pytest.raises(ValueError, match="entropy"):
        jenc.encode_batch_device(frames, 92, "4:2:0", entropy="Device")
    with pytest.raises(ValueError, match="entropy"):
        jenc.VideoEncoder(str(tmp_path / "v.avi"), 25.0, "cpu", entropy="")
    assert not os.path.exists(tmp_path / "v.avi")
    for entropy in jenc.ENTROPY:
        with pytest.raises(RuntimeError, match="no CPU path"):
            jenc.BatchEncoder("cpu", 92, "4:2:0", entropy=entropy)
    with pytest.raises(RuntimeError, match="no CPU path"):
        jenc.encode_batch_device(frames, 92, "4:2:0", entropy="device")
    with pytest.raises(RuntimeError, match="no CPU path"):
        jenc.VideoEncoder(str(tmp_path / "w.avi"), 25.0, "cpu", entropy="device")
    assert not os.path.exists(tmp_path / "w.avi")


def test_both_command_lines_take_ov_entropy(capsys):
    import celeb_statistic
    import demo_video
    for mod, extra in ((demo_video, []), (celeb_statistic, ["-fidx", "0"])):
        p = mod.make_parser()
        assert p.parse_args(extra).ov_entropy == "host"
        assert p.parse_args(extra + ["--ov_entropy", "device"]).ov_entropy == "device"
        assert p.parse_args(extra + ["--ov_entropy", "host"]).ov_entropy == "host"
        with pytest.raises(SystemExit):
            p.parse_args(extra + ["--ov_entropy", "gpu"])
        assert "--ov_entropy" in capsys.readouterr().err
