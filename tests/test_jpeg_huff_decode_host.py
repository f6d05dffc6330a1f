"""CPU: the host side of the device Huffman decoder (csrc/jpeg_huff_decode.hip): its entry points are declared, exported
and bound; vnf_jpeg_huff_prepare splits the scan of every golden frame into the segments the file has, byte for byte;
the stand-alone checker of the per-lane bodies (tools/jpeg_huff_decode_check.cpp: the very functions the kernels call,
run serially under a sanitizer) passes; the Python layer and the command lines take `entropy` / --decode_entropy."""
import ctypes
import glob
import io
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import jpeg_restatement as R
from conftest import REPO

NEW = ("vnf_jpeg_huff_prepared_bound", "vnf_jpeg_huff_prepare", "vnf_jpeg_huff_decode_workspace_bytes",
       "vnf_jpeg_huff_decode_frames")
OK_CASES = [c for c in R.load_cases()[0] if c["expect"] == "ok"]
NOT_TAKEN_CASES = [c for c in R.load_cases()[0] if c["expect"] != "ok"]
INVALID, CAPACITY = -1, -4
CANARY = 64
TABLE_BYTES = 2448            # a decode table of the blob


@pytest.fixture(scope="module")
def jpeg():
    import __graft_entry__ as ge
    ge.build()
    from vn_celeb_face_recognition_amd import jpeg
    return jpeg


def test_the_entry_points_are_declared_exported_and_bound(jpeg):
    from vn_celeb_face_recognition_amd import _lib
    lib = _lib.load()
    hdr = open(os.path.join(REPO, "include", "vnface.h")).read()
    declared = set(re.findall(r"\b(vnf_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared and hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert _lib.SIGNATURES["vnf_jpeg_huff_prepared_bound"][0] is ctypes.c_int64
    assert _lib.SIGNATURES["vnf_jpeg_huff_decode_workspace_bytes"][0] is ctypes.c_int64
    assert len(_lib.SIGNATURES["vnf_jpeg_huff_decode_frames"][1]) == 11
    assert jpeg.ENTROPY == ("host", "device")


def parse_blob(blob):
    """-> (header dict, [segment bytes])"""
    magic, total, nseg, ri, tables_at, ntables, seg_at, data_at, ncomp = struct.unpack_from("<9I", blob, 0)
    sel = struct.unpack_from("<8B", blob, 36)
    assert magic == 0x31444856 and total == len(blob) and total % 16 == 0
    assert tables_at == 64 and seg_at == tables_at + ntables * TABLE_BYTES and data_at % 16 == 0 and data_at >= seg_at + 8 * nseg
    segs, end = [], data_at
    for s in range(nseg):
        at, n = struct.unpack_from("<2I", blob, seg_at + 8 * s)
        assert at % 16 == 0 and at >= end and at + n <= total
        assert not any(blob[end:at])                                # the padding between segments is zero
        segs.append(bytes(blob[at:at + n]))
        end = at + n
    assert not any(blob[end:]) and total - end < 16
    return dict(nseg=nseg, ri=ri, ntables=ntables, ncomp=ncomp, dc_sel=sel[:4], ac_sel=sel[4:]), segs


def scan_of(data):
    """the entropy-coded bytes of a one-scan file: behind the SOS header, up to EOI"""
    at = data.index(b"\xff\xda")
    at += 2 + struct.unpack_from(">H", data, at + 2)[0]
    assert data[-2:] == b"\xff\xd9"
    return data[at:-2]


@pytest.mark.parametrize("case", OK_CASES, ids=[c["name"] for c in OK_CASES])
def test_prepare_splits_the_scan_of_every_golden_case(jpeg, case):
    from vn_celeb_face_recognition_amd import _lib
    data = case["jpg"]
    rc, info = jpeg.probe(data)
    assert rc == 0
    bound = jpeg.huff_prepared_bound(len(data), info)
    buf = np.full(bound + CANARY, 0x5A, np.uint8)
    rc, n = jpeg.huff_prepare(data, info, buf[:bound])
    assert rc == 0 and n <= bound and (buf[bound:] == 0x5A).all()
    blob = buf[:n].tobytes()
    head, segs = parse_blob(blob)
    mcus = (info.blocks_w[0] // info.h[0]) * (info.blocks_h[0] // info.v[0])
    ri = info.restart_interval
    assert head["ri"] == ri and head["ncomp"] == info.components
    assert head["nseg"] == len(segs) == (-(-mcus // ri) if ri else 1)
    assert all(s < head["ntables"] for s in head["dc_sel"][:info.components] + head["ac_sel"][:info.components])
    joined = b"".join(s.replace(b"\xff", b"\xff\x00") + (bytes([0xFF, 0xD0 + (i & 7)]) if i + 1 < len(segs) else b"")
                      for i, s in enumerate(segs))
    assert joined == scan_of(data)
    # one byte short: refused, nothing behind the buffer touched, the length not reported
    buf = np.full(n - 1 + CANARY, 0x5A, np.uint8)
    got = ctypes.c_int64(-7)
    rc = _lib.load().vnf_jpeg_huff_prepare(data, len(data), ctypes.byref(info), buf.ctypes.data, n - 1, ctypes.byref(got))
    assert rc == CAPACITY and got.value == -7 and (buf[n - 1:] == 0x5A).all()
    # the same bytes wherever they are written: the blob is position-independent
    again = np.zeros(n + 16, np.uint8)
    assert jpeg.huff_prepare(data, info, again[16:]) == (0, n) and again[16:].tobytes() == blob


def test_prepare_refuses_truncated_headers_and_a_wrong_restart_order(jpeg):
    rst = next(c["jpg"] for c in OK_CASES if jpeg.probe(c["jpg"])[1].restart_interval and c["jpg"].count(b"\xff\xd1"))
    rc, info = jpeg.probe(rst)
    out = np.zeros(jpeg.huff_prepared_bound(len(rst), info), np.uint8)
    assert jpeg.huff_prepare(rst, info, out)[0] == 0
    sos = rst.index(b"\xff\xda")
    for cut in (0, 1, 2, 20, sos // 2, sos, sos + 3):
        assert jpeg.huff_prepare(rst[:cut], info, out)[0] == INVALID, cut
    # RST1 where RST0 belongs; the markers swapped; a marker that is no RSTn
    first, second = rst.index(b"\xff\xd0", sos), rst.index(b"\xff\xd1", sos)
    assert first < second
    for at, byte in ((first + 1, 0xD1), (second + 1, 0xD0), (first + 1, 0xC4)):
        bad = bytearray(rst)
        bad[at] = byte
        assert jpeg.huff_prepare(bytes(bad), info, out)[0] == INVALID
        co = np.zeros(info.coef_count, np.int16)
        assert jpeg.entropy_decode(bytes(bad), info, co) == INVALID          # as the host decoder
    assert jpeg.huff_prepare(rst[:second], info, out)[0] == INVALID           # the scan ends where RST1 belongs
    # an info of other bytes
    other = next(c["jpg"] for c in OK_CASES if c["name"] == "64x48_420_noise_q95")
    assert jpeg.huff_prepare(other, info, out)[0] == INVALID
    with pytest.raises(ValueError):
        jpeg.huff_prepare(rst, info, np.zeros(out.size, np.int16))


@pytest.mark.parametrize("case", NOT_TAKEN_CASES, ids=[c["name"] for c in NOT_TAKEN_CASES])
def test_the_not_taken_goldens_are_refused(jpeg, case):
    assert len(NOT_TAKEN_CASES) == 2
    rc, _ = jpeg.probe(case["jpg"])
    assert rc == jpeg.NOT_TAKEN
    info = jpeg.probe(OK_CASES[0]["jpg"])[1]
    out = np.zeros(1 << 16, np.uint8)
    assert jpeg.huff_prepare(case["jpg"], info, out)[0] == INVALID


def test_standalone_checker_passes_under_the_sanitizers(tmp_path):
    """Three sets of files: the golden JPEGs, tests/golden/images/*.jpg, and one 256x256 noise frame (4:2:0, quality
    95): a scan of about 77 KB, over 600 subsequences at the 1024-bit default -- two full workgroup-loads of 256 and a
    remainder -- and about 19000 at 32 bits."""
    from PIL import Image
    exe = str(tmp_path / "jpeg_huff_decode_check")
    r = subprocess.run(["c++", "-std=c++17", "-g", "-O2", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        os.path.join(REPO, "tools", "jpeg_huff_decode_check.cpp"),
                        os.path.join(REPO, "vn_celeb_face_recognition_amd", "csrc", "jpeg_entropy.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    gold = []
    for c in OK_CASES:
        gold.append(str(tmp_path / (c["name"] + ".jpg")))
        with open(gold[-1], "wb") as f:
            f.write(c["jpg"])
    noise = np.random.default_rng(256).integers(0, 256, (256, 256, 3), dtype=np.uint8)
    buf = io.BytesIO()
    Image.fromarray(noise).save(buf, format="JPEG", quality=95, subsampling=2)
    assert len(buf.getvalue()) * 8 // 1024 > 2 * 256
    big = str(tmp_path / "noise_256.jpg")
    with open(big, "wb") as f:
        f.write(buf.getvalue())
    images = sorted(glob.glob(os.path.join(REPO, "tests", "golden", "images", "*.jpg")))
    assert images
    for files in (gold, images, [big]):
        r = subprocess.run([exe] + files, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stdout + r.stderr
        m = re.search(r"every file equal: (\d+) files, (\d+) damaged inputs \((\d+) decoded by both, identical\), "
                      r"host-accepted but lane-refused: (\d+)", r.stdout)
        assert m, r.stdout + r.stderr
        assert int(m.group(1)) == len(files) and int(m.group(2)) == 48 * len(files) and int(m.group(4)) == 0, r.stdout


def test_unknown_entropy_is_refused_and_device_entropy_has_no_cpu_path(jpeg):
    from vn_celeb_face_recognition_amd.video import run_stream
    data = OK_CASES[0]["jpg"]
    for bad in ("gpu", "Device", ""):
        with pytest.raises(ValueError, match="entropy"):
            jpeg.decode_batch_device([data], "cpu", None, entropy=bad)
        with pytest.raises(ValueError, match="entropy"):
            jpeg.decode_batch([data], "cpu", None, entropy=bad)
    with pytest.raises(RuntimeError, match="no CPU path"):
        jpeg.decode_batch_device([data], "cpu", None, entropy="device")
    with pytest.raises(RuntimeError, match="no CPU path"):
        jpeg.decode_batch([data], "cpu", None, entropy="device")
    import inspect
    for fn in (jpeg.decode_batch_device, jpeg.decode_batch):
        p = inspect.signature(fn).parameters["entropy"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default == "host"
    assert inspect.signature(run_stream).parameters["decode_entropy"].default == "host"


def test_both_command_lines_take_decode_entropy(capsys):
    import celeb_statistic
    import demo_video
    for mod, extra in ((demo_video, []), (celeb_statistic, ["-fidx", "0"])):
        p = mod.make_parser()
        assert p.parse_args(extra).decode_entropy == "host"
        assert p.parse_args(extra + ["--decode_entropy", "device"]).decode_entropy == "device"
        assert p.parse_args(extra + ["--decode_entropy", "host", "--host_decode"]).decode_entropy == "host"
        with pytest.raises(SystemExit):
            p.parse_args(extra + ["--decode_entropy", "gpu"])
        assert "--decode_entropy" in capsys.readouterr().err
