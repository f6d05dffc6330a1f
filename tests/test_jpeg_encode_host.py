"""CPU: the arithmetic of the device JPEG encoder stated in NumPy (tests/jpeg_encode_restatement.py) and the host half
of the encoder (csrc/jpeg_huff_encode.cpp through ctypes: tables, geometry, the Huffman pass) against Pillow's own
files, and the streaming AVI writer.  Every comparison is exact: zero differing coefficients, identical bytes."""
import ctypes
import io

import numpy as np
import pytest

import jpeg_encode_restatement as E

GRID = [(w, h, s, q, c) for (w, h) in E.SIZES for s in (E.S444, E.S422, E.S420) for q in E.QUALITIES for c in ("noise", "ramp")]
GRID.append((1920, 1080, E.S420, 92, "noise"))
ROUND_TRIP = [(w, h, s, q, "noise") for (w, h) in E.SIZES for s in (E.S444, E.S422, E.S420) for q in (30, 100)]
ROUND_TRIP.append((130, 70, E.S420, 92, "ramp"))
CANARY = 4096


def _id(p):
    return "%dx%d_s%d_q%d_%s" % p


@pytest.fixture(scope="module")
def jpeg():
    import __graft_entry__ as ge
    ge.build()
    from vn_celeb_face_recognition_amd import jpeg as j
    return j


@pytest.fixture(scope="module")
def jenc(jpeg):
    from vn_celeb_face_recognition_amd import jpeg_encode
    return jpeg_encode


def _pillow_coefs(jpeg, data):
    rc, info = jpeg.probe(data)
    assert rc == 0
    coefs = np.zeros(info.coef_count, np.int16)
    assert jpeg.entropy_decode(data, info, coefs) == 0
    return info, coefs


@pytest.mark.parametrize("case", GRID, ids=_id)
def test_restatement_equals_pillow_coefficients(jpeg, case):
    w, h, s, q, content = case
    rgb = E.make_frame(w, h, content)
    info, want = _pillow_coefs(jpeg, E.pillow_jpeg(rgb, q, s))
    assert np.array_equal(jpeg.quant_table(info)[:2], E.quant_tables(q))
    got = E.encode_coefs(rgb, E.quant_tables(q), s)
    assert got.shape == want.shape
    assert int((got != want).sum()) == 0


@pytest.mark.parametrize("quality", [1, 30, 50, 75, 92, 100])
def test_quant_tables_equal_pillow(jenc, quality):
    from PIL import Image
    q = Image.open(io.BytesIO(E.pillow_jpeg(E.make_frame(16, 16, "ramp"), quality, E.S420))).quantization
    got = jenc.quant_tables(quality)
    assert got.dtype == np.uint8 and got.shape == (2, 64)
    assert list(got[0]) == list(q[0]) and list(got[1]) == list(q[1])
    assert np.array_equal(got, E.quant_tables(quality))


def test_quant_tables_and_info_refuse_bad_arguments(jenc):
    from vn_celeb_face_recognition_amd import _lib
    lib = _lib.load()
    buf = np.zeros((2, 64), np.uint8)
    for q in (0, 101, -5):
        assert lib.vnf_jpeg_quant_tables(q, buf[0].ctypes.data, buf[1].ctypes.data) == -1
    assert lib.vnf_jpeg_quant_tables(50, None, buf[1].ctypes.data) == -1
    info = _lib.JpegInfo()
    assert lib.vnf_jpeg_encode_info(16, 16, E.GRAY, 75, ctypes.byref(info)) == -1          # frames are RGB
    assert lib.vnf_jpeg_encode_info(16, 16, 7, 75, ctypes.byref(info)) == -1
    assert lib.vnf_jpeg_encode_info(0, 16, E.S420, 75, ctypes.byref(info)) == -1
    assert lib.vnf_jpeg_encode_info(16, 65536, E.S420, 75, ctypes.byref(info)) == -1
    assert lib.vnf_jpeg_encode_info(16, 16, E.S420, 0, ctypes.byref(info)) == -1
    assert lib.vnf_jpeg_encode_info(16, 16, E.S420, 75, None) == -1


@pytest.mark.parametrize("case", ROUND_TRIP, ids=_id)
def test_encode_info_equals_probe_and_scan_bytes_equal_pillow(jpeg, jenc, case):
    from PIL import Image
    w, h, s, q, content = case
    rgb = E.make_frame(w, h, content, seed=3)
    data = E.pillow_jpeg(rgb, q, s)
    info, coefs = _pillow_coefs(jpeg, data)
    mine = jenc.encode_info(w, h, s, q)
    assert bytes(mine) == bytes(info)                                  # every field vnf_jpeg_probe fills
    hw, hh, bw, bh, count = E.geometry(w, h, s)
    assert list(mine.blocks_w) == bw and list(mine.blocks_h) == bh and mine.coef_count == count
    out = jenc.entropy_encode(coefs, mine)
    assert out[:2] == b"\xff\xd8" and out[-2:] == b"\xff\xd9"
    a, b = data.index(b"\xff\xda"), out.index(b"\xff\xda")
    assert out[b:] == data[a:]                                         # SOS header, scan and EOI
    rc, info2 = jpeg.probe(out)
    assert rc == 0 and bytes(info2) == bytes(info)
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(out)).convert("RGB")),
                          np.asarray(Image.open(io.BytesIO(data)).convert("RGB")))
    back = np.zeros(info2.coef_count, np.int16)
    assert jpeg.entropy_decode(out, info2, back) == 0 and np.array_equal(back, coefs)


def test_restated_coefficients_make_pillows_file(jpeg, jenc):
    """the two halves together, without a GPU: restated kernels + the Huffman pass == Image.save, whole file"""
    for (w, h, s, q) in ((33, 47, E.S420, 92), (8, 24, E.S420, 75), (17, 9, E.S422, 30), (64, 48, E.S444, 100)):
        rgb = E.make_frame(w, h, "noise", seed=9)
        coefs = E.encode_coefs(rgb, E.quant_tables(q), s)
        assert jenc.entropy_encode(coefs, jenc.encode_info(w, h, s, q)) == E.pillow_jpeg(rgb, q, s)


def _guarded_encode(coefs, info, capacity):
    """entropy-encode into a buffer of exactly `capacity` bytes between two canaries -> (status, length, intact, bytes)"""
    from vn_celeb_face_recognition_amd import _lib
    buf = np.full(capacity + 2 * CANARY, 0x5A, np.uint8)
    n = ctypes.c_int64(-1)
    rc = _lib.load().vnf_jpeg_entropy_encode(coefs.ctypes.data, ctypes.byref(info), buf.ctypes.data + CANARY, capacity,
                                             ctypes.byref(n))
    intact = bool((buf[:CANARY] == 0x5A).all() and (buf[CANARY + capacity:] == 0x5A).all())
    return rc, n.value, intact, buf[CANARY:CANARY + capacity].tobytes()


def test_capacity_is_checked_on_every_write(jpeg, jenc):
    rgb = E.make_frame(33, 47, "noise")
    data = E.pillow_jpeg(rgb, 92, E.S420)
    info, coefs = _pillow_coefs(jpeg, data)
    need = len(data)
    assert _guarded_encode(coefs, info, need) == (0, need, True, data)                 # exact capacity
    rc, n, intact, _ = _guarded_encode(coefs, info, need - 1)
    assert (rc, n, intact) == (-4, need, True)                                         # VNF_E_CAPACITY, nothing outside
    for cap in (0, 1, 19, 20, 600, need // 2):                                         # inside every header segment and the scan
        rc, n, intact, got = _guarded_encode(coefs, info, cap)
        assert (rc, n, intact) == (-4, need, True) and got == data[:cap]
    from vn_celeb_face_recognition_amd import _lib
    n = ctypes.c_int64()
    assert _lib.load().vnf_jpeg_entropy_encode(coefs.ctypes.data, ctypes.byref(info), None, 0, ctypes.byref(n)) == -4
    assert n.value == need                                                             # a sizing call needs no buffer


def test_values_outside_the_baseline_range_and_bad_infos_are_refused(jpeg, jenc):
    from vn_celeb_face_recognition_amd import _lib
    info = jenc.encode_info(16, 16, E.S420, 75)
    coefs = np.zeros(info.coef_count, np.int16)
    assert _guarded_encode(coefs, info, 4096)[0] == 0
    for at, v, ok in ((5, 1023, True), (5, -1023, True), (5, 1024, False), (5, -1024, False),     # AC: category 10 is the last
                      (0, 2047, True), (0, -2047, True), (0, 2048, False), (0, -2048, False)):    # DC difference: category 11
        c = coefs.copy()
        c[at] = v
        rc, _, intact, _ = _guarded_encode(c, info, 4096)
        assert intact and (rc == 0) == ok, (at, v, rc)
    c = coefs.copy()
    c[0], c[64] = 1500, -1500                        # each DC is in range, their difference is not
    assert _guarded_encode(c, info, 4096)[0] == -1
    for field, value in (("components", 1), ("restart_interval", 4), ("coef_count", 64), ("width", 0), ("sampling", E.GRAY)):
        bad = _lib.JpegInfo.from_buffer_copy(bytes(info))
        setattr(bad, field, value)
        assert _guarded_encode(coefs, bad, 4096)[0] == -1, field
    bad = _lib.JpegInfo.from_buffer_copy(bytes(info))
    bad.quant[2][5] += 1                             # two tables are written: the chroma components share one
    assert _guarded_encode(coefs, bad, 4096)[0] == -1
    bad = _lib.JpegInfo.from_buffer_copy(bytes(info))
    bad.quant[0][0] = 0
    assert _guarded_encode(coefs, bad, 4096)[0] == -1


def test_streaming_avi_writer_reads_back_and_equals_the_batch_writer(tmp_path):
    from vn_celeb_face_recognition_amd.mjpeg_avi import MjpegAviWriter, read_mjpeg_avi, write_mjpeg_avi
    frames = [E.make_frame(33, 47, "noise", seed=i) for i in range(5)]
    jpegs = [E.pillow_jpeg(f, 92, E.S420) for f in frames]
    p, p2 = str(tmp_path / "s.avi"), str(tmp_path / "b.avi")
    wr = MjpegAviWriter(p, 25.0)
    for j in jpegs:
        wr.append(j, (33, 47))
    with pytest.raises(ValueError):
        wr.append(jpegs[0], (47, 33))
    assert wr.close() == 5
    fps, got, n = read_mjpeg_avi(p)
    assert n == 5 and fps == 25.0 and [got.compressed(i) for i in range(5)] == jpegs
    assert write_mjpeg_avi(p2, frames, 25.0, quality=92) == 5
    assert open(p, "rb").read() == open(p2, "rb").read()
    with pytest.raises(ValueError):
        MjpegAviWriter(str(tmp_path / "none.avi"), 25.0).close()


def test_merge_of_three_ranks_is_in_frame_order(tmp_path):
    import struct
    from vn_celeb_face_recognition_amd.jpeg_encode import PART_MAGIC, VideoEncoder
    from vn_celeb_face_recognition_amd.mjpeg_avi import merge_mjpeg_parts, read_mjpeg_avi
    n_frames, world, total = 2, 3, 11                # batches of 2 frames, batch b on rank b % 3, the last one short
    jpegs = {num: E.pillow_jpeg(E.make_frame(24, 8, "noise", seed=num), 75, E.S420) for num in range(1, total + 1)}
    out = str(tmp_path / "v.avi")
    parts = [VideoEncoder.part_path(out, r) for r in range(world)]
    for r, p in enumerate(parts):
        with open(p, "wb") as f:
            f.write(PART_MAGIC)
            for num in range(1, total + 1):
                if ((num - 1) // n_frames) % world == r:
                    f.write(struct.pack("<IIII", num, len(jpegs[num]), 24, 8) + jpegs[num])
    assert merge_mjpeg_parts(parts, out, 30.0) == total
    fps, got, n = read_mjpeg_avi(out)
    assert n == total and fps == 30.0
    assert [got.compressed(i) for i in range(total)] == [jpegs[num] for num in range(1, total + 1)]
    with open(parts[1], "ab") as f:                  # a frame number twice, a cut file: errors, not a silent video
        f.write(struct.pack("<IIII", 1, len(jpegs[1]), 24, 8) + jpegs[1])
    with pytest.raises(ValueError):
        merge_mjpeg_parts(parts, str(tmp_path / "w.avi"), 30.0)
    with open(parts[2], "ab") as f:
        f.write(b"\x01\x02\x03")
    with pytest.raises(ValueError):
        merge_mjpeg_parts([parts[0], parts[2]], str(tmp_path / "x.avi"), 30.0)


def test_writers_leave_nothing_behind_on_an_error(tmp_path):
    import os
    import types
    from vn_celeb_face_recognition_amd.mjpeg_avi import MjpegAviWriter, merge_mjpeg_parts, read_mjpeg_part, write_mjpeg_avi
    a, b = E.make_frame(24, 8, "noise"), E.make_frame(8, 24, "noise")
    p = str(tmp_path / "bad.avi")
    with pytest.raises(ValueError):
        write_mjpeg_avi(p, [a, a, b], 25.0)                          # a size mismatch after two good frames
    assert not os.path.exists(p)

    def failing():
        yield a
        raise RuntimeError("decoder died")
    with pytest.raises(RuntimeError):
        write_mjpeg_avi(p, failing(), 25.0)
    assert not os.path.exists(p)
    with pytest.raises(ValueError):
        write_mjpeg_avi(p, [], 25.0)
    assert not os.path.exists(p)
    wr = MjpegAviWriter(p, 25.0)
    assert wr.size is None
    wr.append(E.pillow_jpeg(a, 75, E.S420), (24, 8))
    assert wr.size == (24, 8) and os.path.exists(p)
    wr.abort()
    assert not os.path.exists(p)
    # a spool file is read record by record, and a merge that fails leaves no video
    part = str(tmp_path / "v.avi.rank0.part")
    with open(part, "wb") as f:
        f.write(b"VNFMJPG1" + b"\x01\x00\x00\x00\x05\x00\x00\x00\x18\x00\x00\x00\x08\x00\x00\x00" + b"12345" + b"\x02\x00")
    it = read_mjpeg_part(part)
    assert isinstance(it, types.GeneratorType) and next(it) == (1, (24, 8), b"12345")
    with pytest.raises(ValueError):
        next(it)                                                     # the cut second record
    with pytest.raises(ValueError):
        merge_mjpeg_parts([part], str(tmp_path / "v.avi"), 25.0)
    assert not os.path.exists(tmp_path / "v.avi")
