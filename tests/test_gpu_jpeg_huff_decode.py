"""GPU: the Huffman pass of the JPEG frame decoder on the device (csrc/jpeg_huff_decode.hip behind
vnf_jpeg_huff_prepare, jpeg.py entropy="device", run_stream decode_entropy="device", --decode_entropy device).  Expected
coefficients: the host decoder's (jpeg.entropy_decode, itself pinned to Pillow by tests/test_jpeg_host.py); expected
pixels: Pillow's.  Every comparison is exact; the coefficients, the statuses and the workspace sit between guard
regions that must come back untouched."""
import ctypes
import io

import numpy as np
import pytest
import torch

import jpeg_restatement as R
from conftest import load_image

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 4096       # bytes on either side of every buffer the call writes (a multiple of 16: the alignments hold)
OK_CASES = [c for c in R.load_cases()[0] if c["expect"] == "ok"]
INVALID = -1


def _jpeg():
    from vn_celeb_face_recognition_amd import jpeg
    return jpeg


def _guarded(nbytes):
    whole = torch.full((nbytes + 2 * GUARD,), 0x5A, dtype=torch.uint8, device=DEV)
    return whole, whole[GUARD:GUARD + nbytes]


def _intact(whole, nbytes):
    host = whole.cpu().numpy()
    return bool((host[:GUARD] == 0x5A).all() and (host[GUARD + nbytes:] == 0x5A).all())


def _encode(rgb, **kw):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(rgb).save(buf, format="JPEG", **kw)
    return buf.getvalue()


def prepare(data, info):
    """-> the blob of one frame (uint8 numpy of exactly its length)"""
    jpeg = _jpeg()
    out = np.zeros(jpeg.huff_prepared_bound(len(data), info), np.uint8)
    rc, n = jpeg.huff_prepare(data, info, out)
    assert rc == 0 and 64 <= n <= out.size and n % 16 == 0
    return out[:n].copy()


def device_huff_decode(blobs, info, subseq_bits=0, sizes=None, stream=None):
    """blobs (list of uint8 numpy) of one geometry through vnf_jpeg_huff_decode_frames -> (status (n) int32,
    coefs (n, coef_count) int16), numpy.  sizes: the blob sizes handed to the call (default: the real ones)."""
    jpeg = _jpeg()
    n, cc = len(blobs), int(info.coef_count)
    offs, at = [], 0
    for b in blobs:
        offs.append(at)
        at += (b.size + 15) & ~15
    sizes = [b.size for b in blobs] if sizes is None else sizes
    flat = np.full(at, 0xEE, np.uint8)
    for o, b in zip(offs, blobs):
        flat[o:o + b.size] = b
    ws_bytes = jpeg.huff_decode_workspace_bytes(n, info, max(sizes), subseq_bits)
    bufs = [_guarded(n * cc * 2), _guarded(4 * n), _guarded(ws_bytes)]
    (_, coefs), (_, status), (_, ws) = bufs
    dev = torch.from_numpy(flat).to(DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
        jpeg.huff_decode_frames(dev, offs, sizes, info, coefs.view(torch.int16), status.view(torch.int32), ws, subseq_bits)
    torch.cuda.synchronize()
    for (whole, _), nbytes in zip(bufs, (n * cc * 2, 4 * n, ws_bytes)):
        assert _intact(whole, nbytes)
    return status.view(torch.int32).cpu().numpy(), coefs.view(torch.int16).cpu().numpy().reshape(n, cc)


def host_coefs(data, info):
    co = np.zeros(info.coef_count, np.int16)
    return _jpeg().entropy_decode(data, info, co), co


def check_frames(frames, subseq_bits):
    """frames of one geometry: every one decodes on the device to the host decoder's coefficients"""
    jpeg = _jpeg()
    infos = [jpeg.probe(d)[1] for d in frames]
    status, coefs = device_huff_decode([prepare(d, i) for d, i in zip(frames, infos)], infos[0], subseq_bits)
    assert list(status) == [0] * len(frames)
    for k, (d, i) in enumerate(zip(frames, infos)):
        rc, want = host_coefs(d, i)
        assert rc == 0 and np.array_equal(coefs[k], want), k
    return coefs


@pytest.mark.parametrize("subseq_bits", [32, 0], ids=["32", "default"])
def test_every_golden_case_equals_the_host_decoder(subseq_bits):
    """One call per geometry: frames with other tables and other restart intervals share a batch.  At 32 bits the
    3.6 KB scan of 64x48_420_noise_q95 is about 900 lanes (several loads); the restart cases give many short segments,
    some shorter than one subsequence."""
    jpeg = _jpeg()
    groups = {}
    for c in OK_CASES:
        rc, info = jpeg.probe(c["jpg"])
        assert rc == 0
        groups.setdefault((info.width, info.height, info.sampling), []).append(c["jpg"])
    assert any(len(g) > 1 for g in groups.values())
    assert any(jpeg.probe(c["jpg"])[1].restart_interval for c in OK_CASES)
    for frames in groups.values():
        check_frames(frames, subseq_bits)


@pytest.fixture(scope="module")
def noise_256():
    return np.random.default_rng(256).integers(0, 256, (256, 256, 3), dtype=np.uint8)


@pytest.fixture(scope="module")
def jpeg_1080p():
    from vn_celeb_face_recognition_amd.synth import make_frames
    frames, _ = make_frames(1, 8, seed=5)
    return _encode(frames[0], quality=92, subsampling=2)


def test_noise_frame_spans_loads_with_and_without_restarts(noise_256):
    """256x256 noise, 4:2:0, quality 95: a scan of about 77 KB -- over 600 lanes at the default 1024 bits (two full
    loads of 256 and a remainder), about 19000 at 32.  restart_marker_rows=1: 16 segments, each longer than one
    subsequence."""
    plain = _encode(noise_256, quality=95, subsampling=2)
    rst = _encode(noise_256, quality=95, subsampling=2, restart_marker_rows=1)
    assert len(plain) * 8 // 1024 > 2 * 256 and _jpeg().probe(rst)[1].restart_interval == 16
    for sb in (0, 32, 4096):
        a = check_frames([plain, rst], sb)
        assert np.array_equal(a[0], a[1])


def test_1080p_frame_is_decoded_and_repeats(jpeg_1080p):
    """At the default: about 4700 lanes in one group of loads.  At 32 bits: about 150000 lanes, more than 256 loads, so
    the second synchronise level takes several launches.  Twice: identical bytes."""
    rc, info = _jpeg().probe(jpeg_1080p)
    assert rc == 0 and (info.width, info.height) == (1920, 1080)
    a = check_frames([jpeg_1080p], 0)
    assert np.array_equal(a, check_frames([jpeg_1080p], 0))
    assert len(jpeg_1080p) * 8 // 32 > 256 * 256
    assert np.array_equal(a, check_frames([jpeg_1080p], 32))


def _flipped_frame_the_host_refuses(data, info):
    """a copy of `data` with one bit of its scan flipped that prepares, that the host decoder refuses and that Pillow
    still decodes (libjpeg warns and goes on)"""
    jpeg = _jpeg()
    scan = data.index(b"\xff\xda") + 14
    rng = np.random.default_rng(3)
    for _ in range(400):
        b = bytearray(data)
        b[int(rng.integers(scan, len(data) - 2))] ^= 1 << int(rng.integers(0, 8))
        b = bytes(b)
        out = np.zeros(jpeg.huff_prepared_bound(len(b), info), np.uint8)
        if jpeg.huff_prepare(b, info, out)[0] != 0 or host_coefs(b, info)[0] == 0:
            continue
        try:
            jpeg.decode_host(b)
        except Exception:
            continue
        return b
    raise AssertionError("no such flip among 400")


def test_mixed_batch_statuses_are_per_frame():
    jpeg = _jpeg()
    names = ["33x47_420_q75", "33x47_420_q30", "33x47_420_q100"]
    good = [next(c["jpg"] for c in OK_CASES if c["name"] == n) for n in names]
    info = jpeg.probe(good[0])[1]
    flipped = _flipped_frame_the_host_refuses(good[0], info)
    blobs = [prepare(good[0], info), prepare(good[1], jpeg.probe(good[1])[1]), prepare(flipped, info),
             prepare(good[2], jpeg.probe(good[2])[1]), prepare(good[1], jpeg.probe(good[1])[1])]
    cut = good[2][:len(good[2]) - 40]                          # a truncated file: it prepares, its last segment ends early
    assert host_coefs(cut, info)[0] == INVALID
    blobs.append(prepare(cut, jpeg.probe(cut)[1]))
    sizes = [b.size for b in blobs]
    sizes[1] = (sizes[1] * 2 // 3) & ~15                       # a blob cut short: its last segment ends past the size
    for sb in (32, 0):
        status, coefs = device_huff_decode(blobs, info, sb, sizes=sizes)
        assert list(status) == [0, INVALID, INVALID, 0, 0, INVALID]
        for k, d in ((0, good[0]), (3, good[2]), (4, good[1])):
            rc, want = host_coefs(d, jpeg.probe(d)[1])
            assert rc == 0 and np.array_equal(coefs[k], want)
    # through the Python layer: the batch falls back, and the pixels are Pillow's
    from vn_celeb_face_recognition_amd.upload import FrameUploader
    up = FrameUploader(DEV, depth=3)
    try:
        batch = [good[0], flipped, good[1]]
        assert jpeg.decode_batch_device(batch, DEV, up, entropy="device") is None
        dev, ev, slot, host = jpeg.decode_batch(batch, DEV, up, entropy="device")
        ev.synchronize()
        got = dev.cpu().numpy()
        for i, d in enumerate(batch):
            assert np.array_equal(got[i], jpeg.decode_host(d)) and np.array_equal(host[i], jpeg.decode_host(d))
        up.release(slot, ev)
        # a truncated file prepares (its last segment just ends early) and is refused by the lanes: the same way down
        assert jpeg.decode_batch_device([good[0], good[0][:len(good[0]) - 40]], DEV, up, entropy="device") is None
        # and the ring still serves a good batch afterwards
        r = jpeg.decode_batch_device(good, DEV, up, entropy="device")
        r[1].synchronize()
        assert all(np.array_equal(r[0].cpu().numpy()[i], jpeg.decode_host(d)) for i, d in enumerate(good))
        up.release(r[2], r[1])
    finally:
        up.close()


def test_decode_batch_device_gives_the_same_rgb_with_either_entropy(noise_256):
    """per-frame tables: quality 30, quality 92 and optimize=True (Huffman tables of the frame's own)"""
    from vn_celeb_face_recognition_amd.upload import FrameUploader
    jpeg = _jpeg()
    a = np.ascontiguousarray(load_image("mrDam_HaHo_recog.jpg")[:200, :312])
    noise = np.ascontiguousarray(np.resize(noise_256, (200, 312, 3)))
    frames = [_encode(a, quality=30, subsampling=2), _encode(a, quality=92, subsampling=2),
              _encode(a, quality=92, subsampling=2, optimize=True), _encode(noise, quality=92, subsampling=2, optimize=True)]
    up = FrameUploader(DEV, depth=3)
    try:
        got = {}
        for entropy in jpeg.ENTROPY:
            tm = {}
            r = jpeg.decode_batch_device(frames, DEV, up, timing=tm, entropy=entropy)
            assert r is not None and r[2] >= 0
            r[1].synchronize()
            got[entropy] = (r[0].cpu().numpy(), tm["upload_bytes"])
            up.release(r[2], r[1])
        assert np.array_equal(got["host"][0], got["device"][0])
        for i, d in enumerate(frames):
            assert np.array_equal(got["device"][0][i], jpeg.decode_host(d))
        assert got["device"][1] < got["host"][1]                  # the compressed frames are the smaller upload
        r = jpeg.decode_batch_device(frames, DEV, up, entropy="device", subseq_bits=64)
        r[1].synchronize()
        assert np.array_equal(r[0].cpu().numpy(), got["host"][0])
        up.release(r[2], r[1])
        with pytest.raises(ValueError, match="subseq_bits"):
            jpeg.decode_batch_device(frames, DEV, up, entropy="device", subseq_bits=48)
    finally:
        up.close()


def test_run_stream_writes_the_same_rows_with_either_decode_entropy(tmp_path, monkeypatch):
    from vn_celeb_face_recognition_amd import jpeg, models
    from vn_celeb_face_recognition_amd.cli_utils import open_frame_source
    from vn_celeb_face_recognition_amd.mjpeg_avi import write_mjpeg_avi
    from vn_celeb_face_recognition_amd.pipeline import FacePipeline
    from vn_celeb_face_recognition_amd.video import run_stream
    a = load_image("mrDam_HaHo_recog.jpg")
    m = np.ascontiguousarray(a[:, ::-1])
    avi = str(tmp_path / "clip.avi")
    assert write_mjpeg_avi(avi, [a, m, a, m], 25.0) == 4
    det = models.MTCNN(keep_all=True, min_face_size=50, device=DEV, max_batch=2, max_height=a.shape[0], max_width=a.shape[1])
    enc = models.InceptionResnetV1(pretrained=None, compute_dtype="f32", max_batch=16).to(DEV).eval()
    clf = models.MLPModel(512, 1001).to(DEV).eval()
    pipe = FacePipeline(det, enc, clf, {"label": list(range(1001)), "name": ["c%d" % i for i in range(1001)]}, 160, 0.0)
    taken = []
    real = jpeg._decode_batch_huff_device

    def spy(frames, uploader, timing, subseq_bits):
        r = real(frames, uploader, timing, subseq_bits)
        taken.append(r is not None)
        return r

    monkeypatch.setattr(jpeg, "_decode_batch_huff_device", spy)
    rows_host, n_host = run_stream(open_frame_source(avi), pipe, 2, device=DEV)
    assert taken == []
    rows_dev, n_dev = run_stream(open_frame_source(avi), pipe, 2, device=DEV, decode_entropy="device")
    assert taken == [True, True] and n_host == n_dev == 4
    assert rows_dev == rows_host and sorted(rows_dev) == [1, 2, 3, 4]
    assert sum("c" in rows_dev[k].split(",")[1] for k in rows_dev) == 4       # faces were found and named on every frame
    with pytest.raises(ValueError, match="decode_entropy"):
        run_stream(open_frame_source(avi), pipe, 2, device=DEV, decode_entropy="gpu")
    torch.cuda.synchronize()


def test_documented_statuses():
    from vn_celeb_face_recognition_amd import _lib
    jpeg = _jpeg()
    lib = _lib.load()
    st = _lib.current_stream_ptr()
    data = next(c["jpg"] for c in OK_CASES if c["name"] == "33x47_420_q75")
    info = jpeg.probe(data)[1]
    blob = prepare(data, info)
    cc = int(info.coef_count)
    one = ctypes.c_int64 * 1
    assert lib.vnf_jpeg_huff_decode_frames(None, None, None, 0, ctypes.byref(info), 0, None, None, None, 0, st) == 0   # n == 0
    ws_bytes = jpeg.huff_decode_workspace_bytes(1, info, blob.size)
    dev = torch.from_numpy(np.concatenate([blob, np.zeros(32, np.uint8)])).to(DEV)
    coefs = torch.full((cc + 8,), 77, dtype=torch.int16, device=DEV)
    status = torch.full((1,), 9, dtype=torch.int32, device=DEV)
    ws = torch.zeros((ws_bytes + 16,), dtype=torch.uint8, device=DEV)

    def call(inf=info, blobs=None, off=0, size=blob.size, sb=0, cp=None, sp=None, wp=None, nbytes=ws_bytes, n=1):
        return lib.vnf_jpeg_huff_decode_frames(
            dev.data_ptr() if blobs is None else blobs, one(off), one(size), n, ctypes.byref(inf), sb,
            coefs.data_ptr() if cp is None else cp, status.data_ptr() if sp is None else sp,
            ws.data_ptr() if wp is None else wp, nbytes, st)

    def changed(**fields):
        bad = _lib.JpegInfo.from_buffer_copy(bytes(info))
        for k, v in fields.items():
            setattr(bad, k, v)
        return bad

    assert call(n=-1) == -1
    assert call(blobs=0) == -1 and call(cp=0) == -1 and call(sp=0) == -1 and call(wp=0) == -1              # NULL
    assert lib.vnf_jpeg_huff_decode_frames(dev.data_ptr(), None, one(blob.size), 1, ctypes.byref(info), 0, coefs.data_ptr(),
                                           status.data_ptr(), ws.data_ptr(), ws_bytes, st) == -1
    assert call(blobs=dev.data_ptr() + 8) == -1 and call(wp=ws.data_ptr() + 8) == -1                        # misaligned
    assert call(cp=coefs.data_ptr() + 1) == -1 and call(sp=status.data_ptr() + 2) == -1 and call(off=8) == -1
    assert call(off=-16) == -1 and call(size=-1) == -1 and call(size=(1 << 28) + 16) == -1
    for sb in (16, 31, 48, 8192 + 32, -32):
        assert call(sb=sb) == -1 and lib.vnf_jpeg_huff_decode_workspace_bytes(1, ctypes.byref(info), blob.size, sb) == -1
    assert call(changed(sampling=7)) == -1 and call(changed(coef_count=cc + 64)) == -1 and call(changed(width=0)) == -1
    assert lib.vnf_jpeg_huff_decode_workspace_bytes(-1, ctypes.byref(info), blob.size, 0) == -1
    assert lib.vnf_jpeg_huff_decode_workspace_bytes(1, ctypes.byref(info), -1, 0) == -1
    assert call(nbytes=ws_bytes - 1) == -4                                                                 # VNF_E_CAPACITY
    assert jpeg.huff_decode_workspace_bytes(1, info, blob.size, 32) > ws_bytes
    assert call(sb=32) == -4                                     # more lanes than this workspace was sized for
    torch.cuda.synchronize()
    assert int(status.item()) == 9 and bool((coefs == 77).all())                  # a refused call enqueues nothing
    assert call() == 0
    torch.cuda.synchronize()
    rc, want = host_coefs(data, info)
    got = coefs.cpu().numpy()
    assert rc == 0 and int(status.item()) == 0 and np.array_equal(got[:cc], want) and (got[cc:] == 77).all()
    # a blob of garbage, and one whose header promises more than its size: refused, inside their buffers
    junk = np.random.default_rng(1).integers(0, 256, blob.size, dtype=np.uint8)
    lying = blob.copy()
    lying[8:12] = np.frombuffer(np.uint32(0x7FFFFFFF).tobytes(), np.uint8)        # nseg
    rst = next(c["jpg"] for c in OK_CASES if c["name"].startswith("33x47_420") and jpeg.probe(c["jpg"])[1].restart_interval)
    over = prepare(rst, jpeg.probe(rst)[1])
    seg_at = int(np.frombuffer(over[24:28].tobytes(), np.uint32)[0])
    over[seg_at + 8:seg_at + 12] = over[seg_at:seg_at + 4]                        # the second segment on top of the first
    status2, _ = device_huff_decode([junk, lying, blob, over], info)
    assert list(status2) == [INVALID, INVALID, 0, INVALID]
