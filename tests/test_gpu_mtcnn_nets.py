"""R-Net and O-Net on their own, layer by layer, on the MI355X: MTCNN.debug_net runs the cascade's own launch sequence
(prefix offsets, crop, fused front, fused mid, plan, heads scatter) on a caller-made rectangle table, debug_net_tap
reads every buffer of it, and tests/mtcnn_net_reference.py restates each layer in float64 from the DECODED PREVIOUS
TAP with a derived bar (its header).  What no bar can see -- a candidate's slot, the batch offset, the chunk boundary
-- is checked bit for bit.  Four detector handles for the module: the three forms at max_batch 2, the default at 5."""
import os
import time

import numpy as np
import pytest
import torch

import mtcnn_net_reference as R
from conftest import mtcnn_state_dicts

pytestmark = pytest.mark.gpu

H, W = R.SIZES[0]
_handles = {}
_t0 = [None]
FIGS = {}      # (net, form, layer) -> [largest err / A, largest err / bar, largest err / the 4e-7 figure]


def _vnf_error():
    from vn_celeb_face_recognition_amd._lib import VnfError
    return VnfError


def _det(form, max_batch=2):
    """The module's handle of a form; the switches are read when the handle is created, so the environment is restored
    right behind it.  A fresh handle refuses a tap: no debug call precedes it."""
    from vn_celeb_face_recognition_amd.models import MTCNN
    if (form, max_batch) in _handles:
        return _handles[form, max_batch]
    if _t0[0] is None:
        _t0[0] = time.time()
    names = ("VNF_AUTOTUNE", "VNF_MTCNN_MID", "VNF_MTCNN_DTYPE")
    keep = {k: os.environ.get(k) for k in names}
    for k in names:
        os.environ.pop(k, None)
    os.environ["VNF_AUTOTUNE"] = "0"
    os.environ.update(R.FORM_ENV[form])
    try:
        det = MTCNN(device="cuda:0", max_batch=max_batch, max_height=H, max_width=W)
        det._ensure(max_batch, H, W)
    finally:
        for k, v in keep.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    with pytest.raises(_vnf_error(), match="error -1: .*precedes the tap"):
        det.debug_net_tap(2, "heads")
    _handles[form, max_batch] = det
    return det


@pytest.fixture(scope="module", autouse=True)
def _module_handles():
    yield
    if _t0[0] is not None:
        print("\n%d detector handles, %.1f s since the first" % (len(_handles), time.time() - _t0[0]))
    for k in sorted(FIGS):
        print("net %d %-5s %-6s  err/A %.3e  /bar %.3f  /4e-7 figure %.3f" % (k + tuple(FIGS[k])))
    _handles.clear()


_cache = {}


def _inputs(size):
    """frames (2,H,W,3) and the rectangles of a frame size, once."""
    if size not in _cache:
        _cache[size] = (R.frames(*size), R.rectangles(*size))
    return _cache[size]


def _oracle(size, net):
    """om._crops of every rectangle on both frames, (2, n, S, S, 3) fp32, once per size and net."""
    if (size, net) not in _cache:
        fr, rc = _inputs(size)
        c = R.oracle_crops(fr, np.repeat(np.arange(2), len(rc)), np.concatenate([rc, rc]), R.S_OF[net])
        _cache[size, net] = c.view(2, len(rc), *c.shape[1:]).numpy()
    return _cache[size, net]


def _cases(size):
    """(frames, rects, counts, (frame, rectangle) of every row) for n = 1, 17 and all: M = 1 for dense / heads, one past a
    16-row tile, and both frames with ragged last tiles."""
    fr, rc = _inputs(size)
    n = len(rc)
    assert n > 17
    yield fr[:1], rc[:1], [1], [(0, 0)]
    yield fr[:1], rc[:17], [17], [(0, k) for k in range(17)]
    yield fr, np.concatenate([rc, rc]), [n, n], [(f, k) for f in range(2) for k in range(n)]


def _f32_bits(t):
    return t.float().contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------ crops
@pytest.mark.parametrize("net", (2, 3))
@pytest.mark.parametrize("size", R.SIZES)
def test_crops_are_the_oracles_bits(size, net):
    """crop_resize_rows_kernel against om._crops (torch's area interpolation, normalised) on the same rectangles: the
    strips on 240 x 320 (every nch branch: the rectangles' chunk counts are asserted), the per-pixel gather on 233 x 317."""
    fr, rc = _inputs(size)
    nch = {R.chunk_count(r[2], r[3]) for r in rc.tolist()}
    assert {(1, 1), (2, 1), (32, 1), (33, 1)} <= nch and (size[1] != 320 or (60, 0) in nch)
    assert ((size[1] * 3) % 16 == 0) == (size == R.SIZES[0])
    det, want = _det("mid"), _oracle(size, net)
    for frames, rects, counts, rows in _cases(size):
        det.debug_net(frames, net, rects, counts)
        assert det.debug_status == 0
        raw, split, c0 = det.debug_net_tap(net, "crops")
        assert not split and c0 == 0 and raw.shape == (len(rows), R.S_OF[net], R.S_OF[net], 4)
        got = raw.view(np.float32)
        assert np.array_equal(got[..., :3], np.stack([want[f, k] for f, k in rows]))
        assert not raw[..., 3].any()


# ------------------------------------------------------------------------------------------------ layers
@pytest.mark.parametrize("net", (2, 3))
@pytest.mark.parametrize("form", R.FORMS)
def test_every_layer_within_its_bar(form, net):
    """Every tap in plan order against the float64 layer computed from the decoded previous tap; no element left out."""
    det, sd, nf = _det(form), mtcnn_state_dicts()[net - 1], R.NF_OF[net]
    for frames, rects, counts, rows in _cases(R.SIZES[0]):
        table = torch.from_numpy(det.debug_net(frames, net, rects, counts))
        assert det.debug_status == 0 and table.shape == (len(rows), nf)
        for name, written in R.tap_names(net, form):
            if not written:
                with pytest.raises(_vnf_error(), match="error -1: .*never reaches memory"):
                    det.debug_net_tap(net, name)
        raw, split, _ = det.debug_net_tap(net, "crops")
        x = R.decode_tap(raw, split)
        for layer in R.layers(net, sd, form):
            raw, split, c0 = det.debug_net_tap(net, layer.name)
            assert split == R.is_split(form) and c0 == 0 and raw.shape[0] == len(rows)
            got = R.decode_tap(raw, split)
            ok, figs = R.check_layer(layer, x, got, form)
            f = FIGS.setdefault((net, form, layer.name), [0.0, 0.0, 0.0])
            f[:] = [max(a, b) for a, b in zip(f, figs)]
            print("net %d %-5s n %2d %-6s  err/A %.3e  /bar %.3f  /4e-7 figure %.3f" % ((net, form, len(rows), layer.name) + figs))
            assert bool(ok.all()), (net, form, len(rows), layer.name, int((~ok).sum()), figs)
            if net == 2 and layer.name == "pool1":
                assert not raw[..., 28:].any()
            x = got
        h = x.reshape(len(rows), -1)
        assert float((table[:, 0].double() - R.softmax1(h)).abs().max()) <= 1e-6
        assert torch.equal(table[:, 1:].contiguous().view(torch.int32), _f32_bits(h[:, 2:nf + 1]))


# ------------------------------------------------------------------------------------------------ slots
def _all_taps(det, net, form):
    return {name: det.debug_net_tap(net, name)[0] for name, written in R.tap_names(net, form) if written}


@pytest.mark.parametrize("net", (2, 3))
@pytest.mark.parametrize("form", ("mid", "f32"))
def test_a_candidates_bits_do_not_depend_on_where_it_sits(form, net):
    """The rectangles tiled to 200 rows of one frame, and to 120 + 80 rows of two: every tap row and table row equals,
    bit for bit, the row of the same rectangle on the same frame run alone -- across 16-row tiles, wave and workgroup
    boundaries and the second frame's batch offset."""
    det = _det(form)
    fr, rc = _inputs(R.SIZES[0])
    p = len(rc)
    alone = []
    for f in range(2):
        t = det.debug_net(fr[f:f + 1], net, rc, [p])
        alone.append((t.view(np.int32), _all_taps(det, net, form)))
    tiled = rc[np.arange(200) % p]
    t = det.debug_net(fr[:1], net, tiled, [200]).view(np.int32)
    assert det.debug_status == 0
    assert np.array_equal(t, alone[0][0][np.arange(200) % p])
    for name, raw in _all_taps(det, net, form).items():
        assert np.array_equal(raw, alone[0][1][name][np.arange(200) % p]), name
    t = det.debug_net(fr, net, np.concatenate([tiled[:120], tiled[:80]]), [120, 80]).view(np.int32)
    assert np.array_equal(t[:120], alone[0][0][np.arange(120) % p]) and np.array_equal(t[120:], alone[1][0][np.arange(80) % p])
    for name, raw in _all_taps(det, net, form).items():
        assert raw.shape[0] == 200
        assert np.array_equal(raw[:120], alone[0][1][name][np.arange(120) % p]), name
        assert np.array_equal(raw[120:], alone[1][1][name][np.arange(80) % p]), name


def _chunk_case(det, net, frame_of, per_frame, chunk):
    fr, rc = _inputs(R.SIZES[0])
    p, b = len(rc), len(frame_of)
    frames = np.ascontiguousarray(fr[frame_of])
    small = det.debug_net(frames, net, np.concatenate([rc] * b), [p] * b).view(np.int32).reshape(b, p, -1)
    tiled = rc[np.arange(per_frame) % p]
    t = det.debug_net(frames, net, np.concatenate([tiled] * b), [per_frame] * b).view(np.int32).reshape(b, per_frame, -1)
    assert det.debug_status == 0
    for f in range(b):
        assert np.array_equal(t[f], small[f][np.arange(per_frame) % p]), f
    total = b * per_frame
    c0 = (total - 1) // chunk * chunk
    assert 0 < c0 and c0 % per_frame != 0          # more than one chunk, the boundary inside a frame
    raw, split, got_c0 = det.debug_net_tap(net, "heads")
    assert got_c0 == c0 and raw.shape[0] == total - c0
    # ... and the tap is that chunk: its rows are the table's rows from c0 on
    vals = _f32_bits(R.decode_tap(raw, split).reshape(total - c0, -1)[:, 2:R.NF_OF[net] + 1]).numpy()
    assert np.array_equal(vals, t.reshape(total, -1)[c0:, 1:])


def test_onet_chunk_boundary_inside_the_second_frame():
    """2 x 1100 candidates on the max_batch = 2 handle: O-Net's chunk is 2048 rows."""
    _chunk_case(_det("mid"), 3, [0, 1], 1100, 2048)


def test_rnet_chunk_boundary_on_the_five_frame_handle():
    """5 x 1700 candidates on the max_batch = 5 handle: R-Net's chunk is 8192 rows."""
    _chunk_case(_det("mid", 5), 2, [0, 1, 0, 1, 0], 1700, 8192)


# ------------------------------------------------------------------------------------------------ arguments
def test_hook_arguments_are_checked():
    det = _det("mid")
    fr, rc = _inputs(R.SIZES[0])
    err = _vnf_error()
    for net in (1, 4):
        with pytest.raises(err, match="error -1: .*neither 2 .* nor 3"):
            det.debug_net(fr[:1], net, rc[:1], [1])
    with pytest.raises(err, match="error -4: .*2049 rectangles.* 2048 rows"):
        det.debug_net(fr[:1], 2, rc[np.zeros(2049, dtype=np.int64)], [2049])
    with pytest.raises(err, match="error -4: .*3 frames.*max_batch 2"):
        det.debug_net(np.ascontiguousarray(fr[[0, 1, 0]]), 2, rc[:3], [1, 1, 1])
    outside = rc[:1].copy()
    outside[0, 3] = W + 1
    with pytest.raises(err, match="error -1: .*leaves the frame"):
        det.debug_net(fr[:1], 3, outside, [1])
    with pytest.raises(err, match="error -1: .*precedes the tap"):     # the refused calls left nothing to tap
        det.debug_net_tap(3, "heads")
    det.debug_net(fr[:1], 3, rc[:1], [1])
    with pytest.raises(err, match="error -1: .*no such tap: conv9"):
        det.debug_net_tap(3, "conv9")
    with pytest.raises(err, match="error -1: .*no such tap: pool3"):   # R-Net has none
        det.debug_net_tap(2, "pool3")
    with pytest.raises(err, match="error -1: .*precedes the tap"):     # the last call was O-Net's
        det.debug_net_tap(2, "heads")
    assert det.debug_net_tap(3, "heads")[0].shape == (1, 1, 1, 16)
    # the hook leaves the detector as it was: the same detections on a frame pair before and after it
    from conftest import load_image
    pair = np.ascontiguousarray(np.stack([load_image("mrDam_HaHo_recog.jpg")[60:60 + H, 100:100 + W]] * 2))
    before = det.detect(pair, landmarks=True)
    det.debug_net(fr, 2, np.concatenate([rc, rc]), [len(rc)] * 2)
    after = det.detect(pair, landmarks=True)
    assert sum(len(b) for b in before[0]) >= 2
    for a, b in zip(before, after):
        for ai, bi in zip(a, b):
            assert np.array_equal(np.asarray(ai), np.asarray(bi))


# Figures of the run on the MI355X (17 tests, all passed; the crops are the oracle's bits on both frame sizes, every pool
# of a stored buffer is exact, every bit check holds).  Per net, form and layer, over n = 1, 17 and 50 candidates: the
# largest |got - ref| / A, its ratio to the bar, and its ratio to the project's 4e-7 * A (+ 2^-21 * A in the split forms)
# with the same store terms -- reported, not asserted.  The exact-f32 plans exceed that figure on conv2 and dense of both
# nets and on O-Net's conv3 (1.10 .. 1.53 of it, as torch's own fp32 convolution does on the host: 1.47 / 1.53 on conv2);
# nothing comes nearer to the derived bar than 0.25 (the split fronts, where the pair's 2^-24 floor sets err / A).
#
#   R-Net        mid (default)               split (VNF_MTCNN_MID=0)     f32 (VNF_MTCNN_DTYPE=f32)
#   layer   err/A     /bar   /4e-7     err/A     /bar   /4e-7     err/A     /bar   /4e-7
#   pool1   7.08e-07  0.165  0.239     7.08e-07  0.165  0.239     3.16e-07  0.176  0.676
#   conv2   (fused)                    4.42e-07  0.028  0.376     5.91e-07  0.039  1.354
#   pool2   3.63e-07  0.023  0.309     exact                      exact
#   conv3   1.81e-07  0.015  0.161     1.81e-07  0.015  0.161     3.29e-07  0.028  0.698
#   dense   2.92e-07  0.008  0.257     2.93e-07  0.008  0.258     4.97e-07  0.014  1.104
#   heads   1.83e-07  0.021  0.134     1.61e-07  0.019  0.129     3.04e-07  0.039  0.633
#
#   O-Net
#   pool1   2.35e-06  0.252  0.434     2.35e-06  0.252  0.434     3.15e-07  0.170  0.597
#   conv2   (fused)                    1.05e-06  0.050  0.401     7.65e-07  0.044  1.526
#   pool2   1.05e-06  0.050  0.377     exact                      exact
#   conv3   4.32e-07  0.012  0.411     4.32e-07  0.012  0.411     5.95e-07  0.017  1.378
#   pool3   exact                      exact                      exact
#   conv4   2.84e-07  0.018  0.246     2.99e-07  0.018  0.239     3.63e-07  0.023  0.784
#   dense   3.93e-07  0.006  0.345     4.35e-07  0.006  0.392     5.32e-07  0.008  1.187
#   heads   3.34e-07  0.021  0.252     3.61e-07  0.022  0.272     3.59e-07  0.023  0.705
#
# Handle creations: 4 (1.5 s from the first to the module's end).  Wall time of the module: 3.6 s, of which the slowest
# test (the first: R-Net crops at 240 x 320, with the first handle and the oracle's crops) takes 0.32 s; the slowest
# layer test (default form, O-Net: three runs and their float64 layers) 0.30 s.
