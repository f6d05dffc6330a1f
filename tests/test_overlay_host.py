"""CPU: the frame overlay stated in NumPy (tests/jpeg_encode_restatement.py) and the host side of vnf_overlay_draw
(jpeg_encode.overlay_ops) against what they replace, cli_utils.draw_boxes_on_image (Pillow), byte for byte.  The
negative-anchor cases pin what the installed Pillow does with them (int() of the anchor, FreeType started at the
signed fraction)."""
import numpy as np
import pytest

import jpeg_encode_restatement as E

CASES = sorted(E.OVERLAY_CASES)


def _want(frame, boxes, names):
    from vn_celeb_face_recognition_amd.cli_utils import draw_boxes_on_image
    return draw_boxes_on_image(frame, boxes, names)


@pytest.mark.parametrize("case", CASES)
def test_restatement_equals_draw_boxes_on_image(case):
    boxes, names = E.OVERLAY_CASES[case]
    frame = E.overlay_frame()
    want = _want(frame, boxes, names)
    assert int((E.overlay(frame, boxes, names) != want).sum()) == 0
    if case not in ("wholly_outside",):
        assert (want != frame).any()                      # the case paints something


@pytest.mark.parametrize("case", CASES)
def test_ops_table_painted_in_numpy_equals_draw_boxes_on_image(case):
    from vn_celeb_face_recognition_amd import jpeg_encode
    boxes, names = E.OVERLAY_CASES[case]
    frame = E.overlay_frame()
    ops, masks = jpeg_encode.overlay_ops([boxes], [names])
    assert ops.dtype == jpeg_encode.OP_DTYPE and ops.dtype.itemsize == 32 and masks.dtype == np.uint8
    assert int((E.apply_ops(frame[None], ops, masks)[0] != _want(frame, boxes, names)).sum()) == 0


def test_ops_of_a_batch_are_in_draw_order_per_frame():
    from vn_celeb_face_recognition_amd import jpeg_encode
    frame = E.overlay_frame()
    names = sorted(E.OVERLAY_CASES)[:3]
    batch = np.stack([frame, frame[::-1], frame[:, ::-1]])
    boxes = [E.OVERLAY_CASES[n][0] for n in names]
    labels = [E.OVERLAY_CASES[n][1] for n in names]
    ops, masks = jpeg_encode.overlay_ops(boxes, labels)
    assert list(ops["frame"]) == sorted(ops["frame"])
    got = E.apply_ops(batch, ops, masks)
    for i in range(3):
        assert np.array_equal(got[i], _want(batch[i], boxes[i], labels[i]))
    # the entries of different frames may interleave: only the order inside a frame matters
    order = np.argsort(np.arange(ops.shape[0]) % 2, kind="stable")
    assert np.array_equal(E.apply_ops(batch, ops[order], masks), got)


def test_overlay_ops_checks_its_input():
    from vn_celeb_face_recognition_amd import jpeg_encode
    with pytest.raises(ValueError):
        jpeg_encode.overlay_ops([[(0, 0, 5, 5)]], [[]])
    with pytest.raises(ValueError):
        jpeg_encode.overlay_ops([[(0, 0, 5, 5)]], [["a"], ["b"]])
    with pytest.raises(ValueError):
        jpeg_encode.overlay_ops([[(float("nan"), 0, 5, 5)]], [["a"]])
    ops, masks = jpeg_encode.overlay_ops([[(30.0, 30.0, 10.0, 10.0)]], [["inverted"]])    # Pillow raises; no rectangle
    assert list(ops["kind"]) == [jpeg_encode.LABEL]
    ops, masks = jpeg_encode.overlay_ops([[(1e30, -1e30, 1e30, 1e30)]], [["far"]])
    assert ops.shape[0] <= 1 and masks.size == 0
    ops, masks = jpeg_encode.overlay_ops([[], []], [[], []])
    assert ops.shape == (0,) and masks.shape == (0,)
