"""CPU-only: the host side of face extraction -- the float32 crop rectangles (`crop_rects`) against the reference's
faces through the CPU restatement, `MTCNN.select_boxes` against the reference's selections, and the loud refusals."""
import numpy as np
import pytest
from PIL import Image

import extract_golden as eg


@pytest.fixture(scope="module")
def mtcnn_cpu():
    from vn_celeb_face_recognition_amd.models import MTCNN
    return MTCNN()


def test_crop_rects_and_area_restatement_equal_every_golden_face():
    """Zero differing bytes: pins the float32 margin arithmetic, the edge clamps and the truncation of crop_rects, and
    that interpolate(mode="area").byte() on that rectangle is what the reference computed."""
    img = eg.picture()
    n = 0
    for keep_all, margin, size, boxes, _, _, faces in eg.forward_cases():
        got = eg.restate_boxes(img, boxes, size, margin)
        assert got.shape == faces.shape
        assert int((got != faces).sum()) == 0, (keep_all, margin, size)
        n += len(boxes)
    for box, margin, size, face in eg.extract_face_cases():
        got = eg.restate_boxes(img, box[None], size, margin)[0]
        assert int((got != face).sum()) == 0, (box, margin)
        n += 1
    assert n == 11


def test_crop_rects_values_dtype_and_clamps():
    from vn_celeb_face_recognition_amd.detector import crop_rects
    r = crop_rects(np.array([[10.6, 20.4, 50.2, 80.9], [-5.5, -0.5, 30.0, 700.0]], np.float32), 160, 0, 100, 90)
    assert r.dtype == np.int32 and r.tolist() == [[10, 20, 50, 80], [0, 0, 30, 90]]
    # margin 32 at image_size 160: 32 * 40 / 128 = 10 pixels, 5 to each side; float64 boxes are taken as float32
    assert crop_rects(np.array([[30.0, 30.0, 70.0, 70.0]]), 160, 32, 100, 72).tolist() == [[25, 25, 75, 72]]
    assert crop_rects(np.zeros((0, 4), np.float32), 160, 0, 10, 10).shape == (0, 4)


def test_crop_rects_raises_on_an_empty_rectangle():
    from vn_celeb_face_recognition_amd.detector import crop_rects
    ok = [10.0, 10.0, 40.0, 40.0]
    for box in ([120.0, 10.0, 150.0, 40.0],       # right of a 100-pixel-wide frame: x2 clamps to 100 <= x1
                [10.0, -40.0, 40.0, -5.0],        # above the frame
                [10.2, 10.0, 10.9, 40.0],         # narrower than a pixel
                [10.0, 10.0, float("nan"), 40.0]):
        with pytest.raises(ValueError, match="box 1 "):
            crop_rects(np.array([ok, box], np.float32), 160, 0, 100, 90)


def test_select_boxes_equals_the_reference_single_and_batch(mtcnn_cpu):
    g = eg.golden()
    pil = Image.fromarray(eg.picture())
    thr = float(g["sel/threshold"])
    tables = {t: (g["sel/%s/boxes" % t], g["sel/%s/probs" % t], g["sel/%s/points" % t]) for t in ("det", "syn")}
    picked = set()
    for m in eg.METHODS:
        for t, (b, p, q) in tables.items():
            for img in (pil, eg.picture()):                  # any input form gives the image size
                sb, sp, sq = mtcnn_cpu.select_boxes(b, p, q, img, method=m, threshold=thr)
                assert sb.shape == (1, 4) and sq.shape == (1, 5, 2) and np.ndim(sp) == 0
                assert np.array_equal(sb, g["sel/%s/%s/box" % (t, m)])
                assert sp == g["sel/%s/%s/prob" % (t, m)]
                assert np.array_equal(sq, g["sel/%s/%s/point" % (t, m)])
            if t == "syn":
                picked.add(int(np.flatnonzero((b == sb).all(axis=1))[0]))
        bb, bp, bq = mtcnn_cpu.select_boxes([tables["det"][0], tables["syn"][0]], [tables["det"][1], tables["syn"][1]],
                                            [tables["det"][2], tables["syn"][2]], [pil, pil], method=m, threshold=thr)
        assert isinstance(bb, list) and len(bb) == len(bp) == len(bq) == 2
        assert np.array_equal(np.array(bb), g["sel/batch/%s/box" % m])
        assert np.array_equal(np.array(bp), g["sel/batch/%s/prob" % m])
        assert np.array_equal(np.array(bq), g["sel/batch/%s/point" % m])
    assert len(picked) > 1          # the methods do not all agree on the synthetic table: the cases tell them apart


def test_select_boxes_empty_image_and_filtered_threshold(mtcnn_cpu):
    img = np.zeros((60, 80, 3), np.uint8)
    for m in eg.METHODS:
        assert mtcnn_cpu.select_boxes([], [], [], img, method=m) == (None, None, None)
        b, p, q = mtcnn_cpu.select_boxes([[], []], [[], []], [[], []], [img, img], method=m)
        assert b == [None, None] and p == [[None], [None]] and q == [None, None]
    # largest_over_threshold where the reference's defect would bite (mtcnn.py:431-442 filters the boxes only, so its
    # prob and point would be rows of the unfiltered tables): the largest box is under the threshold
    boxes = np.array([[0, 0, 50, 50], [10, 10, 30, 30], [5, 5, 45, 40]], np.float32)
    probs = np.array([0.5, 0.95, 0.99], np.float32)
    points = np.arange(30, dtype=np.float32).reshape(3, 5, 2)
    sb, sp, sq = mtcnn_cpu.select_boxes(boxes, probs, points, img, method="largest_over_threshold", threshold=0.9)
    assert np.array_equal(sb, boxes[[2]]) and sp == probs[2] and np.array_equal(sq, points[[2]])
    assert mtcnn_cpu.select_boxes(boxes, probs, points, img, method="largest_over_threshold", threshold=0.995) == (None, None, None)
    # mixed batch: one image with boxes, one without
    bb, bp, bq = mtcnn_cpu.select_boxes([boxes, []], [probs, []], [points, []], [img, img], method="probability")
    assert np.array_equal(bb[0], boxes[[2]]) and bb[1] is None and bp[1] == [None] and bq[1] is None
    with pytest.raises(ValueError, match="unknown method"):
        mtcnn_cpu.select_boxes(boxes, probs, points, img, method="smallest")


def test_forward_and_extract_refuse_cpu_loudly(mtcnn_cpu):
    from vn_celeb_face_recognition_amd import detector
    img = np.zeros((32, 32, 3), np.uint8)
    assert mtcnn_cpu.__call__.__func__ is type(mtcnn_cpu).forward
    with pytest.raises(RuntimeError, match="MI355X only"):
        mtcnn_cpu.forward(img)
    with pytest.raises(RuntimeError, match="MI355X only"):
        mtcnn_cpu(img, return_prob=True)
    with pytest.raises(RuntimeError, match="MI355X only"):
        mtcnn_cpu.extract(img, np.array([[2, 2, 20, 20]], np.float32), None)
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="MI355X only"):
            detector.extract_face(img, np.array([2, 2, 20, 20], np.float32))
    x = torch.tensor([0.0, 127.5, 255.0])
    assert torch.equal(detector.fixed_image_standardization(x), torch.tensor([-127.5 / 128, 0.0, 127.5 / 128]))
