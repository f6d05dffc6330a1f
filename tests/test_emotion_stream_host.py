"""CPU: emotions through the frame stream.  The text-run specification (tests/text_overlay_restatement.py) against
Pillow itself, the host tables of vnf_overlay_draw_text, video.run_stream(emotions=k) on one rank and on two gloo
ranks, the sampled FrameSource, and the exported symbol.  Every picture comparison is exact."""
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

import jpeg_encode_restatement as E
import text_overlay_restatement as T
from conftest import GOLDEN, REPO
from test_host_logic import _StubPipe, _StubTicket, _frames_for

K = 6
NTAGS = 690


def _tags():
    return json.load(open(os.path.join(GOLDEN, "etag2idx.json")))["idx2key"]


def _pillow_text(frame, calls, colour=(0, 255, 0)):
    from PIL import Image, ImageDraw
    im = Image.fromarray(frame.copy())
    d = ImageDraw.Draw(im)
    for x, y, s in calls:
        d.text((x, y), s, fill=colour)
    return np.asarray(im)


# ------------------------------------------------------------------------------------------------ the specification
def test_rounded_division_is_the_shift_form_the_kernel_uses():
    x = np.arange(0, 255 * 255 + 1, dtype=np.int64)
    v = x + 128
    assert np.array_equal(T.round_div255(x), ((v >> 8) + v) >> 8)
    assert np.array_equal(T.round_div255(x), np.floor(x / 255.0 + 0.5).astype(np.int64))


def test_restatement_equals_pillow_for_every_tag():
    """'{tag} - {p:.2f}%' for every tag of etag2idx.json at 0.00 %, 100.00 % and a seeded percentage, on noise"""
    assert T.font_is_additive()
    tags = _tags()
    assert len(tags) == NTAGS and max(len(t) for t in tags) == 16
    rng = np.random.default_rng(5)
    noise = rng.integers(0, 256, (20, 190, 3), dtype=np.uint8)
    bad = []
    for t in tags:
        for p in (0.0, 100.0, float(rng.random() * 100)):
            s = "{} - {:.2f}%".format(t, p)
            got = noise.copy()
            T.draw_text(got, 3, 2, s)
            if not np.array_equal(got, _pillow_text(noise, [(3, 2, s)])):
                bad.append(s)
    assert not bad, bad[:5]


EDGE_BOXES = [(-9.3, -7.8, 30.0, 40.0),       # negative anchors: lines start left of and above the frame
              (52.6, 3.2, 79.0, 30.0),        # lines run off the right edge
              (10.5, 36.9, 40.0, 47.0),       # lines run off the bottom edge (and lie below it)
              (12.2, 20.4, 50.0, 44.0),       # over the first face's lines: two runs on top of each other
              (14.7, 22.1, 50.0, 44.0)]


def _edge_case(seed=11, k=3):
    rng = np.random.default_rng(seed)
    tags = _tags()
    frame = rng.integers(0, 256, (48, 80, 3), dtype=np.uint8)
    t = [[tags[int(i)] for i in rng.integers(0, NTAGS, k)] for _ in EDGE_BOXES]
    p = [np.sort(rng.random(k).astype(np.float32))[::-1] for _ in EDGE_BOXES]
    return frame, [np.array(b, np.float32) for b in EDGE_BOXES], t, p


def test_restatement_equals_draw_emotions_across_every_edge():
    from vn_celeb_face_recognition_amd.cli_utils import draw_emotions
    frame, boxes, t, p = _edge_case()
    want = draw_emotions(frame, boxes, t, p)
    lines = T.emotion_lines(boxes, t, p)
    assert min(l[1] for l in lines) < 0 and min(l[2] for l in lines) < 0
    assert max(l[1] for l in lines) > 40 and max(l[2] for l in lines) >= 48
    assert np.array_equal(T.draw_emotions(frame, boxes, t, p), want) and (want != frame).any()


# ------------------------------------------------------------------------------------------------ the host tables
@pytest.fixture(scope="module")
def jenc():
    import __graft_entry__ as ge
    ge.build()
    from vn_celeb_face_recognition_amd import jpeg_encode
    return jpeg_encode


def _runs_as_lines(runs, chars):
    return [(int(r["frame"]), int(r["x"]), int(r["y"]), bytes(chars[r["first"]:r["first"] + r["length"]]).decode("ascii")) for r in runs]


def test_atlas_holds_the_restatements_glyphs(jenc):
    atlas, g = jenc.text_atlas(), T.glyphs()
    assert atlas is not None and atlas["glyphs"].shape[0] == T.LAST - T.FIRST + 1
    for c in range(T.FIRST, T.LAST + 1):
        a, (m, ox, oy, adv) = atlas["glyphs"][c - T.FIRST], g[chr(c)]
        assert int(a["advance"]) == adv and (int(a["w"]), int(a["h"])) == (m.shape[1], m.shape[0])
        if m.size:
            assert (int(a["ox"]), int(a["oy"])) == (ox, oy)
            assert np.array_equal(atlas["coverage"][a["offset"]:a["offset"] + m.size].reshape(m.shape), m)
    head = atlas["bytes"][:8].view("<i4")
    assert head.tolist() == [T.FIRST, T.LAST - T.FIRST + 1]
    assert atlas["bytes"].size == 8 + atlas["glyphs"].nbytes + atlas["coverage"].size


def test_text_runs_order_launches_and_fall_back(jenc):
    frame, boxes, t, p = _edge_case()
    lines = jenc.emotion_lines([boxes], [t], [p])
    assert lines == T.emotion_lines(boxes, t, p)
    runs, chars, ends, ops, masks = jenc.text_runs(lines)
    assert ops.shape[0] == 0 and runs.shape[0] == len(lines) and ends[-1] == runs.shape[0]
    assert len(ends) >= 2                                        # the faces that overlap need a second launch
    # launch by launch the runs are disjoint, and painting them in table order is painting them in draw order
    assert np.array_equal(T.draw_runs(frame[None], _runs_as_lines(runs, chars)), T.draw_runs(frame[None], lines))
    lo = 0
    for hi in ends:
        seen = np.zeros(frame.shape[:2], bool)
        for ln in _runs_as_lines(runs[lo:hi], chars):
            one = (T.draw_runs(np.zeros_like(frame)[None], [ln])[0] != 0).any(axis=2)
            ys, xs = np.nonzero(one)
            if ys.size:
                rect = np.zeros_like(seen)
                rect[ys.min():ys.max() + 1, xs.min():xs.max() + 1] = True
                assert not (seen & rect).any()
                seen |= rect
        lo = hi
    apart = [(0, 2, 2, "a - 1.00%"), (0, 2, 20, "b - 2.00%"), (1, 2, 2, "c - 3.00%"), (0, 2, 30, ""), (0, 40, 2, "   ")]
    runs, chars, ends, ops, _ = jenc.text_runs(apart)
    assert ends.tolist() == [3] and runs.shape[0] == 3 and ops.shape[0] == 0      # no ink: no run
    # a line outside the atlas takes its whole frame to the LABEL path, and the picture is Pillow's either way
    # ('s' and ')' start a pixel left of the pen: their first ink column must survive the LABEL path too)
    mixed = [(0, 4, 3, "vui - 12.50%"), (0, 6, 9, "buồn - 7.25%"), (1, 4, 3, "vui - 1.00%"), (0, 30, 20, "x" * 65),
             (0, 3, 30, "sầu - 1.00%"), (0, 0, 38, ") sad - 3.00%")]
    frames = np.random.default_rng(3).integers(0, 256, (2, 48, 80, 3), dtype=np.uint8)
    runs, chars, ends, ops, masks = jenc.text_runs(mixed)
    assert runs.shape[0] == 1 and int(runs[0]["frame"]) == 1 and ops.shape[0] == 5 and (ops["kind"] == jenc.LABEL).all()
    got = T.draw_runs(E.apply_ops(frames, ops, masks), _runs_as_lines(runs, chars))
    want = np.stack([_pillow_text(frames[0], [(x, y, s) for f, x, y, s in mixed if f == 0]),
                     _pillow_text(frames[1], [(x, y, s) for f, x, y, s in mixed if f == 1])])
    assert np.array_equal(got, want)
    # no atlas (a font whose strings are not the sum of their glyphs): everything is a LABEL
    apart += [(1, 30, 20, "sad - 1.00%"), (1, -1, 34, "surprise - 55.12%"), (0, 50, 30, "]; - 2.00%")]
    runs, _, ends, ops, masks = jenc.text_runs(apart, atlas=None)
    assert runs.shape[0] == 0 and ends.size == 0 and ops.shape[0] == 6
    want = T.draw_runs(frames, apart)
    assert np.array_equal(E.apply_ops(frames, ops, masks), want)
    assert np.array_equal(want, np.stack([_pillow_text(frames[i], [(x, y, s) for f, x, y, s in apart if f == i]) for i in range(2)]))
    # every tag, both ways, the same picture (the measurement tool compares exactly this on the device)
    rows = [(0, 3, 2, "{} - {:.2f}%".format(t, 12.5)) for t in _tags()]
    wide = np.random.default_rng(4).integers(0, 256, (1, 16, 190, 3), dtype=np.uint8)
    for ln in rows[::7]:
        _, _, _, ops, masks = jenc.text_runs([ln], atlas=None)
        assert np.array_equal(E.apply_ops(wide, ops, masks), T.draw_runs(wide, [ln])), ln


def test_header_declares_and_library_exports_the_text_entry_point(jenc):
    from vn_celeb_face_recognition_amd import _lib
    hdr = open(os.path.join(REPO, "include", "vnface.h")).read()
    assert "vnf_overlay_draw_text" in set(re.findall(r"\b(vnf_[a-z0-9_]+)\s*\(", hdr))
    assert hasattr(_lib.load(), "vnf_overlay_draw_text") and "vnf_overlay_draw_text" in _lib.SIGNATURES
    for name, dt in (("vnf_text_run", jenc.RUN_DTYPE), ("vnf_text_glyph", jenc.GLYPH_DTYPE)):
        body = re.search(r"typedef struct \{([^}]*)\} %s;" % name, hdr).group(1)
        fields = re.findall(r"\b([a-z0-9_]+)\s*[,;]", body)
        assert fields == list(dt.names) and dt.itemsize == 4 * len(fields)
    assert int(re.search(r"#define VNF_TEXT_RUN_MAX (\d+)", hdr).group(1)) == jenc.TEXT_RUN_MAX
    assert int(re.search(r"#define VNF_TEXT_GLYPH_MAX (\d+)", hdr).group(1)) == jenc.TEXT_GLYPH_MAX


# ------------------------------------------------------------------------------------------------ the stream
class _EmoTicket(_StubTicket):
    pass


class _EmoPipe(_StubPipe):
    """_StubPipe whose tickets carry top-K emotions that depend on the frame number and the face alone"""

    def submit(self, frames_dev, classify=True):
        t = super().submit(frames_dev, classify)
        counts, boxes = t.result()[0], t.result()[1]
        n = int(sum(counts))
        t.emo_idx = torch.zeros((n, K), dtype=torch.int32)
        t.emo_prob = torch.zeros((n, K), dtype=torch.float32)
        for o in range(n):
            frame, face = int(boxes[o][0]), int(boxes[o][1])
            t.emo_idx[o] = (torch.arange(K) * 97 + frame * 7 + face * 3) % NTAGS
            t.emo_prob[o] = 1.0 / (torch.arange(K) + 2 + face + (frame % 5) * 0.125)
        return t


def _emo_row(tm, num, names, boxes, shape, emotions=None):
    from vn_celeb_face_recognition_amd.video import tracker_row
    line = tracker_row(tm, num, names, boxes, shape)
    if emotions is None:
        return line
    idx, prob = emotions
    assert idx.dtype == np.int64 and idx.shape == prob.shape == (len(names), K)
    return line[:-1] + ',"%s","%s"\n' % (idx.tolist(), [[float(v) for v in r] for r in prob])


def _keep(count):
    from vn_celeb_face_recognition_amd.statistics import frame_is_sampled
    return frame_is_sampled(count, 4.0, [1, 3])


def _emo_stream(rank, world, n_total, n_frames, cap, sampled, k=K):
    from vn_celeb_face_recognition_amd.video import FrameSource, run_stream
    frames = _frames_for(n_total)
    # sampled == "iter": a decoder-like source, whose kept frames' numbers are learnt as the stream is pulled
    src = FrameSource(iter(list(frames)) if sampled == "iter" else frames, 4.0 if sampled else 25.0,
                      keep=_keep if sampled else None)
    seen = {}

    def on_frame(frame, number, names, boxes, emotions=None):
        seen[number] = None if emotions is None else (emotions[0].tolist(), emotions[1].tolist(), len(names))
    rows, processed = run_stream(src, _EmoPipe(), n_frames, rank, world, device="cpu", cap=cap, on_frame=on_frame,
                                 emotions=k, row=_emo_row)
    return rows, processed, src.reads, seen


def _emo_worker(rank, world, port, q, n_total, n_frames, cap, sampled):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    sys.path.insert(0, REPO)
    import torch.distributed as dist
    from vn_celeb_face_recognition_amd import dist as vdist
    vdist.init_from_env("gloo")
    rows, processed, reads, seen = _emo_stream(rank, world, n_total, n_frames, cap, sampled)
    q.put((rank, processed, reads, seen, "".join(rows[k] for k in sorted(rows)) if rank == 0 else ""))
    dist.barrier()
    dist.destroy_process_group()


def _want_emotions(num, n_faces):
    idx = [[(j * 97 + num * 7 + f * 3) % NTAGS for j in range(K)] for f in range(n_faces)]
    prob = [[float(np.float32(1.0) / np.float32(j + 2 + f + (num % 5) * 0.125)) for j in range(K)] for f in range(n_faces)]
    return idx, prob


# (frames, batch, cap, sampled): 5 batches (rank 1 sends an empty block in the last round); a cap below a batch's faces
# (the spill gather); the same two on a sampled source (23 frames at 4 fps, -fidx 1 3: 12 kept, 3 batches)
# and a sampled plain iterator (rank 0 derives the other rank's frame numbers from what it has pulled itself), also with
# one-frame batches: 11 rounds, more than the retire lag
STREAMS = [(19, 4, None, False), (19, 4, 2, False), (23, 4, None, True), (23, 4, 2, True), (21, 1, None, "iter"),
           (23, 4, None, "iter")]


@pytest.mark.parametrize("n_total,n_frames,cap,sampled", STREAMS)
def test_stream_carries_emotions_one_rank_equals_two_gloo_ranks(n_total, n_frames, cap, sampled):
    import torch.multiprocessing as mp
    rows1, p1, reads1, seen1 = _emo_stream(0, 1, n_total, n_frames, cap, sampled)
    numbers = [n for n in range(1, n_total + 1) if not sampled or _keep(n)]
    assert sorted(rows1) == numbers == sorted(seen1) and p1 == reads1 == len(numbers)
    fps = 4.0 if sampled else 25.0
    for num in numbers:                                          # number and time are the original stream's
        cells = rows1[num].split(",", 1)
        assert cells[0] == str(num / fps) and (',%d,"' % num) in rows1[num]
        idx, prob = _want_emotions(num, num % 3)
        assert rows1[num].endswith(',"%s","%s"\n' % (idx, prob)), rows1[num]
        assert seen1[num] == (idx, prob, num % 3)
    want = "".join(rows1[k] for k in sorted(rows1))
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 20000 + (os.getpid() % 2000) + n_total + 100 * bool(sampled) + 200 * bool(cap) + 400 * (sampled == "iter") + 800 * n_frames
    procs = [ctx.Process(target=_emo_worker, args=(r, 2, port, q, n_total, n_frames, cap, sampled)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=180) for _ in range(2))
    for p in procs:
        p.join(60)
    batches = [numbers[i:i + n_frames] for i in range(0, len(numbers), n_frames)]
    for r in range(2):
        own = [n for b in batches[r::2] for n in b]
        assert res[r][1] == res[r][2] == len(own)                # .reads: the sampled frames of its own batches only
        assert sorted(res[r][3]) == own and all(res[r][3][n] == seen1[n] for n in own)
    assert len(batches) % 2 == 1                                 # rank 1 has no batch in the last round
    assert res[0][4] == want


def test_stream_without_emotions_is_the_parents():
    """emotions=0: the 517-wide path -- tickets without emo_* attributes, no keyword handed to the callbacks, and the
    rows the parent's run_stream produced (the literals tests/test_host_logic.py pins)"""
    from vn_celeb_face_recognition_amd.video import FrameSource, run_stream
    frames = _frames_for(23)
    calls = []
    rows0, _ = run_stream(FrameSource(frames, 25.0), _StubPipe(), 4, 0, 1, device="cpu", emotions=0,
                          on_frame=lambda *a, **kw: calls.append((len(a), kw)))
    rows_default, _ = run_stream(FrameSource(frames, 25.0), _StubPipe(), 4, 0, 1, device="cpu")
    assert rows0 == rows_default and calls and all(c == (4, {}) for c in calls)
    assert rows0[5] == '0.2,"[\'n5\', \'n5\']",5,"[[%s, 0.0, %s, 5.0], [%s, 0.25, %s, 5.25]]"\n' % (5 / 6, 15 / 6, 5 / 6, 15 / 6)
    assert rows0[3] == '0.12,"[]",3,"[]"\n'
    with pytest.raises(AttributeError):                          # asking for emotions a pipe does not produce is an error
        run_stream(FrameSource(frames, 25.0), _StubPipe(), 4, 0, 1, device="cpu", emotions=K)
    with pytest.raises(ValueError):
        run_stream(FrameSource(frames, 25.0), _EmoPipe(), 4, 0, 1, device="cpu", emotions=17)
    big = _EmoPipe()
    big.emotion = type("M", (), {"num_classes": 1 << 24})()
    with pytest.raises(ValueError, match="2\\^24"):
        run_stream(FrameSource(frames, 25.0), big, 4, 0, 1, device="cpu", emotions=K)


def test_sampled_source_reads_only_what_it_keeps():
    from vn_celeb_face_recognition_amd.video import FrameSource
    frames = _frames_for(23)
    loads = []

    def load(f):
        loads.append(int(f[0, 0, 0]))
        return f
    kept = [n for n in range(1, 24) if _keep(n)]
    assert kept == [1, 3, 5, 7, 9, 11, 13, 15, 17, 19, 21, 23]
    src = FrameSource(frames, 4.0, load=load, keep=_keep)
    assert src.total == 12 and [src.number_of(i) for i in range(12)] == kept
    got = list(src.rank_batches(5))
    assert [b for b, _, _ in got] == [0, 1, 2] and [len(q) for _, q, _ in got] == [5, 5, 2]
    assert [i for _, _, inf in got for i in inf] == [[n / 4.0, n] for n in kept]
    assert src.reads == 12 and loads == kept                     # frame i holds i in its first channel
    for r in range(2):
        s = FrameSource(frames, 4.0, keep=_keep)
        mine = list(s.rank_batches(5, r, 2))
        assert [b for b, _, _ in mine] == ([0, 2] if r == 0 else [1])
        assert s.reads == sum(len(q) for _, q, _ in mine) == (7 if r == 0 else 5)
        assert all(int(f[0, 0, 0]) == n for _, q, inf in mine for f, (_, n) in zip(q, inf))
    # compressed access asks for the kept frames alone
    asked = []

    def jpeg_bytes(i):
        asked.append(i + 1)
        return None                                              # "not a JPEG": the batch falls back to decoding
    s = FrameSource(frames, 4.0, compressed=jpeg_bytes, keep=_keep)
    first = next(s.rank_batches(5, compressed=True))
    assert asked == [1] and [n for _, n in first[2]] == kept[:5]
    # a decoder (plain iterator): every frame is pulled, the kept ones are counted and numbered
    it = FrameSource(iter(list(frames)), 4.0, keep=_keep)
    got_it = list(it.rank_batches(5))
    assert [i for _, _, inf in got_it for i in inf] == [[n / 4.0, n] for n in kept]
    assert it.total == 12 and it.reads == 12 and [it.number_of(i) for i in range(12)] == kept
    # without `keep` nothing changes
    plain = FrameSource(frames, 25.0)
    assert plain.total == 23 and plain.number_of(4) == 5 and [len(q) for _, q, _ in plain.rank_batches(5)] == [5, 5, 5, 5, 3]
