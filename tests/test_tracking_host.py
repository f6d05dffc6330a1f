"""CPU: the host side of the face tracks.  The oracle (tests/track_oracle.py) on hand-made cases whose answer is written
out here, tracking.pool_tracks / name_tracks / the argument checks of link_tracks, video.run_stream(faces=...) on the CPU
stand-ins of test_host_logic.py on one rank and on two gloo ranks, the tracker's Track column, and the two entries'
declarations."""
import os
import re
import sys

import numpy as np
import pytest
import torch

import gallery_oracle as go
import track_oracle as to
from conftest import REPO
from test_host_logic import _StubPipe, _frames_for
from vn_celeb_face_recognition_amd import tracking

T = 0.5


def _scores(n, pairs):
    s = np.full((n, n), 0.1)
    np.fill_diagonal(s, 1.0)
    for (i, j), v in pairs.items():
        s[i, j] = s[j, i] = v
    return s


# ------------------------------------------------------------------------------------------------ the oracle
def test_oracle_a_chain_over_three_frames():
    o = to.link_scores(_scores(3, {(0, 1): 0.9, (1, 2): 0.8, (0, 2): 0.95}), [0, 1, 2], None, T, 0.0, 1)
    assert o.next.tolist() == [1, 2, -1] and o.prev.tolist() == [-1, 0, 1] and o.track.tolist() == [0, 0, 0] and o.n_tracks == 1
    assert o.link_score.tolist() == [-np.inf, 0.9, 0.8]
    assert o.margin_t == pytest.approx(0.3) and o.margin_iou == np.inf and o.margin_lead == np.inf    # (0, 2) is out of the window


def test_oracle_two_people_crossing():
    # frame 0: A, B; frame 1: B', A' -- the order inside a frame means nothing
    o = to.link_scores(_scores(4, {(0, 3): 0.9, (1, 2): 0.85, (0, 2): 0.55, (1, 3): 0.6}), [0, 0, 1, 1], None, T, 0.0, 1)
    assert o.next.tolist() == [3, 2, -1, -1] and o.prev.tolist() == [-1, -1, 1, 0] and o.track.tolist() == [0, 1, 1, 0]
    assert o.margin_lead == pytest.approx(0.25) and o.margin_t == pytest.approx(0.05)


def test_oracle_a_best_that_is_not_mutual_links_nothing():
    # frame 0: A, C; frame 1: B.  A's best is B, but B's best predecessor is C
    o = to.link_scores(_scores(3, {(0, 2): 0.8, (1, 2): 0.9}), [0, 0, 1], None, T, 0.0, 1)
    assert o.next.tolist() == [-1, 2, -1] and o.prev.tolist() == [-1, -1, 1] and o.track.tolist() == [0, 1, 1] and o.n_tracks == 2
    assert o.margin_lead == pytest.approx(0.1)


def test_oracle_a_gap_is_bridged_by_max_gap_2_only():
    s = _scores(2, {(0, 1): 0.9})
    assert to.link_scores(s, [0, 2], None, T, 0.0, 2).track.tolist() == [0, 0]
    o = to.link_scores(s, [0, 2], None, T, 0.0, 1)
    assert o.track.tolist() == [0, 1] and o.margin_t == np.inf                   # no pair in the window at all


def test_oracle_the_nearest_frame_wins_over_a_better_score_farther_away():
    o = to.link_scores(_scores(3, {(0, 1): 0.6, (0, 2): 0.95, (1, 2): 0.1}), [0, 1, 2], None, T, 0.0, 2)
    assert o.next.tolist() == [1, -1, -1] and o.prev.tolist() == [-1, 0, -1] and o.track.tolist() == [0, 0, 1]
    assert o.margin_lead == np.inf                                               # the runners-up are at another distance


def test_oracle_rows_of_one_frame_are_never_linked():
    o = to.link_scores(_scores(2, {(0, 1): 1.0}), [0, 0], None, 0.0, 0.0, 4)
    assert o.next.tolist() == [-1, -1] and o.n_tracks == 2


def test_oracle_boxes_and_nan():
    boxes = np.array([[0, 0, 10, 10], [5, 0, 15, 10], [20, 0, 30, 10]], np.float32)      # IoU(0,1) = 1/3, IoU(0,2) = 0
    assert to.overlap(boxes[0], boxes[1]) == (50.0, 150.0)
    s = _scores(3, {(0, 1): 0.9, (0, 2): 0.95})
    o = to.link_scores(s, [0, 1, 1], boxes, T, 0.3, 1)
    assert o.next.tolist() == [1, -1, -1] and o.margin_iou == pytest.approx(min(50 / 150 - 0.3, 0.3))
    assert to.link_scores(s, [0, 1, 1], boxes, T, 0.0, 1).next.tolist() == [2, -1, -1]
    s[0, 2] = s[2, 0] = np.nan
    o = to.link_scores(s, [0, 1, 1], None, T, 0.0, 1)
    assert o.next.tolist() == [1, -1, -1] and o.margin_t == pytest.approx(0.4)


def test_oracle_sequential_sums_are_fp32_in_row_order():
    x = np.array([[1.0, 2.0 ** -24], [2.0 ** -24, 1.0], [2.0 ** -24, 2.0 ** -24]], np.float32)
    sums, counts = to.sequential_sums(x, [0, 1, 0], 2)
    assert counts.tolist() == [2, 1] and sums.dtype == np.float32
    assert sums[0].tolist() == [1.0, 2.0 ** -23] and sums[1].tolist() == [2.0 ** -24, 1.0]    # 1 + 2^-24 rounds to 1


# ------------------------------------------------------------------------------------------------ tracking.py
def _result(emb, track):
    track = np.asarray(track, np.int32)
    n = int(track.max()) + 1
    unit = go.normalize(emb).astype(np.float32)
    sums, counts = to.sequential_sums(unit, track, n)
    z = np.full(track.shape, -1, np.int32)
    return tracking.TrackResult(track, z, z, np.zeros(track.shape, np.float32), n, sums, counts.astype(np.int32))


def test_pool_tracks_rules():
    rng = np.random.default_rng(3)
    emb = rng.standard_normal((6, 32)).astype(np.float32) * np.array([[1], [20], [3], [5], [7], [0.5]], np.float32)
    res = _result(emb, [0, 1, 0, 2, 0, 2])
    pooled = tracking.pool_tracks(emb, res)
    assert pooled.dtype == np.float32 and pooled.shape == (3, 32)
    assert np.array_equal(pooled[1].view(np.int32), emb[1].view(np.int32))       # a track of one face: as it is, bit for bit
    for k, members in ((0, [0, 2, 4]), (2, [3, 5])):
        want_dir = go.normalize(go.normalize(emb[members]).sum(axis=0, keepdims=True))[0]
        want_len = np.linalg.norm(emb[members].astype(np.float64), axis=1).mean()
        assert np.linalg.norm(pooled[k]) == pytest.approx(want_len, rel=1e-6)
        assert np.abs(pooled[k] / np.linalg.norm(pooled[k]) - want_dir).max() < 1e-6
    unit = go.normalize(emb).astype(np.float32)                                  # unit rows (InceptionResnetV1): a unit template
    pooled = tracking.pool_tracks(unit, _result(unit, [0, 1, 0, 2, 0, 2]))
    assert np.abs(np.linalg.norm(pooled, axis=1) - 1.0).max() < 1e-6
    with pytest.raises(ValueError):
        tracking.pool_tracks(emb[:5], res)


class _StubClassifier:
    num_classes = 4
    device = "cpu"

    def __init__(self):
        self.calls = []

    def classify(self, emb, want_logp=True):
        self.calls.append((tuple(emb.shape), emb.dtype, want_logp))
        return None, emb[:, 0].to(torch.int32), emb[:, 1]


def test_name_tracks_classifies_then_identifies():
    label2name = {"label": [0, 1, 2, 3], "name": ["a", "b", "c", "d"]}
    pooled = np.zeros((3, 16), np.float32)
    pooled[:, 0], pooled[:, 1] = [2, 0, 3], [0.9, 0.4, 0.6]
    c = _StubClassifier()
    assert tracking.name_tracks(pooled, c, label2name, 0.5) == ["c", "Unknown", "d"]
    assert c.calls == [((3, 16), torch.float32, False)]
    assert tracking.name_tracks(pooled, c, label2name, {"0": 0.3, "2": 0.95, "3": 0.5}) == ["Unknown", "a", "d"]
    assert tracking.name_tracks(np.zeros((0, 16), np.float32), c, label2name, 0.5) == [] and len(c.calls) == 2


def test_link_tracks_refuses_before_it_touches_a_device():
    emb = np.zeros((3, 32), np.float32)
    ok = dict(threshold=0.5, device="cuda:0")
    bad = [((emb, [0, 2, 1]), ok, "sorted"), ((emb, [0, 1]), ok, "ordinals"), ((emb, [0.0, 1.0, 2.0]), ok, "integer"),
           ((emb, [-1, 0, 1]), ok, "lie in"), ((np.zeros((3, 20), np.float32), [0, 1, 2]), ok, "multiple of 16"),
           ((emb, [0, 1, 2]), dict(ok, threshold=float("nan")), "NaN"), ((emb, [0, 1, 2]), dict(ok, min_iou=float("nan")), "NaN"),
           ((emb, [0, 1, 2]), dict(ok, max_gap=0), "max_gap"), ((emb, [0, 1, 2]), dict(ok, max_gap=256), "max_gap"),
           ((emb, [0, 1, 2]), dict(ok, max_gap=1.5), "max_gap"), ((emb, [0, 1, 2], np.zeros((2, 4))), ok, "boxes"),
           ((emb, [0, 1, 2]), dict(ok, min_iou=0.3), "needs the boxes"),
           ((emb, [0, 1, 2], np.full((3, 4), np.inf)), ok, "non-finite")]
    for args, kw, msg in bad:
        with pytest.raises(ValueError, match=msg):
            tracking.link_tracks(*args, **kw)
    with pytest.raises(RuntimeError, match="no CPU path"):
        tracking.link_tracks(emb, [0, 1, 2], threshold=0.5, device="cpu")
    assert tracking.frame_first([0, 0, 2, 2, 2, 3], 5).tolist() == [0, 2, 2, 5, 6, 6]


# ------------------------------------------------------------------------------------------------ the stream's sink
def _stream(rank, world, n_total, n_frames, cap, sink):
    from vn_celeb_face_recognition_amd.video import FrameSource, run_stream
    got = []

    def faces(number, tm, box, emb):
        assert emb.dtype == np.float32 and emb.shape == (512,) and box.dtype == np.float32 and box.shape == (4,)
        got.append((int(number), float(tm), [float(v) for v in box], float(emb[0]), float(np.abs(emb[1:]).max())))
    kw = {"faces": faces} if sink else {}
    rows, _ = run_stream(FrameSource(_frames_for(n_total), 25.0), _StubPipe(), n_frames, rank, world, device="cpu", cap=cap, **kw)
    return rows, got


def _want_faces(n_total):
    """what _StubPipe puts into frame i: i % 3 faces, embedding (i, 0, ...), box (i, k, i + 10, k + 20)"""
    return sorted((i, i / 25.0, [float(i), float(k), i + 10.0, k + 20.0], float(i), 0.0) for i in range(1, n_total + 1) for k in range(i % 3))


def _sink_worker(rank, world, port, q, n_total, n_frames, cap):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    sys.path.insert(0, REPO)
    import torch.distributed as dist
    from vn_celeb_face_recognition_amd import dist as vdist
    vdist.init_from_env("gloo")
    rows, got = _stream(rank, world, n_total, n_frames, cap, True)
    q.put((rank, got, "".join(rows[k] for k in sorted(rows)) if rank == 0 else ""))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("n_total,n_frames,cap", [(19, 4, None), (23, 4, 2)])       # cap 2: the follow-up gather carries faces too
def test_stream_hands_every_face_to_the_sink_once(n_total, n_frames, cap):
    import torch.multiprocessing as mp
    plain, none = _stream(0, 1, n_total, n_frames, cap, False)
    rows1, got1 = _stream(0, 1, n_total, n_frames, cap, True)
    assert none == [] and rows1 == plain                                          # the rows do not see the sink
    assert sorted(got1) == _want_faces(n_total) and len(got1) == sum(i % 3 for i in range(1, n_total + 1))
    for num in range(1, n_total + 1):                                             # inside a frame: the order of the tracker row
        assert [g[2][1] for g in got1 if g[0] == num] == [float(k) for k in range(num % 3)]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 24000 + (os.getpid() % 2000) + n_total + 200 * bool(cap)
    procs = [ctx.Process(target=_sink_worker, args=(r, 2, port, q, n_total, n_frames, cap)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=180) for _ in range(2))
    for p in procs:
        p.join(60)
    assert res[1][1] == []                                                        # rank 0 alone feeds the sink
    assert sorted(res[0][1]) == _want_faces(n_total)                              # its own frames and the other rank's alike
    for num in range(1, n_total + 1):
        assert [g[2][1] for g in res[0][1] if g[0] == num] == [float(k) for k in range(num % 3)]
    assert res[0][2] == "".join(plain[k] for k in sorted(plain))                  # byte-identical rows


# ------------------------------------------------------------------------------------------------ the tracker file
def test_the_track_column_round_trips(tmp_path):
    from vn_celeb_face_recognition_amd import statistics as st
    assert st.tracker_header(True, False) == ['Time', 'Names', 'Frame_idx', 'Bboxes']          # unchanged without the flag
    assert st.tracker_header(True, True, True) == ['Time', 'Names', 'Frame_idx', 'Bboxes', 'Emotion', 'Track']
    assert st.tracker_header(True, track_faces=True)[-1] == 'Track'
    box = [[10.0, 20.0, 30.0, 40.0], [50.0, 20.0, 70.0, 40.0]]
    plain = st.tracker_row(0.5, ["a", "b"], 3, box, (100, 200), True)
    tracked = st.tracker_row(0.5, ["a", "b"], 3, box, (100, 200), True, tracks=np.array([4, 0], np.int32))
    assert tracked == plain[:-1] + ',"[4, 0]"\n'
    path = str(tmp_path / "tracker.csv")
    lines = [st.tracker_row(0.5 * i, ["a", "b"] if i % 2 else [], i, box if i % 2 else [], (100, 200), True,
                            tracks=[i // 2, 7] if i % 2 else []) for i in range(1, 7)]
    with open(path, "w") as fp:
        fp.write(",".join(st.tracker_header(True, track_faces=True)) + "\n" + "".join(lines))
    df = st.read_tracker_csv(path)
    assert list(df) == ['Time', 'Names', 'Frame_idx', 'Bboxes', 'Track']
    assert df['Track'] == ['[0, 7]', '[]', '[1, 7]', '[]', '[2, 7]', '[]'] and df['Names'][0] == "['a', 'b']"
    out = st.export_json_stat_dynamic_itv(df, str(tmp_path / "t.json"), 2, n_appear=1, log=False)
    assert sorted(out["1"]["celebrities"]) == ["a", "b"] and len(out["2"]["celebrities"]["a"]) == 1
    without = {k: v for k, v in df.items() if k != 'Track'}                      # the statistics do not read the column
    assert st.export_json_stat_dynamic_itv(without, str(tmp_path / "u.json"), 2, n_appear=1, log=False) == out


def test_header_declares_and_signatures_bind_both_entries():
    from vn_celeb_face_recognition_amd import _lib
    hdr = open(os.path.join(REPO, "include", "vnface.h")).read()
    declared = set(re.findall(r"\b(vnf_[a-z0-9_]+)\s*\(", hdr))
    for name, nargs in (("vnf_gallery_tracks", 15), ("vnf_gallery_track_sums", 8), ("vnf_gallery_tracks_workspace_bytes", 1)):
        assert name in declared and name in _lib.SIGNATURES
        proto = re.search(r"^int(?:64_t)? %s\(([^;]*)\);" % name, hdr, re.M).group(1)
        assert len(proto.split(",")) == nargs == len(_lib.SIGNATURES[name][1]), name
