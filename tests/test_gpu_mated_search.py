"""GPU: vnf_gallery_mated_search (csrc/gallery_mated.hip) and GalleryModel.mated_search against the float64 oracle
tests/gallery_calibration_oracle.py.

Scores are held to gallery_oracle.tol(dim) and the returned rows to the tolerant comparison (the oracle's float64 score of
the returned row is within tol of the oracle's best), so no near-tie is excluded; every returned row must satisfy its
column's label predicate and the exclusion exactly.  Bitwise claims (chunkings, batch position, a NaN neighbour, the
agreement with vnf_gallery_search) compare the int32 views.  Every raw call runs with guard bytes around its three outputs
and its workspace."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import gallery_calibration_oracle as gco
import gallery_oracle as go
from test_gpu_gallery import DEV, Guarded, RawGallery, _rows
from vn_celeb_face_recognition_amd import _lib
from vn_celeb_face_recognition_amd.gallery import GalleryModel

pytestmark = pytest.mark.gpu
INVALID, CAPACITY = -1, -4


@functools.lru_cache(maxsize=None)
def _case(G, dim=512):
    """G rows of 3..7 classes in random order, 37 probes with labels of the same classes (one of a label nobody carries),
    an exclusion per probe (a row of the probe's label where there is one, some -1), and the float64 scores."""
    rng = np.random.default_rng(500 + G + dim)
    nc = 3 + G % 5
    g, q = _rows(G, dim, 300 + G), _rows(37, dim, 9)
    labels = rng.integers(0, nc, G)
    ql = rng.integers(0, nc, 37)
    ql[11] = nc + 2
    excl = np.full(37, -1, np.int64)
    for f in range(37):
        mine = np.flatnonzero(labels == ql[f])
        if mine.size and f % 4:
            excl[f] = mine[rng.integers(0, mine.size)]
    s64 = go.scores(q, g)
    for a in (g, q, labels, ql, excl, s64):
        a.setflags(write=False)
    return g, labels, q, ql, excl, s64


def mated(rg, q, ql, excl=None, chunk_rows=0):
    """The C ABI with guards -> (idx, label, score), each (F,2) numpy."""
    qd = torch.from_numpy(np.array(q, np.float32)).to(DEV)
    f = qd.shape[0]
    qld = torch.from_numpy(np.asarray(ql).astype(np.int32)).to(DEV)
    exd = None if excl is None else torch.from_numpy(np.asarray(excl).astype(np.int32)).to(DEV)
    nbytes = rg.lib.vnf_gallery_mated_search_workspace_bytes(f, rg.size, chunk_rows)
    assert nbytes >= 8
    outs = [Guarded((f, 2), torch.int32), Guarded((f, 2), torch.int32), Guarded((f, 2), torch.float32)]
    ws = Guarded((nbytes,), torch.uint8)
    _lib.check(rg.lib.vnf_gallery_mated_search(rg.h, ctypes.c_void_p(qd.data_ptr()), ctypes.c_void_p(qld.data_ptr()),
                                               None if exd is None else ctypes.c_void_p(exd.data_ptr()), f,
                                               *[ctypes.c_void_p(o.t.data_ptr()) for o in outs], chunk_rows,
                                               ctypes.c_void_p(ws.t.data_ptr()), nbytes, _lib.current_stream_ptr()))
    torch.cuda.synchronize()
    assert all(o.intact() for o in outs) and ws.intact(), "guard bytes overwritten"
    return tuple(o.t.cpu().numpy() for o in outs)


def check(got, s64, labels, ql, excl, t):
    """Predicates exactly, scores and rows tolerantly; absent candidates exactly.  Returns the largest score error."""
    idx, lab, sc = got
    oi, _, osc = gco.mated(s64, labels, ql, excl)
    assert idx.shape == lab.shape == sc.shape == (s64.shape[0], 2)
    worst = 0.0
    for f in range(s64.shape[0]):
        for col in (0, 1):
            j = int(idx[f, col])
            if oi[f, col] < 0:
                assert j == -1 and lab[f, col] == -1 and sc[f, col] == -np.inf, (f, col, j, sc[f, col])
                continue
            assert 0 <= j < s64.shape[1] and lab[f, col] == labels[j], (f, col, j)
            if col == 0:
                assert labels[j] == ql[f] and (excl is None or j != excl[f]), (f, j)
            else:
                assert labels[j] != ql[f], (f, j)
            err = abs(float(sc[f, col]) - osc[f, col])
            worst = max(worst, err)
            assert err <= t, (f, col, float(sc[f, col]), osc[f, col])
            assert s64[f, j] >= osc[f, col] - t, (f, col, j, s64[f, j], osc[f, col])
    return worst


def _same(a, b):
    return all(np.array_equal(x.view(np.int32), y.view(np.int32)) for x, y in zip(a, b))


@pytest.mark.parametrize("G", [1, 15, 16, 17, 33, 1000])
def test_shapes_meet_the_oracle(G):
    g, labels, q, ql, excl, s64 = _case(G)
    rg = RawGallery(512).add(g, labels)
    worst = 0.0
    for F in (0, 1, 15, 17, 37):
        worst = max(worst, check(mated(rg, q[:F], ql[:F]), s64[:F], labels, ql[:F], None, go.tol(512)))
        worst = max(worst, check(mated(rg, q[:F], ql[:F], excl[:F]), s64[:F], labels, ql[:F], excl[:F], go.tol(512)))
    print("G=%d: max |score - float64 oracle| = %.3g (tol %.3g)" % (G, worst, go.tol(512)))
    rg.close()


def test_dim_32_has_no_hard_coded_stride():
    g, labels, q, ql, excl, s64 = _case(33, 32)
    rg = RawGallery(32).add(g, labels)
    for F in (0, 1, 15, 17, 37):
        for cr in (0, 16):
            check(mated(rg, q[:F], ql[:F], excl[:F], chunk_rows=cr), s64[:F], labels, ql[:F], excl[:F], go.tol(32))
    rg.close()


def test_chunkings_agree_bitwise():
    g, labels, q, ql, excl, s64 = _case(1000)
    rg = RawGallery(512).add(g, labels)
    for ex in (None, excl):
        base = mated(rg, q, ql, ex)
        check(base, s64, labels, ql, ex, go.tol(512))
        for cr in (16, 48, 96, 1000, 18):      # 18: chunks that do not begin on a multiple of 4
            assert _same(base, mated(rg, q, ql, ex, chunk_rows=cr)), cr
    rg.close()
    g, labels, q, ql, excl, s64 = _case(33)
    rg = RawGallery(512).add(g, labels)
    base = mated(rg, q, ql, excl)
    for cr in (16, 48, 96, 1000):
        assert _same(base, mated(rg, q, ql, excl, chunk_rows=cr)), cr
    rg.close()


def test_a_probe_alone_equals_the_probe_in_a_batch_bitwise():
    g, labels, q, ql, excl, _ = _case(1000)
    rg = RawGallery(512).add(g, labels)
    batch = mated(rg, q, ql, excl)
    for i in (0, 15, 16, 36):
        alone = mated(rg, q[i:i + 1], ql[i:i + 1], excl[i:i + 1])
        assert all(np.array_equal(a[0].view(np.int32), b[i].view(np.int32)) for a, b in zip(alone, batch)), i
    rg.close()


def test_a_nan_probe_leaves_the_others_alone():
    g, labels, q, ql, excl, _ = _case(1000)
    rg = RawGallery(512).add(g, labels)
    clean = q[:5].copy()
    dirty = clean.copy()
    dirty[2, 100] = np.nan
    a, b = mated(rg, clean, ql[:5], excl[:5]), mated(rg, dirty, ql[:5], excl[:5])
    for i in (0, 1, 3, 4):
        assert all(np.array_equal(x[i].view(np.int32), y[i].view(np.int32)) for x, y in zip(a, b)), i
    # NaN scores tie below every number: the first qualifying row of each kind
    first_m = [j for j in range(1000) if labels[j] == ql[2] and j != excl[2]][0]
    first_n = [j for j in range(1000) if labels[j] != ql[2]][0]
    assert b[0][2].tolist() == [first_m, first_n] and np.isnan(b[2][2]).all()
    rg.close()


@pytest.mark.parametrize("G", [1, 15, 16])
def test_columns_are_the_first_qualifying_entries_of_the_search(G):
    g, labels, q, ql, excl, _ = _case(G)
    rg = RawGallery(512).add(g, labels)
    si, sl, ss = rg.search(q, 16)
    for ex in (None, excl):
        mi, ml, ms = mated(rg, q, ql, ex)
        for f in range(37):
            want = [None, None]
            for r in range(16):
                j = int(si[f, r])
                if j < 0:
                    break
                col = 0 if labels[j] == ql[f] else 1
                if col == 0 and ex is not None and ex[f] == j:
                    continue
                if want[col] is None:
                    want[col] = r
            for col in (0, 1):
                if want[col] is None:
                    assert mi[f, col] == -1 and ml[f, col] == -1 and ms[f, col] == -np.inf
                else:
                    r = want[col]
                    assert (mi[f, col], ml[f, col]) == (si[f, r], sl[f, r]), (f, col)
                    assert ms[f, col:col + 1].view(np.int32)[0] == ss[f, r:r + 1].view(np.int32)[0], (f, col)
    rg.close()


def test_exact_ties_go_to_the_smaller_index_in_both_columns():
    g, labels, q, ql, excl, _ = _case(1000)
    g, labels = g.copy(), labels.copy()
    v = _rows(1, 512, 5)[0]
    g[3] = g[40] = g[7] = g[900] = v
    labels[3] = labels[40] = 1
    labels[7] = labels[900] = 2
    rg = RawGallery(512).add(g, labels)
    probes, pl = np.stack([v, v, v]), np.array([1, 2, 0])
    for cr in (0, 16):
        idx, lab, sc = mated(rg, probes, pl, chunk_rows=cr)
        assert idx[0].tolist() == [3, 7] and lab[0].tolist() == [1, 2]
        assert idx[1].tolist() == [7, 3] and lab[1].tolist() == [2, 1]
        assert idx[2, 1] == 3                                                       # label 0: all four are non-mates
        assert len(set(sc[:2].view(np.int32).reshape(-1).tolist())) == 1 and abs(sc[0, 0] - 1.0) <= go.tol(512)
        idx, _, sc2 = mated(rg, probes, pl, np.array([3, 7, 3]), chunk_rows=cr)     # the winner excluded: the next duplicate
        assert idx[0].tolist() == [40, 7] and idx[1].tolist() == [900, 3] and idx[2, 1] == 3
        assert np.array_equal(sc2[:2].view(np.int32), sc[:2].view(np.int32))
    rg.close()


def test_self_calibration_through_the_model():
    G = 150
    g = _rows(G, 512, 77)
    labels = np.random.default_rng(78).integers(0, 4, G)
    labels[labels == 3] = 0
    labels[60] = 3                                    # label 3 has one row
    s64 = go.scores(g, g)
    off = s64 - 2.0 * np.eye(G)
    assert off.max() < 1.0 - 4 * go.tol(512)          # every row is its own best match by a margin, on the CPU
    m = GalleryModel(512, max_batch=64).to(DEV).add(g, labels)      # three batches: exclude travels with its probes
    probes = torch.from_numpy(m._emb).to(DEV)
    idx, lab, sc = (t.cpu().numpy() for t in m.mated_search(probes, labels))
    assert idx.dtype == lab.dtype == np.int32 and sc.dtype == np.float32 and idx.shape == (G, 2)
    assert np.array_equal(idx[:, 0], np.arange(G)) and np.array_equal(lab[:, 0], labels) and np.abs(sc[:, 0] - 1).max() <= go.tol(512)
    check((idx, lab, sc), s64, labels, labels, None, go.tol(512))
    ex = np.arange(G)
    idx2, lab2, sc2 = (t.cpu().numpy() for t in m.mated_search(probes, torch.from_numpy(labels).to(DEV), torch.from_numpy(ex).to(DEV)))
    assert (idx2[:, 0] != ex).all()
    assert (idx2[60, 0], lab2[60, 0], sc2[60, 0]) == (-1, -1, -np.inf) and (idx2[np.arange(G) != 60, 0] >= 0).all()
    assert np.array_equal(idx2[:, 1], idx[:, 1]) and np.array_equal(sc2[:, 1].view(np.int32), sc[:, 1].view(np.int32))   # column 1 ignores exclude
    check((idx2, lab2, sc2), s64, labels, labels, ex, go.tol(512))
    m.chunk_rows = 48
    assert _same((idx2, lab2, sc2), tuple(t.cpu().numpy() for t in m.mated_search(probes, labels, ex)))
    one = GalleryModel(512).to(DEV).add(g[:20], np.full(20, 6))
    idx, lab, sc = (t.cpu().numpy() for t in one.mated_search(probes[:20], np.full(20, 6), np.arange(20)))
    assert (idx[:, 1] == -1).all() and (lab[:, 1] == -1).all() and np.isneginf(sc[:, 1]).all() and (idx[:, 0] >= 0).all()


def test_the_model_refuses_what_search_refuses_and_bad_labels():
    g, labels, q, ql, excl, _ = _case(33)
    m = GalleryModel(512).to(DEV).add(g, labels)
    qd = torch.from_numpy(q.copy()).to(DEV)
    with pytest.raises(ValueError, match="empty"):
        GalleryModel(512).to(DEV).mated_search(qd, ql)
    with pytest.raises(RuntimeError, match="cuda"):
        m.mated_search(qd.cpu(), ql)
    with pytest.raises(ValueError, match="expected"):
        m.mated_search(qd[:, :256], ql)
    with pytest.raises(ValueError, match="labels"):
        m.mated_search(qd, ql[:36])
    with pytest.raises(ValueError, match="labels"):
        m.mated_search(qd, ql.astype(np.float32))
    with pytest.raises(ValueError, match="labels"):
        m.mated_search(qd, torch.from_numpy(ql.astype(np.float64)))
    with pytest.raises(ValueError, match="exclude"):
        m.mated_search(qd, ql, excl[:5])
    with pytest.raises(ValueError, match="exclude"):
        m.mated_search(qd, ql, excl.astype(np.float64))
    idx, _, _ = m.mated_search(qd[:0], ql[:0])
    assert idx.shape == (0, 2)


def test_error_codes():
    g, labels, q, ql, excl, _ = _case(33)
    rg = RawGallery(512).add(g, labels)
    lib = rg.lib
    qd = torch.from_numpy(np.concatenate([q[:4].reshape(-1), np.zeros(4, np.float32)])).to(DEV)
    qld = torch.from_numpy(ql[:4].astype(np.int32)).to(DEV)
    out = [torch.empty((8,), dtype=torch.int32, device=DEV) for _ in range(3)]
    need = lib.vnf_gallery_mated_search_workspace_bytes(4, 33, 16)
    assert need == 3 * 4 * 2 * 8                       # three chunks of 16 rows, 2 F keys each
    ws = torch.empty((need + 8,), dtype=torch.uint8, device=DEV)
    P = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)

    def call(qp=P(qd), lp=P(qld), o0=P(out[0]), o1=P(out[1]), o2=P(out[2]), wp=P(ws), nbytes=need, F=4):
        return lib.vnf_gallery_mated_search(rg.h, qp, lp, None, F, o0, o1, o2, 16, wp, nbytes, None)

    assert call() == 0
    for kw in ("qp", "lp", "o0", "o1", "o2", "wp"):
        assert call(**{kw: None}) == INVALID, kw
    assert call(qp=P(qd, 4)) == INVALID                # q_dev not 16-byte aligned
    assert call(wp=P(ws, 4)) == INVALID                # workspace not 8-byte aligned
    assert call(F=-1) == INVALID
    assert call(nbytes=need - 8) == CAPACITY
    assert call(F=0, qp=None, wp=None, nbytes=0) == 0  # F == 0: a no-op before any pointer is looked at
    assert lib.vnf_gallery_mated_search(None, P(qd), P(qld), None, 4, P(out[0]), P(out[1]), P(out[2]), 16, P(ws), need, None) == INVALID
    assert lib.vnf_gallery_mated_search_workspace_bytes(-1, 33, 0) == INVALID
    assert lib.vnf_gallery_mated_search_workspace_bytes(4, 33, -1) == INVALID
    assert lib.vnf_gallery_mated_search_workspace_bytes(0, 33, 0) == 8
    torch.cuda.synchronize()
    rg.close()
